"""The teacher-free ABMIL step behind the C-ABI (mhimx_pure_step_run) against the Python orchestration of FusedTrainer(model="mhim_pure"),
eager and as a replayed hipGraph, on three legs:
  sizes200   200 device-resident bags of 200 distinct sizes, 9 000 .. 59 745 rows (the sizes DESIGN section 5 used for mhim): nothing repeats
  c1         512 x 1024, 8 rotating bags (BASELINE config c1)
  n10000     10 000 x 1024, 8 rotating bags
The routes are alternated ROUNDS times in one process; every figure is ms per step over a window of at least WINDOW_S seconds that ends in
a device synchronise; per route the median and min .. max over the rounds are reported (one JSON line at the end).
    python tools/exp_pure_step.py            (MHIMX_STEP_EXEC=0 in the environment turns the "exec" routes into the Python route too)"""
import json, os, random, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mhim_mil_amd import synth
from mhim_mil_amd.mhim import MHIM
from mhim_mil_amd.engine import FusedTrainer

D = 1024
ROUNDS = int(os.environ.get("ROUNDS", 5))
WINDOW_S = float(os.environ.get("WINDOW_S", 0.6))
NB = int(os.environ.get("NB", 200))
dev = torch.device("cuda", 0)
base = synth.mhim_state(7, input_dim=D, merge_enable=False)


def trainer(executor):
    m = MHIM(input_dim=D, n_classes=2, baseline="attn", act="gelu", da_act="relu", merge_enable=False, dropout=0.25)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in base.items()})
    tr = FusedTrainer(m.to(dev).train(), None, model="mhim_pure")
    tr.use_executor = bool(executor) and tr.use_executor
    return tr


def window(step_fns):
    """ms per step of calling every function of step_fns in turn, over and over, for at least WINDOW_S seconds (device-complete)."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for f in step_fns:
            f()
        n += len(step_fns)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= WINDOW_S:
            return dt / n * 1e3


g = torch.Generator(device=dev); g.manual_seed(5)
sizes = [9000 + 255 * j for j in range(NB)]
random.Random(3).shuffle(sizes)
x0 = torch.randn(max(sizes), D, device=dev, generator=g).abs_()
label = torch.tensor([1], device=dev)
legs = {"sizes200": [x0[:n] for n in sizes],
        "c1": [torch.randn(512, D, device=dev, generator=g).abs_() for _ in range(8)],
        "n10000": [torch.randn(10000, D, device=dev, generator=g).abs_() for _ in range(8)]}
sample = legs["sizes200"][::10]                                   # the sizes whose steps are also captured and replayed

tr_c, tr_p = trainer(True), trainer(False)
routes = {}
for leg, bags in legs.items():
    routes[leg, "exec_eager"] = [lambda b=b: tr_c.train_step(b, label) for b in bags]
    routes[leg, "python_eager"] = [lambda b=b: tr_p.train_step(b, label) for b in bags]
routes["sizes200", "exec_eager_sample"] = [lambda b=b: tr_c.train_step(b, label) for b in sample]
# replayed graphs: one trainer per route and leg (a graph's buffers are its own)
graphs = {}
for name, ex in (("exec_replay", True), ("python_replay", False)):
    for leg, bags in (("sizes200", sample), ("c1", legs["c1"][:1]), ("n10000", legs["n10000"][:1])):
        tr = trainer(ex)
        graphs[leg, name] = (tr, [tr.capture(b, label, warmup=1) for b in bags])
        routes[leg, name if leg != "sizes200" else name + "_sample"] = [gr.replay for gr in graphs[leg, name][1]]
for fns in routes.values():                                        # warm every shape of every route
    for f in fns:
        f()
torch.cuda.synchronize()
assert tr_c.last.get("exec") == tr_c.use_executor and tr_p.last.get("exec") is False

ms = {k: [] for k in routes}
for r in range(ROUNDS):
    for k, fns in routes.items():
        ms[k].append(window(fns))
out = {"rounds": ROUNDS, "window_s": WINDOW_S, "executor": bool(tr_c.use_executor),
       "mean_rows_sizes200": sum(sizes) / len(sizes), "ms_per_step": {}}
for (leg, name), v in ms.items():
    out["ms_per_step"][f"{leg}.{name}"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(f"{leg:9s} {name:22s} median {statistics.median(v):.4f} ms/step   min {min(v):.4f} .. max {max(v):.4f}")
med = lambda k: out["ms_per_step"][k]["median"]
out["ratios"] = {
    "sizes200.exec_eager/python_eager": round(med("sizes200.exec_eager") / med("sizes200.python_eager"), 4),
    "c1.exec_eager/python_eager": round(med("c1.exec_eager") / med("c1.python_eager"), 4),
    "n10000.exec_eager/python_eager": round(med("n10000.exec_eager") / med("n10000.python_eager"), 4),
    "sizes200_sample.exec_eager/exec_replay": round(med("sizes200.exec_eager_sample") / med("sizes200.exec_replay_sample"), 4),
    "c1.exec_eager/exec_replay": round(med("c1.exec_eager") / med("c1.exec_replay"), 4),
    "n10000.exec_eager/exec_replay": round(med("n10000.exec_eager") / med("n10000.exec_replay"), 4),
}
print(json.dumps(out))
