"""Accumulation windows of the full MHIM(ABMIL) model: FusedTrainer(model="mhim", accumulation_steps=k).window_step timed on
  A   8 bags per window, sizes log-uniform in 500 .. 30 000 rows (fixed seed), 6 rotating windows
  B   8 bags of 10 000 rows: window_step (mhimx_window_run) against the same window forced through mhimx_ragged_window_run
      (route names "<route>" and "<route>+forced"; the second exists only where the checkout has the ragged call) - the price of raggedness
  C   32 bags per window, sizes uniform in 64 .. 2 000 rows (fixed seed), 4 rotating windows
D = 1024, dropout 0.25, the V2 recipe.  One invocation times ROUNDS windows of at least WINDOW_S seconds per leg (each ends in a device
synchronise) and prints one JSON line {"route": ..., "ms_per_bag": {leg: [..]}, "exec": {leg: route name}}.  To compare two checkouts, run
this file from each of them alternately (REPO=<checkout> selects the package that is imported; the route is whatever that checkout's
window_step does: before mhimx_ragged_window_run existed, the bags on HIP streams from Python) and summarise the collected lines:
    python tools/exp_ragged_window.py --summarize new.jsonl parent.jsonl
which prints median and min .. max per leg and route and says whether the ranges overlap."""
import json, math, os, random, statistics, sys, time

if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
    res = {}
    for path in sys.argv[2:]:
        for line in open(path):
            line = line.strip()
            if line.startswith("{"):
                d = json.loads(line)
                for leg, v in d["ms_per_bag"].items():
                    res.setdefault(leg.split("+")[0], {}).setdefault(d["route"] + ("+forced" if "+" in leg else ""), []).extend(v)
    for leg, routes in sorted(res.items()):
        for route, v in sorted(routes.items()):
            print(f"{leg:3s} {route:14s} n={len(v)}  median {statistics.median(v):.4f} ms/bag   min {min(v):.4f} .. max {max(v):.4f}")
        names = sorted(routes)
        for i, ra in enumerate(names):
            for rb in names[i + 1:]:
                a, b = routes[ra], routes[rb]
                apart = max(a) < min(b) or max(b) < min(a)
                print(f"{leg:3s} {ra} / {rb}: ranges {'do NOT overlap' if apart else 'OVERLAP'}; median ratio {statistics.median(a) / statistics.median(b):.3f}")
    sys.exit(0)

sys.path.insert(0, os.environ.get("REPO") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mhim_mil_amd import synth
from mhim_mil_amd.mhim import MHIM
from mhim_mil_amd.engine import FusedTrainer

D = 1024
ROUNDS = int(os.environ.get("ROUNDS", 5))
WINDOW_S = float(os.environ.get("WINDOW_S", 0.6))
LEGS = os.environ.get("LEGS", "A,B,C").split(",")
dev = torch.device("cuda", 0)
CFG = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999,
           merge_ratio=0.9, temp_t=0.1, dropout=0.25)
base = synth.mhim_state(7, input_dim=D, merge_k=5)


def trainer(accum):
    def mk(sd):
        m = MHIM(input_dim=D, n_classes=2, baseline="attn", **CFG)
        sd = dict(sd)
        sd["merge.global_q"] = sd["merge.global_q_mm"]
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        m = m.to(dev).train()
        m.merge.dropout = 0.0
        return m
    return FusedTrainer(mk(base), mk(synth.spread_teacher(base)), aux_alpha=0.5, mm=0.9997, accumulation_steps=accum)


def timed(fns, bags_per_call):
    """ms per bag of calling every function of fns in turn, over and over, for at least WINDOW_S seconds (device-complete)."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for f in fns:
            f()
        n += len(fns) * bags_per_call
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= WINDOW_S:
            return dt / n * 1e3


g = torch.Generator(device=dev); g.manual_seed(5)
rnd = random.Random(3)
big = [int(round(math.exp(rnd.uniform(math.log(500), math.log(30000))))) for _ in range(48)]
small = [rnd.randint(64, 2000) for _ in range(128)]
x0 = torch.randn(30000, D, device=dev, generator=g).abs_()
labels = [torch.tensor([j % 2], device=dev) for j in range(32)]
windows = {
    "A": (8, [[x0[:n] for n in big[w:w + 8]] for w in range(0, 48, 8)]),
    "B": (8, [[torch.randn(10000, D, device=dev, generator=g).abs_() for _ in range(8)]]),
    "C": (32, [[x0[:n] for n in small[w:w + 32]] for w in range(0, 128, 32)]),
}
out = {"route": os.environ.get("ROUTE_NAME", "new"), "rounds": ROUNDS, "window_s": WINDOW_S, "ms_per_bag": {}, "exec": {},
       "sizes": {"A": big, "C": small}}
for leg in LEGS:
    k, wins = windows[leg]
    tr = trainer(k)
    forms = {leg: [lambda w=w, k=k: tr.window_step(w, labels[:k]) for w in wins]}
    if leg == "B" and hasattr(tr, "_exec_ragged_window"):
        assert tr._ragged_window_ok(wins[0], labels[:k])
        forms["B+forced"] = [lambda w=w, k=k: tr._exec_ragged_window(w, labels[:k], None, True) for w in wins]
    for name, fns in forms.items():                                    # warm every shape
        for f in fns:
            f()
        torch.cuda.synchronize()
        out["exec"][name] = str(tr.last.get("exec"))
        out["ms_per_bag"][name] = []
    for _ in range(ROUNDS):                                            # the forms of a leg alternate
        for name, fns in forms.items():
            out["ms_per_bag"][name].append(round(timed(fns, k), 5))
    del tr, forms
    torch.cuda.empty_cache()
print(json.dumps(out))
