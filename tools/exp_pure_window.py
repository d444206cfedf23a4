"""Accumulation windows of the teacher-free ABMIL model: FusedTrainer(model="mhim_pure", accumulation_steps=k).window_step timed on
  A   c1: windows of 8 bags of 512 x 1024, 8 rotating windows, dropout 0.25
  B   mid-size ragged: 200 distinct sizes 9 000 .. 59 745 (tools/exp_pure_step.py's list) in windows of 8
  C8  small ragged: 200 sizes drawn with a fixed seed from 64 .. 4 000, windows of 8
  C32 the same sizes in windows of 32
One invocation times ROUNDS windows of at least WINDOW_S seconds per leg (each ends in a device synchronise) and prints one JSON line
{"route": ..., "ms_per_bag": {leg: [..]}}.  To compare two checkouts, run this file from each of them alternately (REPO=<checkout> selects
the package that is imported; the route is whatever that checkout's window_step does: before mhimx_pure_window_run existed, the
bag-after-bag Python route) and summarise the collected lines:
    python tools/exp_pure_window.py --summarize new.jsonl parent.jsonl
which prints median and min .. max per leg and route and says whether the ranges overlap.  ROW_CAP (default 524288) is the trainer's
pure_window_row_cap during the run (leg B's windows have up to 420 000 rows)."""
import json, os, random, statistics, sys, time

if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
    res = {}
    for path in sys.argv[2:]:
        for line in open(path):
            line = line.strip()
            if line.startswith("{"):
                d = json.loads(line)
                for leg, v in d["ms_per_bag"].items():
                    res.setdefault(leg, {}).setdefault(d["route"], []).extend(v)
    for leg, routes in sorted(res.items()):
        for route, v in sorted(routes.items()):
            print(f"{leg:4s} {route:8s} n={len(v)}  median {statistics.median(v):.4f} ms/bag   min {min(v):.4f} .. max {max(v):.4f}")
        if len(routes) == 2:
            (ra, a), (rb, b) = sorted(routes.items())
            apart = max(a) < min(b) or max(b) < min(a)
            print(f"{leg:4s} ranges {'do NOT overlap' if apart else 'OVERLAP'}; median {ra}/{rb} = {statistics.median(a) / statistics.median(b):.3f}")
    sys.exit(0)

sys.path.insert(0, os.environ.get("REPO") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mhim_mil_amd import synth
from mhim_mil_amd.mhim import MHIM
from mhim_mil_amd.engine import FusedTrainer

D = 1024
ROUNDS = int(os.environ.get("ROUNDS", 5))
WINDOW_S = float(os.environ.get("WINDOW_S", 0.6))
LEGS = os.environ.get("LEGS", "A,B,C8,C32").split(",")
dev = torch.device("cuda", 0)
base = synth.mhim_state(7, input_dim=D, merge_enable=False)


def trainer(accum):
    m = MHIM(input_dim=D, n_classes=2, baseline="attn", act="gelu", da_act="relu", merge_enable=False, dropout=0.25)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in base.items()})
    tr = FusedTrainer(m.to(dev).train(), None, model="mhim_pure", accumulation_steps=accum)
    if hasattr(tr, "pure_window_row_cap"):
        tr.pure_window_row_cap = int(os.environ.get("ROW_CAP", 524288))
    return tr


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
mid = [9000 + 255 * j for j in range(200)]
random.Random(3).shuffle(mid)
small = [random.Random(17 + j).randint(64, 4000) for j in range(200)]
x0 = torch.randn(max(mid), D, device=dev, generator=g).abs_()
labels = [torch.tensor([j % 2], device=dev) for j in range(32)]
windows = {
    "A": (8, [[torch.randn(512, D, device=dev, generator=g).abs_() for _ in range(8)] for _ in range(8)]),
    "B": (8, [[x0[:n] for n in mid[w:w + 8]] for w in range(0, 200, 8)]),
    "C8": (8, [[x0[:n] for n in small[w:w + 8]] for w in range(0, 200, 8)]),
    "C32": (32, [[x0[:n] for n in small[w:w + 32]] for w in range(0, 192, 32)]),
}
out = {"route": os.environ.get("ROUTE_NAME", "new"), "rounds": ROUNDS, "window_s": WINDOW_S, "ms_per_bag": {}, "exec": {}}
for leg in LEGS:
    k, wins = windows[leg]
    tr = trainer(k)
    fns = [lambda w=w, k=k: tr.window_step(w, labels[:k]) for w in wins]
    for f in fns:                                                  # warm every shape
        f()
    torch.cuda.synchronize()
    out["exec"][leg] = bool(tr.last.get("exec"))
    out["ms_per_bag"][leg] = [round(timed(fns, k), 5) for _ in range(ROUNDS)]
    del tr, fns
    torch.cuda.empty_cache()
print(json.dumps(out))
