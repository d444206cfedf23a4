"""The full MHIM(DSMIL) train call (mhimx_dsmil_mhim_window_run) beside today's per-op autograd route of the same build, same box, same
session:
  W8  FusedTrainer(model="mhim", accumulation_steps=8).window_step on a window of 8 bags of whole-slide sizes (9 000 .. 20 220 rows)
  S1  FusedTrainer(model="mhim", accumulation_steps=1).train_step on one bag of 10 000 rows
each x 1024 features, C = 2, dropout 0.25 on both models, merge_k = 5, the V2 recipe (mask_ratio_h 0.03 / hr 0.5, merge_ratio 0.9), through
the native call ("native") and with use_executor = False ("python": bag_project, forward_teacher, student_rows and the autograd graph
over dsmil.py's per-op functions).  The protocol is tools/exp_dsmil_window.py's: the two routes are timed alternately, ROUNDS times each,
every sample a window of at least WINDOW_S seconds that ends in a device synchronise; one JSON line {"ms_per_bag": {leg: {route: [..]}},
"launches": {leg: {route: n}}} is printed, then the medians and ranges and whether the call's median lies below today's route's minimum.
The launch counts come from one profiled call per leg and route (torch.profiler; null where the profiler is not available)."""
import json, os, statistics, sys, time

sys.path.insert(0, os.environ.get("REPO") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mhim_mil_amd import synth
from mhim_mil_amd.mhim import MHIM
from mhim_mil_amd.engine import FusedTrainer

D = 1024
ROUNDS = int(os.environ.get("ROUNDS", 5))
WINDOW_S = float(os.environ.get("WINDOW_S", 0.6))
LEGS = os.environ.get("LEGS", "W8,S1").split(",")
dev = torch.device("cuda", 0)
V2 = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999,
          merge_ratio=0.9, temp_t=0.1, dropout=0.25)
states = [synth.mhim_state(seed, input_dim=D, merge_k=5, baseline="dsmil") for seed in (7, 11)]      # student, a teacher of its own


def model(sd):
    m = MHIM(input_dim=D, n_classes=2, baseline="dsmil", **V2)
    sd = dict(sd)
    sd["merge.global_q"] = sd["merge.global_q_mm"]
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(dev).train()


def trainer(accum, native):
    tr = FusedTrainer(model(states[0]), model(states[1]), aux_alpha=0.5, mm=0.9997, accumulation_steps=accum)
    tr.use_executor = bool(native)
    return tr


def timed(fn, bags_per_call):
    """ms per bag of calling fn over and over for at least WINDOW_S seconds (device-complete)."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += bags_per_call
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= WINDOW_S:
            return dt / n * 1e3


def launches(fn):
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception:
        return None


g = torch.Generator(device=dev); g.manual_seed(5)
sizes = [9000, 12315, 15630, 18945, 11040, 20220, 14100, 16905]
x0 = torch.randn(max(sizes), D, device=dev, generator=g).abs_()
labels = [torch.tensor([j % 2], device=dev) for j in range(8)]
out = {"rounds": ROUNDS, "window_s": WINDOW_S, "ms_per_bag": {}, "launches": {}, "exec": {}}
for leg in LEGS:
    k = 8 if leg == "W8" else 1
    trs = {"native": trainer(k, True), "python": trainer(k, False)}
    if leg == "W8":
        bags = [x0[:n] for n in sizes]
        fns = {r: (lambda tr=tr: tr.window_step(bags, labels)) for r, tr in trs.items()}
    else:
        fns = {r: (lambda tr=tr: tr.train_step(x0[:10000], labels[1])) for r, tr in trs.items()}
    for r, f in fns.items():                                       # warm both routes
        f(); f()
        torch.cuda.synchronize()
        out["exec"].setdefault(leg, {})[r] = trs[r].last.get("exec")
    out["ms_per_bag"][leg] = {r: [] for r in fns}
    for _ in range(ROUNDS):                                        # alternately: both routes see the same box state
        for r, f in fns.items():
            out["ms_per_bag"][leg][r].append(round(timed(f, k), 5))
    out["launches"][leg] = {r: launches(f) for r, f in fns.items()}
    del trs, fns
    torch.cuda.empty_cache()
print(json.dumps(out))
for leg, routes in out["ms_per_bag"].items():
    for r, v in routes.items():
        print(f"{leg:3s} {r:7s} n={len(v)}  median {statistics.median(v):.4f} ms/bag   min {min(v):.4f} .. max {max(v):.4f}   launches {out['launches'][leg][r]}")
    a, b = routes["native"], routes["python"]
    met = statistics.median(a) < min(b)
    print(f"{leg:3s} the call's median {'lies BELOW' if met else 'does NOT lie below'} today's route's minimum; ranges "
          f"{'do not overlap' if max(a) < min(b) else 'overlap'}; median native/python = {statistics.median(a) / statistics.median(b):.3f}")
