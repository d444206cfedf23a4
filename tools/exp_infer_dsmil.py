"""DSMIL validation-pass timing on the GPU box: tools/exp_infer.py's 64 bags (same seeds: D = 1024, N log-uniform in 500..30 000) through
an MHIM(DSMIL) model, the per-bag forward_test loop with validate_func's mix and its cross-entropy call (the parent's only route; what
validate.validate runs with chunk=0) against MHIM.infer_many (mhimx_infer_dsmil_run: one C call per chunk of bags).

    python tools/exp_infer_dsmil.py                        both legs in one process, alternated five times (DESIGN.md "Inference")
    python tools/exp_infer_dsmil.py --leg many --passes 3  a fixed number of passes (under rocprofv3 --kernel-trace --stats: the per-launch
                                                           breakdown of the native call)

Both legs are warmed up first; a window is timed with device events around its passes and ends with a device synchronise; windows are
repeated until one exceeds half a second.  The device clock torch reports is noted before and after."""
import argparse, json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mhim_mil_amd import synth
from mhim_mil_amd.mhim import MHIM

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=["both", "loop", "many"], default="both")
ap.add_argument("--passes", type=int, default=0, help="> 0: exactly this many timed passes per leg instead of half-second windows")
ap.add_argument("--bags", type=int, default=64)
ap.add_argument("--classes", type=int, default=2)
ap.add_argument("--row-cap", type=int, default=0, help="MHIM.infer_row_cap for this run (0: the default; the DSMIL cap is derived from it)")
ap.add_argument("--repeats", type=int, default=5)
a = ap.parse_args()

D, E = 1024, 512
dev = torch.device("cuda", 0)
rng = np.random.default_rng(2024)
sizes = [int(round(math.exp(u))) for u in rng.uniform(math.log(500), math.log(30000), size=a.bags)]
g = torch.Generator(device=dev); g.manual_seed(2000)
xs = [torch.randn(n, D, device=dev, generator=g).abs_() for n in sizes]
labels = torch.from_numpy(rng.integers(0, a.classes, size=a.bags)).to(dev)
lab1 = [labels[j:j + 1] for j in range(a.bags)]
rows = sum(sizes)

sd = synth.mhim_state(7, input_dim=D, n_classes=a.classes, baseline="dsmil", merge_enable=False)
model = MHIM(input_dim=D, n_classes=a.classes, baseline="dsmil", act="gelu", merge_enable=False, dropout=0.25)
model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
model = model.to(dev).eval()
if a.row_cap:
    model.infer_row_cap = a.row_cap
crit = torch.nn.CrossEntropyLoss()


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate(dev))
    except Exception as e:                                   # (the management library is not everywhere)
        return f"not read ({type(e).__name__})"


def leg_loop():
    """validate.validate's loop body for DSMIL, bag after bag (engine.CommonMIL.validate_func's mix)."""
    loss_sum = None
    with torch.no_grad():
        for x, y in zip(xs, lab1):
            lg = model.forward_test(x.unsqueeze(0))[0]
            logits = 0.5 * lg[0] + 0.5 * lg[1]
            loss = crit(logits.view(1, -1), y.view(1))
            loss_sum = loss if loss_sum is None else loss_sum + loss
    return loss_sum / len(xs)


def leg_many():
    logits, loss = model.infer_many(xs, labels=labels)
    assert model.last["infer_native"]
    return loss.sum() / len(xs)


def window(fn):
    """(ms per pass by device events, ms per pass by the host clock, passes) over a window of at least half a second (or --passes)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    e0.record()
    while True:
        float(fn()); n += 1                                 # a pass ends with the host reading the mean loss, as validate does
        if (a.passes and n >= a.passes) or (not a.passes and time.perf_counter() - t0 > 0.5):
            break
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, 1e3 * (time.perf_counter() - t0) / n, n


legs = {"loop": leg_loop, "many": leg_many}
names = ["loop", "many"] if a.leg == "both" else [a.leg]
clock0 = clock_mhz()
vals = {n: float(legs[n]()) for n in names}               # warm-up: allocator, per-device kernel attributes, workspace
for n in names:
    float(legs[n]())
torch.cuda.synchronize()
times = {n: [] for n in names}
for rep in range(a.repeats):
    for n in names:
        ms, host_ms, k = window(legs[n])
        times[n].append(ms)
        print(f"repeat {rep} {n}: {ms:.3f} ms/pass (events), {host_ms:.3f} (host clock) over {k} passes", flush=True)
res = {"bags": a.bags, "rows": rows, "D": D, "classes": a.classes, "min_N": min(sizes), "max_N": max(sizes), "mean_loss": vals,
       "clock_MHz_before_after": [clock0, clock_mhz()]}
for n in names:
    t = times[n]
    res[n] = {"ms_per_pass_median": float(np.median(t)), "min": min(t), "max": max(t), "spread": max(t) - min(t)}
if "many" in names:
    res["calls_per_pass"] = model.last["infer_calls"]
    res["rows_per_call_cap"] = model.infer_rows_per_call()
if len(names) == 2:
    res["ratio_loop_over_many"] = res["loop"]["ms_per_pass_median"] / res["many"]["ms_per_pass_median"]
    res["faster_by_more_than_spread"] = (res["loop"]["ms_per_pass_median"] - res["many"]["ms_per_pass_median"]
                                         > max(res["loop"]["spread"], res["many"]["spread"]))
    res["mean_loss_abs_diff"] = abs(vals["loop"] - vals["many"])
print(json.dumps(res), flush=True)
