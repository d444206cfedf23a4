"""TransMIL validation-pass timing on the GPU box: 64 bags through an MHIM(TransMIL) model, the per-bag forward_test loop with its
cross-entropy call (the parent's only route; what validate.validate runs with chunk=0) against MHIM.infer_many (mhimx_infer_transmil_run:
one C call per chunk of bags).  Two legs of bags: "large" - 64 bags of 739 .. 21 997 rows, log-uniform (the spread of
tools/exp_surv_train.py's ragged leg), D = 1024 - and "small" - 64 bags of 512 rows.

    python tools/exp_infer_transmil.py                          both routes alternated in one process: 3 warm-up passes, then 12 timed
                                                                passes each, device events around a whole pass (DESIGN.md "Inference for
                                                                TransMIL")
    python tools/exp_infer_transmil.py --route many --passes 2 --bags-leg small
                                                                a fixed number of passes of one route (under rocprofv3 --kernel-trace
                                                                --stats: the per-launch breakdown and the launch count of a chunk)"""
import argparse, json, math, os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mhim_mil_amd import synth
from mhim_mil_amd.mhim import MHIM

ap = argparse.ArgumentParser()
ap.add_argument("--route", choices=["both", "loop", "many"], default="both")
ap.add_argument("--bags-leg", choices=["both", "large", "small"], default="both")
ap.add_argument("--passes", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--bags", type=int, default=64)
a = ap.parse_args()

D, CLASSES = 1024, 2
dev = torch.device("cuda", 0)
rng = random.Random(11)
SIZES = {"large": [int(round(math.exp(rng.uniform(math.log(739), math.log(21997))))) for _ in range(a.bags)], "small": [512] * a.bags}

sd = synth.mhim_state(7, input_dim=D, n_classes=CLASSES, baseline="selfattn", merge_enable=False)
model = MHIM(input_dim=D, n_classes=CLASSES, baseline="selfattn", act="gelu", merge_enable=False, dropout=0.25)
model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
model = model.to(dev).eval()
crit = torch.nn.CrossEntropyLoss()


def run_leg(name):
    sizes = SIZES[name]
    g = torch.Generator(device=dev); g.manual_seed(2000)
    xs = [torch.randn(n, D, device=dev, generator=g).abs_() for n in sizes]
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, CLASSES, size=len(xs))).to(dev)
    lab1 = [labels[j:j + 1] for j in range(len(xs))]

    def loop():
        """validate.validate's loop body, bag after bag."""
        tot = None
        with torch.no_grad():
            for x, y in zip(xs, lab1):
                loss = crit(model.forward_test(x.unsqueeze(0)).view(1, -1), y)
                tot = loss if tot is None else tot + loss
        return tot / len(xs)

    def many():
        _, loss = model.infer_many(xs, labels=labels)
        assert model.last["infer_native"]
        return loss.sum() / len(xs)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v = float(fn())                                     # a pass ends with the host reading the mean loss, as validate does
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), v

    routes = {"loop": loop, "many": many}
    names = ["loop", "many"] if a.route == "both" else [a.route]
    vals = {}
    for _ in range(a.warmup):
        for n in names:
            vals[n] = timed(routes[n])[1]
    times = {n: [] for n in names}
    for _ in range(a.passes):                               # alternated: both routes see the same clock and thermal state
        for n in names:
            times[n].append(timed(routes[n])[0])
    res = {"leg": name, "bags": len(xs), "rows": sum(sizes), "min_N": min(sizes), "max_N": max(sizes), "D": D, "passes": a.passes,
           "mean_loss": vals}
    for n in names:
        t = times[n]
        res[n] = {"ms_per_pass_median": float(np.median(t)), "min": min(t), "max": max(t)}
    if "many" in names:
        res["calls_per_pass"] = model.last["infer_calls"]
        res["rows_per_call_cap"] = model.infer_rows_per_call()
    if len(names) == 2:
        res["ratio_loop_over_many"] = res["loop"]["ms_per_pass_median"] / res["many"]["ms_per_pass_median"]
        res["many_median_below_loop_min"] = res["many"]["ms_per_pass_median"] < res["loop"]["min"]
        res["mean_loss_abs_diff"] = abs(vals["loop"] - vals["many"])
    print(json.dumps(res), flush=True)
    del xs
    torch.cuda.empty_cache()


for leg in (["large", "small"] if a.bags_leg == "both" else [a.bags_leg]):
    run_leg(leg)
