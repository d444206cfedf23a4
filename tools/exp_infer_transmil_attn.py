"""TransMIL attention maps and instance scores, timing on the GPU box: 64 bags through an MHIM(TransMIL) model on three routes -
"many": MHIM.infer_many (mhimx_infer_transmil_run, logits only: the floor the tail is added to); "attn": MHIM.infer_cls_attn(pseudo=True)
(mhimx_infer_transmil_run_attn: the same call plus both layers' cls-row maps and the pseudo-score); "loop": the route to the same outputs
before that call had its tail - forward_test(return_attn=True) bag after bag plus _trans_score.  The two legs of tools/exp_infer_transmil.py:
"large" - 64 bags of 740 .. 21 823 rows, log-uniform, D = 1024 - and "small" - 64 bags of 512 rows.

    python tools/exp_infer_transmil_attn.py                     the three routes alternated in one process: 3 warm-up passes, then 12 timed
                                                                passes each, device events around a whole pass; median and min .. max
                                                                (DESIGN.md "Inference for TransMIL: attention maps and instance scores")
    python tools/exp_infer_transmil_attn.py --route attn --passes 2 --bags-leg small
                                                                a fixed number of passes of one route (under rocprofv3 --kernel-trace
                                                                --stats: the per-launch breakdown and the launch count of a chunk)"""
import argparse, json, math, os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mhim_mil_amd import nystrom as NY
from mhim_mil_amd import synth
from mhim_mil_amd.mhim import MHIM

ap = argparse.ArgumentParser()
ap.add_argument("--route", choices=["all", "many", "attn", "loop"], default="all")
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


def run_leg(name):
    sizes = SIZES[name]
    g = torch.Generator(device=dev); g.manual_seed(2000)
    xs = [torch.randn(n, D, device=dev, generator=g).abs_() for n in sizes]

    def many():
        return model.infer_many(xs).sum()

    def attn():
        logits, _, _ = model.infer_cls_attn(xs, pseudo=True)
        assert model.last["infer_native"]
        return logits.sum() + model.last["infer_attn"][1].sum()

    def loop():
        tot = None
        with torch.no_grad():
            for x in xs:
                lg, (maps, v) = model.forward_test(x, return_attn=True, return_act=True)
                p = model._trans_score(v[0].permute(1, 0, 2).reshape(x.shape[0], NY.INNER), maps[0][0])
                s = lg.sum() + p.sum()
                tot = s if tot is None else tot + s
        return tot

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v = float(fn())                                     # a pass ends with the host reading one number made of its outputs
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), v

    routes = {"many": many, "attn": attn, "loop": loop}
    names = ["many", "attn", "loop"] if a.route == "all" else [a.route]
    vals = {}
    for _ in range(a.warmup):
        for n in names:
            vals[n] = timed(routes[n])[1]
    times = {n: [] for n in names}
    for _ in range(a.passes):                               # alternated: the routes see the same clock and thermal state
        for n in names:
            times[n].append(timed(routes[n])[0])
    res = {"leg": name, "bags": len(xs), "rows": sum(sizes), "min_N": min(sizes), "max_N": max(sizes), "D": D, "passes": a.passes, "checksum": vals}
    for n in names:
        t = times[n]
        res[n] = {"ms_per_pass_median": float(np.median(t)), "min": min(t), "max": max(t)}
    if "attn" in names:
        res["calls_per_pass"] = len(model.infer_chunks(xs))
    if len(names) == 3:
        res["ratio_loop_over_attn"] = res["loop"]["ms_per_pass_median"] / res["attn"]["ms_per_pass_median"]
        res["ratio_attn_over_many"] = res["attn"]["ms_per_pass_median"] / res["many"]["ms_per_pass_median"]
        res["checksum_rel_diff_attn_loop"] = abs(vals["attn"] - vals["loop"]) / max(abs(vals["loop"]), 1e-30)
    print(json.dumps(res), flush=True)
    del xs
    torch.cuda.empty_cache()


for leg in (["large", "small"] if a.bags_leg == "both" else [a.bags_leg]):
    run_leg(leg)
