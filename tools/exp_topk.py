"""Top-k timing on the GPU box: what it costs to pick the k most attended patches of every slide after a validation pass, on the seeded,
device-resident bag set of tools/exp_infer.py (64 bags, D = 1024, N log-uniform in 500..30 000, 386 276 rows), for k = 64 and k = 2048.

    leg P   MHIM.infer_many(xs, return_attn=True) alone
    leg A   P + a Python loop of torch.topk over the per-bag vectors (tie order implementation-defined)
    leg B   P + a Python loop of ops.select_mask(score_b, k_b, k_b, want_topk=True) (the tie contract, one selection per call)
    leg C   MHIM.infer_topk(xs, k): P's calls + ONE mhimx_topk_many per chunk of bags

    python tools/exp_topk.py                       all legs in one process, warmed, alternated five times; writes the table as markdown
    python tools/exp_topk.py --leg C --k 64 --passes 3      a fixed number of passes of one leg (under rocprofv3 --kernel-trace --stats)
    python tools/exp_topk.py --large-only          the same legs on the bags above 16 384 rows alone (the multi-workgroup path)

A pass ends with ONE host read (the sum of the chosen indices); passes are repeated until a window exceeds half a second.  The bar:
C - P is smaller than both A - P and B - P by more than the largest spread (max - min over the repeats) of the legs involved."""
import argparse, json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mhim_mil_amd import ops, synth
from mhim_mil_amd.mhim import MHIM

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=["all", "P", "A", "B", "C"], default="all")
ap.add_argument("--k", type=int, nargs="*", default=[64, 2048])
ap.add_argument("--passes", type=int, default=0, help="> 0: exactly this many timed passes per leg instead of half-second windows")
ap.add_argument("--bags", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--large-only", action="store_true", help="only the bags above 16 384 rows")
ap.add_argument("--md", default="", help="write the table to this markdown file")
a = ap.parse_args()

D = 1024
dev = torch.device("cuda", 0)
rng = np.random.default_rng(2024)
sizes = [int(round(math.exp(u))) for u in rng.uniform(math.log(500), math.log(30000), size=a.bags)]
g = torch.Generator(device=dev); g.manual_seed(2000)
xs = [torch.randn(n, D, device=dev, generator=g).abs_() for n in sizes]
if a.large_only:
    xs = [x for x in xs if x.shape[0] > 16384]
    sizes = [int(x.shape[0]) for x in xs]
rows = sum(sizes)

sd = synth.mhim_state(7, input_dim=D, merge_k=5)
sd["merge.global_q"] = sd["merge.global_q_mm"]
model = MHIM(input_dim=D, n_classes=2, baseline="attn", act="gelu", da_act="relu", merge_enable=True, merge_k=5, dropout=0.25)
model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
model = model.to(dev).eval()


def leg_P(k):
    logits, attn = model.infer_many(xs, return_attn=True)
    return float(logits.sum())


def leg_A(k):
    logits, attn = model.infer_many(xs, return_attn=True)
    acc = logits.sum().double()
    for v in attn:
        acc = acc + torch.topk(v, min(k, v.numel())).indices.sum()
    return float(acc)


def leg_B(k):
    logits, attn = model.infer_many(xs, return_attn=True)
    acc = logits.sum().double()
    for v in attn:
        kb = min(k, v.numel())
        acc = acc + ops.select_mask(v, kb, kb, True, None, want_topk=True)[2].sum()
    return float(acc)


def leg_C(k):
    logits, idx, val = model.infer_topk(xs, k)
    return float(logits.sum().double() + idx.clamp_min(0).sum())


def window(fn, k):
    """ms per pass over a window of at least half a second (or exactly --passes passes)."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn(k); n += 1
        dt = time.perf_counter() - t0
        if (a.passes and n >= a.passes) or (not a.passes and dt > 0.5):
            return 1e3 * dt / n, n


legs = {"P": leg_P, "A": leg_A, "B": leg_B, "C": leg_C}
names = list(legs) if a.leg == "all" else [a.leg]
res = {"bags": len(xs), "rows": rows, "D": D, "min_N": min(sizes), "max_N": max(sizes), "bags_above_16384": sum(n > 16384 for n in sizes), "k": {}}
lines = ["| k | leg | ms / pass (median) | min .. max | minus P | share of P |", "|---|---|---|---|---|---|"]
for k in a.k:
    sums = {n: legs[n](k) for n in names}                   # warm-up: allocator, per-device kernel attributes, workspaces
    for n in names:
        legs[n](k)
    torch.cuda.synchronize()
    if {"A", "B", "C"} <= set(names):                       # the same instances wherever no tie is cut (continuous attention): equal index sums
        res.setdefault("index_sums", {})[k] = sums
    times = {n: [] for n in names}
    for rep in range(a.repeats):
        for n in names:
            ms, cnt = window(legs[n], k)
            times[n].append(ms)
            print(f"k {k} repeat {rep} {n}: {ms:.3f} ms/pass over {cnt} passes", flush=True)
    r = {n: {"median": float(np.median(t)), "min": min(t), "max": max(t), "spread": max(t) - min(t)} for n, t in times.items()}
    if "P" in r:
        for n in names:
            if n != "P":
                r[n]["minus_P"] = r[n]["median"] - r["P"]["median"]
                r[n]["share_of_P"] = r[n]["minus_P"] / r["P"]["median"]
    if len(names) == 4:
        spread = max(v["spread"] for v in r.values())
        r["largest_spread"] = spread
        r["bar_met"] = bool(r["A"]["minus_P"] - r["C"]["minus_P"] > spread and r["B"]["minus_P"] - r["C"]["minus_P"] > spread)
    res["k"][k] = r
    for n in names:
        v = r[n]
        extra = f"{v['minus_P']:.3f} | {100 * v['share_of_P']:.1f} %" if "minus_P" in v else "- | -"
        lines.append(f"| {k} | {n} | {v['median']:.3f} | {v['min']:.3f} .. {v['max']:.3f} | {extra} |")
res["calls_per_pass"] = model.last["infer_calls"]
print("\n".join(lines), flush=True)
print(json.dumps(res), flush=True)
if a.md:
    with open(a.md, "w") as f:
        f.write("\n".join(lines) + "\n\n```json\n" + json.dumps(res) + "\n```\n")
