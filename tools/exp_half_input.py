"""Half-precision feature bags in the ragged native calls, timed on the GPU box.  For a user whose slide features are fp16 (bf16 with
--dtype bf16) three legs, alternated inside one process, five repeats each, device-event time around synchronised work:
  a   the route before mhimx_*_run_x existed: x.float() of every bag, then the fp32 call
  b   the fp32 call on bags that already are fp32 (the yardstick: what the call costs without any conversion)
  c   the half call on the bags as they are
for  infer   MHIM.infer_many over 64 bags, D = 1024, N log-uniform in 500..30 000 (tools/exp_infer.py's set)
     pure    one FusedTrainer(model="mhim_pure", accumulation_steps=8).window_step over the first 8 of those bags
     mhim    one FusedTrainer(model="mhim", accumulation_steps=8).window_step over the same 8 bags
and prints one JSON line with the median, min, max and spread (max - min) of every leg in ms, and the two statements of the merge bar:
c not slower than b by more than b's own spread; c faster than a.

    python tools/exp_half_input.py [--repeats 5] [--dtype fp16|bf16] [--parts infer,pure,mhim]
    python tools/exp_half_input.py --prof fp16|fp32 --passes 3     the infer leg alone, a fixed number of passes (under rocprofv3
                                                                   --kernel-trace --stats: the projection kernel's time per dtype)"""
import argparse, json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mhim_mil_amd import synth
from mhim_mil_amd.engine import FusedTrainer
from mhim_mil_amd.mhim import MHIM

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
ap.add_argument("--parts", default="infer,pure,mhim")
ap.add_argument("--bags", type=int, default=64)
ap.add_argument("--inner", type=int, default=0, help="calls per timed repeat (0: 20 for infer, 30 for the windows)")
ap.add_argument("--prof", choices=["fp16", "bf16", "fp32"], default=None)
ap.add_argument("--passes", type=int, default=3)
a = ap.parse_args()

D = 1024
dev = torch.device("cuda", 0)
half = {"fp16": torch.float16, "bf16": torch.bfloat16}[a.dtype if a.prof in (None, "fp32") else a.prof]
rng = np.random.default_rng(2024)
sizes = [int(round(math.exp(u))) for u in rng.uniform(math.log(500), math.log(30000), size=a.bags)]
g = torch.Generator(device=dev); g.manual_seed(2000)
xh = [torch.randn(n, D, device=dev, generator=g).abs_().to(half) for n in sizes]       # what the feature files hold
xf = [x.float() for x in xh]                                                            # the same values as fp32 bags
labels = torch.from_numpy(rng.integers(0, 2, size=a.bags)).to(dev)
lab1 = [labels[j:j + 1].contiguous() for j in range(a.bags)]
rows = sum(sizes)
V2 = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999,
          merge_ratio=0.9, temp_t=0.1)


def model(sd, **kw):
    m = MHIM(input_dim=D, n_classes=2, baseline="attn", dropout=0.25, **kw)
    sd = dict(sd)
    if "merge.global_q_mm" in sd:
        sd["merge.global_q"] = sd["merge.global_q_mm"]
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(dev)


def timed(fn, inner):
    """ms per call: `inner` calls between two device events, after a synchronise."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def run(legs, inner, check):
    for f in legs.values():                                    # warm every shape: allocator, kernel attributes, workspaces
        f(); f()
    check()
    times = {n: [] for n in legs}
    for rep in range(a.repeats):
        for n, f in legs.items():
            times[n].append(timed(f, inner))
            print(f"  repeat {rep} {n}: {times[n][-1]:.4f} ms", flush=True)
    out = {n: {"median_ms": float(np.median(t)), "min": min(t), "max": max(t), "spread": max(t) - min(t)} for n, t in times.items()}
    out["c_not_slower_than_b_by_more_than_bs_spread"] = bool(out["c"]["median_ms"] - out["b"]["median_ms"] <= out["b"]["spread"])
    out["c_faster_than_a"] = bool(out["c"]["median_ms"] < out["a"]["median_ms"])
    return out


res = {"dtype": a.dtype, "bags": a.bags, "rows": rows, "D": D, "repeats": a.repeats}
parts = a.parts.split(",")
m_inf = model(synth.mhim_state(7, input_dim=D, merge_k=5), **V2).eval()

if a.prof:
    xs = xf if a.prof == "fp32" else xh
    for _ in range(a.passes + 1):
        m_inf.infer_many(xs, labels=labels)
        assert m_inf.last["infer_native"]
    torch.cuda.synchronize()
    print(json.dumps({"prof": a.prof, "passes": a.passes + 1, "rows": rows, "calls_per_pass": m_inf.last["infer_calls"]}))
    sys.exit(0)

if "infer" in parts:
    def native(xs):
        out = m_inf.infer_many(xs, labels=labels)
        assert m_inf.last["infer_native"]
        return out

    def check():
        assert torch.equal(native(xh)[0], native(xf)[0])      # the bits of the widened call
    print("infer: 64 bags", flush=True)
    res["infer"] = run({"a": lambda: native([x.float() for x in xh]), "b": lambda: native(xf), "c": lambda: native(xh)},
                       a.inner or 20, check)
    res["infer"]["bytes_X_fp32"], res["infer"]["bytes_X_half"] = rows * D * 4, rows * D * 2

w8h, w8f, l8 = xh[:8], xf[:8], lab1[:8]
for part in ("pure", "mhim"):
    if part not in parts:
        continue
    if part == "pure":
        sd = synth.mhim_state(7, input_dim=D, merge_enable=False)
        tr = FusedTrainer(model(sd, act="gelu", da_act="relu", merge_enable=False).train(), None, model="mhim_pure", accumulation_steps=8)
    else:
        sd = synth.mhim_state(7, input_dim=D, merge_k=5)
        tr = FusedTrainer(model(sd, **V2).train(), model(synth.spread_teacher(sd), **V2).train(), aux_alpha=0.5, mm=0.9997,
                          accumulation_steps=8)

    def step(xs, want):
        tr.window_step(xs, l8)
        assert tr.last["exec"] and tr.last["x_dtype"] == want, (tr.last["exec"], tr.last.get("x_dtype"))

    print(f"{part}: one window of 8 bags, {sum(sizes[:8])} rows", flush=True)
    res[part] = run({"a": lambda: step([x.float() for x in w8h], torch.float32), "b": lambda: step(w8f, torch.float32),
                     "c": lambda: step(w8h, half)}, a.inner or 30, lambda: None)
    res[part]["rows"], res[part]["route"] = sum(sizes[:8]), str(tr.last["exec"])
    del tr
    torch.cuda.empty_cache()
print(json.dumps(res), flush=True)
