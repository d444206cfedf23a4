"""Bootstrap C-index timing on the GPU box: the censored concordance index of B = 1000 resamples of an n = 1000 patient test fold.

    device   ONE ops.cindex call (mhimx_cindex: gather, pair counts, final - three launches) for all B resamples, timed with device
             events on the launch stream after a warm-up, median / min / max over the repeats
    host     the CPU restatement of the same definition (tests/surv_oracle.py: cindex_sorted, the sort-and-walk form sksurv uses, and
             cindex_pairs, the O(n^2) definition) on a few resamples, extrapolated to B - what the reference's host loop of
             ``num_bootstrap`` metric calls has to do (engines/metrics.py:58-64, :79); sksurv itself is not installed here

    python tools/exp_cindex.py [--n 1000] [--B 1000] [--repeats 20] [--host-resamples 5] [--md FILE]

The device result is checked against the restatement on the resamples the host leg evaluates (bit-equal) before anything is timed."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mhim_mil_amd import ops
from mhim_mil_amd.validate import bootstrap_indices, _BOOT_SEED
from tests import surv_oracle as SO

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000)
ap.add_argument("--B", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--host-resamples", type=int, default=5)
ap.add_argument("--md", default="", help="write the table to this markdown file")
a = ap.parse_args()

dev = torch.device("cuda", 0)
rng = np.random.default_rng(2025)
event = rng.random(a.n) < 0.6                                   # 40 % censored
time_np = rng.integers(1, 120, a.n).astype(np.float64)           # months: tied times, events and censored samples at the same time
risk_np = rng.standard_normal(a.n).astype(np.float32)
idx = bootstrap_indices(a.n, a.B, _BOOT_SEED, dev)
ev, tm, rk = torch.from_numpy(event).to(dev), torch.from_numpy(time_np).to(dev), torch.from_numpy(risk_np).to(dev)

out = ops.cindex(ev, tm, rk, sample_idx=idx)                     # warm-up: code object, allocator
idx_np = idx[:a.host_resamples].cpu().numpy()
host = {}
for name, fn in (("cindex_sorted", SO.cindex_sorted), ("cindex_pairs", SO.cindex_pairs)):
    t0 = time.perf_counter()
    rows = [SO.as_row(fn(event[i], time_np[i], risk_np[i])) for i in idx_np]
    dt = time.perf_counter() - t0
    assert np.array_equal(np.stack(rows), out[:a.host_resamples].cpu().numpy()), name
    host[name] = {"ms_per_resample": 1e3 * dt / len(idx_np), "ms_extrapolated_to_B": 1e3 * dt / len(idx_np) * a.B}

for _ in range(3):
    ops.cindex(ev, tm, rk, sample_idx=idx)
torch.cuda.synchronize()
ms = []
for _ in range(a.repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ops.cindex(ev, tm, rk, sample_idx=idx)
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
pairs = float(out[:, 1:4].sum())                                 # comparable pairs counted (the tests every i makes: B * n * n)
res = {"n": a.n, "B": a.B, "events": int(event.sum()), "pair_tests": a.B * a.n * a.n, "comparable_pairs": pairs,
       "cindex_mean": float(out[:, 0].mean()), "cindex_std": float(out[:, 0].std()),
       "device_ms": {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "repeats": a.repeats},
       "workspace_bytes": int(ops.L.lib().mhimx_cindex_ws_bytes(a.n, a.B)), "host": host, "host_resamples": a.host_resamples}
lines = ["| leg | ms for B resamples |", "|---|---|",
         f"| device: one ops.cindex call (median of {a.repeats}, min .. max) | {res['device_ms']['median']:.3f} ({min(ms):.3f} .. {max(ms):.3f}) |"]
for name, h in host.items():
    lines.append(f"| host: {name}, {h['ms_per_resample']:.1f} ms per resample x {a.B} (extrapolated from {a.host_resamples}) | "
                 f"{h['ms_extrapolated_to_B']:.0f} |")
print("\n".join(lines), flush=True)
print(json.dumps(res), flush=True)
if a.md:
    with open(a.md, "w") as f:
        f.write("\n".join(lines) + "\n\n```json\n" + json.dumps(res) + "\n```\n")
