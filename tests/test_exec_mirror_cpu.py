"""The two tensor-free mirrors that had no test against the C refusals they mirror, without a GPU:

  * FusedTrainer.step_exec_shapes_ok (the static part of _exec_ok's 'mhim' branch) against mhimx_step_run (csrc/step.hip: check_cfg and the
    call's own argument checks);
  * ops.infer_bags_ok (the per-bag part of MHIM._infer_ok) against mhimx_infer_run_x and mhimx_infer_dsmil_run.

In the pattern of tests/test_pure_step_cpu.py::test_the_trainers_shape_check_mirrors_the_c_refusals and tests/test_ragged_checks_cpu.py:
pointers are made-up addresses, and a 1-byte workspace is the probe that everything before the workspace check passed - its size is the
last thing a call checks, and the words ``workspace too small`` appear in every call's final message.  Where a mirror and a call disagree
the call is right."""
import ctypes as C

import pytest

from mhim_mil_amd import _lib as L
from tests import test_half_input_cpu as H
from tests import test_infer_dsmil_cpu as DS

PASSED = b"workspace too small"
SMR = L.STEP_MAX_ROWS
BIG = 1 << 20


def _cnt(N, **kw):
    """the recipe's counts of a bag of N rows, with single fields replaced"""
    c = H._counts(N)
    c = {n: getattr(c, n) for n, _ in L.StepCounts._fields_}
    c.update(kw)
    return (c["k_top"], c["n_sel"], c["len_keep"], c["Lk"], c["R"])


def _hand(N, k_top, n_sel, R):
    return (k_top, n_sel, N - n_sel, N - n_sel - R, R)


STEP_CASES = [
    # ---- taken
    dict(), dict(N=64), dict(N=SMR, D=256), dict(N=40000, D=1536), dict(pitch=1028), dict(pitch=BIG + 4, N=64), dict(C=1), dict(C=4), dict(k=6),
    dict(N=16384, counts=_hand(16384, 4096, 2048, 1433)), dict(N=16385, D=256, counts=_hand(16385, 16384, 8192, 1193)),
    dict(N=100000, D=256, counts=_hand(100000, 16384, 100, 32768)), dict(N=131071, pitch=8192),
    # ---- refused, each edge by one
    dict(N=63), dict(N=SMR + 1, D=256, counts=_cnt(SMR)),
    dict(N=16384, counts=_hand(16384, 4097, 2048, 1433)), dict(N=16385, D=256, counts=_hand(16385, 16385, 8192, 1193)),
    dict(counts=_hand(512, 31, 0, 50)), dict(counts=_hand(512, 31, 32, 48)),                   # n_sel = 0, n_sel > k_top
    dict(counts=_cnt(512, Lk=_cnt(512)[3] - 1)), dict(counts=_cnt(512, len_keep=_cnt(512)[2] + 1)),      # Lk + R != len_keep, len_keep != N - n_sel
    dict(counts=_hand(512, 31, 16, 0)), dict(counts=_hand(512, 31, 16, 496)),                  # R = 0, Lk = 0
    dict(N=100000, D=256, counts=_hand(100000, 16384, 100, 32769)), dict(counts=_hand(512, 0, 0, 50)),
    dict(C=0), dict(C=5), dict(k=0), dict(k=7), dict(E=256), dict(A=64), dict(D=1000), dict(D=0, pitch=4),
    dict(pitch=1026), dict(pitch=512), dict(N=131072, pitch=8192), dict(ptr=H.X0 + 4), dict(ptr=0), dict(inner=2),
]


def test_step_exec_shapes_ok_mirrors_mhimx_step_run():
    from mhim_mil_amd.engine import FusedTrainer
    lib = L.lib()
    seeds = L.StepSeeds(1, 2, 3, 4)
    seen = []
    for kw in STEP_CASES:
        a = dict(N=512, D=1024, pitch=None, inner=1, ptr=H.X0, counts=None, k=H.K, E=512, A=128, C=2)
        a.update(kw)
        pitch = a["D"] if a["pitch"] is None else a["pitch"]
        counts = _cnt(a["N"]) if a["counts"] is None else a["counts"]
        cfg = H._rcfg(a["D"])
        cfg.E, cfg.A, cfg.C, cfg.k = a["E"], a["A"], a["C"], a["k"]
        took = False
        if a["inner"] == 1:                         # (the C call takes rows of contiguous floats: a strided inner dimension has no C twin)
            r = lib.mhimx_step_run(None, C.byref(cfg), a["ptr"], pitch, a["N"], H.LAB0, C.byref(L.StepCounts(*counts)), C.byref(seeds), 1, H.WS, 1, 1)
            msg = lib.mhimx_last_error()
            assert r < 0 and msg.startswith(b"step:"), (kw, r, msg)
            took = PASSED in msg
        got = FusedTrainer.step_exec_shapes_ok(a["N"], a["D"], pitch, a["inner"], a["ptr"], counts, a["k"], E=a["E"], A=a["A"], C=a["C"],
                                               max_rows=SMR)
        assert got == took, (kw, got, took, lib.mhimx_last_error())
        seen.append(got)
    assert seen[:13] == [True] * 13 and not any(seen[13:]), seen


def _infer_took(call, ns, ldx, xdt, ptr_off):
    lib, n = L.lib(), len(ns)
    bags = H._ibags(ns, ldx=ldx, x=H.X0 + ptr_off)
    if call == "infer":
        out = L.InferOut(logits=H.FAKE, stats=H.FAKE + 4096)
        r = lib.mhimx_infer_run_x(None, C.byref(H._icfg(256)), n, bags, None, C.byref(out), H.WS, 1, xdt)
    else:
        r = lib.mhimx_infer_dsmil_run(None, C.byref(DS._cfg(D=256)), n, bags, None, C.byref(DS._out()), H.WS, 1, xdt)
    msg = lib.mhimx_last_error()
    assert r < 0 and msg.startswith(call.encode() + b":"), (call, ns, ldx, xdt, msg)
    return PASSED in msg


@pytest.mark.parametrize("xdt", [L.X_F32, L.X_F16, L.X_BF16])
def test_infer_bags_ok_mirrors_both_inference_calls(xdt):
    from mhim_mil_amd import ops
    elem = 4 if xdt == L.X_F32 else 2
    unit = 16 // elem
    n_at = (1 << 32) // (BIG * elem)                # N * 2^20 * elem = 2^32: no bound here, the window calls' first refused size
    cases = [
        ([64, 97], 256, 0), ([1], 256, 0), ([64, 97], 264, 0), ([64, 97], 260, 0), ([64, 97], 128, 0), ([64, 97], 256, 8), ([64, 0], 256, 0),
        ([64], BIG, 0), ([64], BIG + unit, 0), ([64, n_at], BIG, 0), ([64, n_at - 1], BIG, 0),
        ([L.INFER_MAX_ROWS], 256, 0), ([L.INFER_MAX_ROWS + 1], 256, 0), ([64, SMR + 1], 256, 0),
    ]
    seen = set()
    for ns, ldx, off in cases:
        got = ops.infer_bags_ok([(N, 256, ldx, 1, H.X0 + off + (j << 33)) for j, N in enumerate(ns)], 256, elem)
        for call in ("infer", "infer_dsmil"):
            took = _infer_took(call, ns, ldx, xdt, off)
            assert got == took, (call, ns, ldx, off, xdt, got, took, L.lib().mhimx_last_error())
        seen.add(got)
    assert seen == {True, False}
    assert ops.infer_bags_ok([(64, 256, 260, 1, H.X0)], 256, elem) == (elem == 4)      # (a multiple of 4 floats, not of 8 two-byte elements)
    assert not ops.infer_bags_ok([(64, 512, 512, 1, H.X0)], 256, elem) and not ops.infer_bags_ok([(64, 256, 256, 2, H.X0)], 256, elem)
    assert not ops.infer_bags_ok([(64, 256, 256, 1, H.X0)], 256, 1)
