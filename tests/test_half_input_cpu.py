"""Half-precision feature bags in the ragged native calls (mhimx_infer_run_x / mhimx_pure_window_run_x / mhimx_ragged_window_run_x)
without a GPU: the three entry points are declared, exported and bound, every refusal of the 2-byte element types is an error status
raised before any device call with the call's own prefix, x_dtype = 0 refuses what the fp32 entry point refuses in the same words, and
the trainer's mirrored shape checks agree with the C checks for 2-byte rows.  Pointers handed over here are made-up addresses: a
refused call never touches them."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
X0, LAB0, WS = FAKE + (1 << 41), FAKE + (1 << 42), FAKE + (1 << 40)
SIX = ("w1", "b1", "wa", "wc", "wp", "bp")
K = 5


# ---------------------------------------------------------------------------------------------------- made-up arguments of the three calls
def _icfg(D=1024, E=512, A=128, Cc=2):
    p = L.StepParams()
    for k, n in enumerate(SIX):
        setattr(p, n, FAKE + 0x1000000 * (k + 1))
    return L.InferCfg(D=D, E=E, A=A, C=Cc, act=2, da_act=1, p=p)


def _ibags(ns, ldx=1024, x=X0):
    return (L.InferBag * max(len(ns), 1))(*[L.InferBag(X=x + (j << 33), ldx=ldx, N=n) for j, n in enumerate(ns)])


def _infer(cfg, ns, xdt, x=True, ws_bytes=1 << 44, **kw):
    lib = L.lib()
    out = L.InferOut(logits=FAKE, stats=FAKE + 4096)
    bags = _ibags(ns, **kw)
    if x:
        r = lib.mhimx_infer_run_x(None, C.byref(cfg), len(ns), bags, None, C.byref(out), WS, ws_bytes, xdt)
    else:
        r = lib.mhimx_infer_run(None, C.byref(cfg), len(ns), bags, None, C.byref(out), WS, ws_bytes)
    return r, lib.mhimx_last_error()


def _pcfg(D=1024, k=0):
    p, g = L.StepParams(), L.StepGrads()
    for j, n in enumerate(SIX):
        setattr(p, n, FAKE + 0x1000000 * (j + 1))
        setattr(g, n, FAKE + 0x1000000 * (j + 20))
    return L.StepCfg(D=D, E=512, A=128, C=2, k=k, act=2, da_act=1, student=p, grad=g, tick=FAKE + 4096, p=FAKE + (1 << 36), g=FAKE + (2 << 36),
                     m=FAKE + (3 << 36), v=FAKE + (4 << 36), n_train=1 << 20, n_all=1 << 20)


def _pure(ns, ldx, xdt, D=1024, ptr_off=0):
    lib = L.lib()
    bags = (L.PureWindowBag * len(ns))(*[L.PureWindowBag(X=X0 + (b << 34) + ptr_off, ldx=ldx, N=ns[b], label_dev=LAB0 + 64 * b, drop_seed=b + 1)
                                         for b in range(len(ns))])
    r = lib.mhimx_pure_window_run_x(None, C.byref(_pcfg(D)), len(ns), bags, 1, WS, 1, 1, xdt)      # (a 1-byte workspace: the last check)
    return r, lib.mhimx_last_error()


def _rcfg(D=1024):
    p, t, g = L.StepParams(), L.StepParams(), L.StepGrads()
    for j, (n, _) in enumerate(L.StepParams._fields_):
        setattr(p, n, FAKE + 0x1000000 * (j + 1))
    for j, n in enumerate(SIX):
        setattr(t, n, FAKE + 0x1000000 * (j + 40))
    for j, (n, _) in enumerate(L.StepGrads._fields_):
        setattr(g, n, FAKE + 0x1000000 * (j + 20))
    return L.StepCfg(D=D, E=512, A=128, C=2, k=K, act=2, da_act=1, attn2score=1, student=p, teacher=t, grad=g, tick=FAKE + 4096,
                     p=FAKE + (1 << 36), g=FAKE + (2 << 36), m=FAKE + (3 << 36), v=FAKE + (4 << 36), n_train=1 << 22, n_all=1 << 22,
                     merge_mm=0.9999, temp_t=0.1, main_alpha=1.0, aux_alpha=0.5)


def _counts(N):
    c = L.StepCounts()
    assert L.lib().mhimx_step_counts_of(N, 0.03, 0.5, 0.9, C.byref(c)) == 0, N
    return c


def _ragged(ns, ldx, xdt, D=1024, ptr_off=0):
    lib = L.lib()
    bags = (L.RaggedWindowBag * len(ns))()
    for b, N in enumerate(ns):
        bags[b].X, bags[b].ldx, bags[b].N, bags[b].label_dev = X0 + (b << 34) + ptr_off, ldx, N, LAB0 + 64 * b
        bags[b].cnt = _counts(N)
        bags[b].seeds = L.StepSeeds(4 * b + 1, 4 * b + 2, 4 * b + 3, 4 * b + 4)
    r = lib.mhimx_ragged_window_run_x(None, C.byref(_rcfg(D)), len(ns), bags, 1, WS, 1, 1, xdt)
    return r, lib.mhimx_last_error()


# ------------------------------------------------------------------------------------------------------------------ 1
def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in ("mhimx_infer_run_x", "mhimx_pure_window_run_x", "mhimx_ragged_window_run_x"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert L.SYMBOLS[name][1] == L.SYMBOLS[name[:-2]][1] + [C.c_int32]      # the fp32 call's arguments + x_dtype
    for name, val in (("F32", L.X_F32), ("F16", L.X_F16), ("BF16", L.X_BF16)):
        assert int(re.search(r"#define MHIMX_X_%s (\d+)" % name, hdr).group(1)) == val
    assert (L.X_F32, L.X_F16, L.X_BF16) == (0, 1, 2)
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == lib.mhimx_version() == 620
    # the header says what the calls replace and what they promise
    assert "datasets/dataset_feat.py:86-93" in hdr and "engines/base_engine.py:77,271" in hdr
    assert re.search(r"[Ss]ame bits as the fp32 call on the widened rows", hdr)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("xdt", [-1, 3])
def test_an_unknown_x_dtype_is_refused_by_all_three(xdt):
    r, msg = _infer(_icfg(), [100, 7], xdt)
    assert r < 0 and msg.startswith(b"infer:") and b"x_dtype" in msg, msg
    r, msg = _pure([64, 97], 1024, xdt)
    assert r < 0 and msg.startswith(b"pure_window:") and b"x_dtype" in msg, msg
    r, msg = _ragged([64, 97], 1024, xdt)
    assert r < 0 and msg.startswith(b"ragged_window:") and b"x_dtype" in msg, msg


@pytest.mark.parametrize("xdt", [L.X_F16, L.X_BF16])
def test_half_pitch_refusals_name_the_bag(xdt):
    # ldx % 8 != 0 (1028 is a valid fp32 pitch: % 4 == 0), ldx < D, ldx above 2^20
    for ldx, word in ((1028, b"row pitch"), (512, b"row pitch"), ((1 << 20) + 8, b"row pitch")):
        r, msg = _infer(_icfg(), [100, 7], xdt, ldx=ldx)
        assert r < 0 and msg.startswith(b"infer: bag 0:") and word in msg, (ldx, msg)
        r, msg = _pure([64, 97], ldx, xdt)
        assert r < 0 and msg.startswith(b"pure_window: bag 0:") and word in msg, (ldx, msg)
        r, msg = _ragged([64, 97], ldx, xdt)
        assert r < 0 and msg.startswith(b"ragged_window: bag 0:") and word in msg, (ldx, msg)
    # the same pitch is fine as fp32 rows: the call gets as far as its workspace check
    assert b"workspace too small" in _infer(_icfg(), [100, 7], L.X_F32, ldx=1028, ws_bytes=1)[1]
    assert b"workspace too small" in _pure([64, 97], 1028, L.X_F32)[1]
    # a 16-byte aligned address is asked of half rows too
    r, msg = _pure([64, 97], 1024, xdt, ptr_off=8)
    assert r < 0 and b"bag 0: null or unaligned rows" in msg
    r, msg = _ragged([64, 97], 1024, xdt, ptr_off=8)
    assert r < 0 and b"bag 0: null or unaligned rows" in msg


@pytest.mark.parametrize("xdt", [L.X_F16, L.X_BF16])
def test_the_byte_bound_of_the_window_calls_counts_two_byte_elements(xdt):
    """N * ldx * (bytes of an element) < 2^32: 131 072 rows of pitch 16 384 are exactly 2^32 bytes of half rows - refused; one row less
    passes (the call then stops at its 1-byte workspace); 200 000 x 8 192, which the fp32 form refuses, passes as half rows."""
    for run, prefix in ((_pure, b"pure_window:"), (_ragged, b"ragged_window:")):
        r, msg = run([64, 131072], 16384, xdt)
        assert r < 0 and msg.startswith(prefix) and b"bag 1: N * ldx * 2" in msg, msg
        r, msg = run([64, 131071], 16384, xdt)
        assert r < 0 and b"workspace too small" in msg, msg
        r, msg = run([64, 200000], 8192, xdt)
        assert r < 0 and b"workspace too small" in msg, msg
        r, msg = run([64, 200000], 8192, L.X_F32)
        assert r < 0 and msg.startswith(prefix) and b"bag 1: N * ldx * 4" in msg, msg


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("what, cfg_kw, ns, bag_kw, ws_bytes", [
    ("N = 0", {}, [10, 0, 10], {}, 1 << 44),
    ("E != 512", {"E": 256}, [10], {}, 1 << 44),
    ("D % 256", {"D": 1000}, [10], {"ldx": 1000}, 1 << 44),
    ("pitch not a multiple of 4 floats", {}, [10], {"ldx": 1026}, 1 << 44),
    ("workspace too small", {}, [100, 7], {}, 4096),
])
def test_x_dtype_0_refuses_in_the_words_of_the_fp32_entry_point(what, cfg_kw, ns, bag_kw, ws_bytes):
    cfg = _icfg(**cfg_kw)
    r0, m0 = _infer(cfg, ns, 0, x=False, ws_bytes=ws_bytes, **bag_kw)
    r1, m1 = _infer(cfg, ns, L.X_F32, ws_bytes=ws_bytes, **bag_kw)
    assert r0 < 0 and r1 == r0 and m1 == m0 and m0.startswith(b"infer:"), (what, m0, m1)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_the_trainers_shape_checks_mirror_the_c_checks_for_two_byte_rows():
    """FusedTrainer.pure_window_shapes_ok / ragged_window_shapes_ok with elem = 2 say no exactly where the C checks of a 2-byte x_dtype do
    (host arithmetic only); elem defaults to 4: the fp32 rule."""
    from mhim_mil_amd.engine import FusedTrainer
    big = L.STEP_MAX_ROWS
    seen = set()
    for ns, ldx, off in (([64, 97], 1024, 0), ([64, 97], 1032, 0), ([64, 97], 1028, 0), ([64, 97], 512, 0), ([64, 97], (1 << 20) + 8, 0),
                         ([64, 131072], 16384, 0), ([64, 131071], 16384, 0), ([64, 200000], 8192, 0), ([64, 97], 1024, 8)):
        ptrs = [X0 + (b << 34) + off for b in range(len(ns))]
        for elem, xdt in ((2, L.X_F16), (2, L.X_BF16), (4, L.X_F32)):
            took = b"workspace too small" in _pure(ns, ldx, xdt, ptr_off=off)[1]                # every check before the workspace's passed
            kw = {} if elem == 4 else {"elem": elem}
            got = FusedTrainer.pure_window_shapes_ok([(N, 1024, ldx, 1, p) for N, p in zip(ns, ptrs)], 1024, max_rows=big,
                                                     row_cap=L.PURE_WINDOW_MAX_ROWS, max_bags=L.PURE_WINDOW_MAX, **kw)
            assert got == took, ("pure", ns, ldx, off, elem, got, took)
            took = b"workspace too small" in _ragged(ns, ldx, xdt, ptr_off=off)[1]
            cnts = [_counts(N) for N in ns]
            got = FusedTrainer.ragged_window_shapes_ok(
                [(N, 1024, ldx, 1, p, (c.k_top, c.n_sel, c.len_keep, c.Lk, c.R)) for N, p, c in zip(ns, ptrs, cnts)], 1024, K, max_rows=big,
                row_cap=L.RAGGED_WINDOW_MAX_ROWS, max_bags=L.RAGGED_WINDOW_MAX, **kw)
            assert got == took, ("ragged", ns, ldx, off, elem, got, took)
            seen.add((elem, got))
    assert seen == {(2, True), (2, False), (4, True), (4, False)}
    assert not FusedTrainer.pure_window_shapes_ok([(64, 1024, 1024, 1, X0)], 1024, elem=1)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_a_mixed_list_raises_before_any_library_call(monkeypatch):
    """ops.infer_many / pure_window_bags look at the dtypes first (shape-only stand-ins: nothing else of them is read), and no entry point
    of the library is reached."""
    from mhim_mil_amd import ops
    monkeypatch.setattr(L, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    mk = lambda dt: types.SimpleNamespace(dtype=dt, shape=(64, 1024))
    for kinds in ((torch.float16, torch.float32), (torch.float16, torch.bfloat16), (torch.bfloat16, torch.bfloat16, torch.float32)):
        with pytest.raises(L.MhimxError, match="mixed dtypes"):
            ops.infer_many(_icfg(), [mk(k) for k in kinds])
        with pytest.raises(L.MhimxError, match="mixed dtypes"):
            ops.pure_window_bags([mk(k) for k in kinds], [None] * len(kinds), [0] * len(kinds))
    with pytest.raises(L.MhimxError, match="fp32, fp16 or bf16"):
        ops.infer_many(_icfg(), [mk(torch.float64)])
    assert ops.x_dtype_of([mk(torch.float16)] * 3) == L.X_F16 and ops.x_dtype_of([mk(torch.bfloat16)]) == L.X_BF16
    assert ops.x_dtype_of([mk(torch.float32)]) == L.X_F32


def test_the_feeder_keeps_half_sources_only_when_asked():
    """feeder._load: fp32 by default (today's behaviour); dtype=None keeps fp16 / bf16 / fp32 sources and widens anything else."""
    from mhim_mil_amd import feeder
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        assert feeder._load(src.to(dt)).dtype == torch.float32
        kept = feeder._load(src.to(dt), None)
        assert kept.dtype == dt and torch.equal(kept, src.to(dt)) and kept.is_contiguous()
    assert feeder._load(src.double(), None).dtype == torch.float32 and feeder._load(src.to(torch.int32), None).dtype == torch.float32
    assert feeder._load(src.half()[None], torch.bfloat16).dtype == torch.bfloat16
