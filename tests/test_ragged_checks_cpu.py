"""The four ragged native calls (mhimx_infer_run_x, mhimx_infer_dsmil_run, mhimx_pure_window_run_x, mhimx_ragged_window_run_x) do NOT
check a bag by the same rules, and the differences are pinned here so that the one shared check (rg_check_bag, csrc/infer_tab.hpp) cannot
merge them:

  * the inference calls cap the row pitch at 2^20 elements for every element type and do not bound N * ldx * element size;
  * the window calls bound N * ldx * element size below 2^32 and cap the pitch only for the 2-byte types;
  * a bag holds up to MHIMX_INFER_MAX_ROWS rows in the inference calls, MHIMX_STEP_MAX_ROWS in the window calls (and at least 64 in
    mhimx_ragged_window_run: the single-bag step's rule);
  * pure_window counts a bag as N rounded up to 32 and checks the total after the loop, ragged_window counts N + k rounded up to 32 and
    checks the running total inside the loop, so that its message names the bag that crossed the limit.

Every expected outcome below was taken from the commit before the checks were shared (this file passed there unchanged).  No GPU: the
checks run before any device call, pointers are made-up addresses, and a 1-byte workspace is the "everything before it passed" probe - the
workspace's size is the last thing a call checks."""
import ctypes as C

import pytest

from mhim_mil_amd import _lib as L
from tests import test_half_input_cpu as H
from tests import test_infer_dsmil_cpu as DS

D = 256
CALLS = ("infer", "infer_dsmil", "pure_window", "ragged_window")
PASSED = b"workspace too small"            # what a call says when every check before the workspace's passed


def _counts(N):
    """a bag's select / Merge counts; above the single-bag limit (where the call must refuse the bag by its N) those of the limit"""
    return H._counts(min(N, L.STEP_MAX_ROWS)) if N >= 64 else L.StepCounts(1, 1, N - 1, 1, 1)


def _call(call, ns, ldx, xdt):
    lib, n = L.lib(), len(ns)
    if call in ("infer", "infer_dsmil"):
        bags = H._ibags(ns, ldx=ldx)
        if call == "infer":
            out = L.InferOut(logits=H.FAKE, stats=H.FAKE + 4096)
            r = lib.mhimx_infer_run_x(None, C.byref(H._icfg(D)), n, bags, None, C.byref(out), H.WS, 1, xdt)
        else:
            r = lib.mhimx_infer_dsmil_run(None, C.byref(DS._cfg(D=D)), n, bags, None, C.byref(DS._out()), H.WS, 1, xdt)
    elif call == "pure_window":
        bags = (L.PureWindowBag * n)(*[L.PureWindowBag(X=H.X0 + (b << 34), ldx=ldx, N=ns[b], label_dev=H.LAB0 + 64 * b, drop_seed=b + 1)
                                       for b in range(n)])
        r = lib.mhimx_pure_window_run_x(None, C.byref(H._pcfg(D)), n, bags, 1, H.WS, 1, 1, xdt)
    else:
        bags = (L.RaggedWindowBag * n)()
        for b, N in enumerate(ns):
            bags[b].X, bags[b].ldx, bags[b].N, bags[b].label_dev = H.X0 + (b << 34), ldx, N, H.LAB0 + 64 * b
            bags[b].cnt, bags[b].seeds = _counts(N), L.StepSeeds(4 * b + 1, 4 * b + 2, 4 * b + 3, 4 * b + 4)
        r = lib.mhimx_ragged_window_run_x(None, C.byref(H._rcfg(D)), n, bags, 1, H.WS, 1, 1, xdt)
    return r, lib.mhimx_last_error()


def _expect(call, ns, ldx, xdt, words):
    """words: what the refusal must say (None: the call gets as far as the workspace check)"""
    r, msg = _call(call, ns, ldx, xdt)
    assert r == -1 and msg.startswith(call.encode() + b":"), (call, ns, ldx, xdt, r, msg)
    for w in ([PASSED] if words is None else words):
        assert w in msg, (call, ns, ldx, xdt, msg)
    if words is not None:
        assert PASSED not in msg, (call, ns, ldx, xdt, msg)


BIG = 1 << 20
SMR = L.STEP_MAX_ROWS


@pytest.mark.parametrize("xdt", [L.X_F32, L.X_F16])
def test_a_pitch_just_above_2_to_the_20(xdt):
    ldx = BIG + (4 if xdt == L.X_F32 else 8)
    pitch = [b"bag 0: row pitch"]
    _expect("infer", [1], ldx, xdt, pitch)
    _expect("infer_dsmil", [1], ldx, xdt, pitch)
    _expect("pure_window", [1], ldx, xdt, None if xdt == L.X_F32 else pitch + [b"above 2^20"])
    _expect("ragged_window", [1], ldx, xdt, [b"bag 0 (N = 1)"])                 # (the single-bag step's 64-row minimum comes first)
    _expect("ragged_window", [64], ldx, xdt, None if xdt == L.X_F32 else pitch + [b"above 2^20"])
    for call in CALLS:                                                           # the pitch AT 2^20 is everybody's
        _expect(call, [64], BIG, xdt, None)


@pytest.mark.parametrize("xdt", [L.X_F32, L.X_BF16])
def test_a_bag_of_2_to_the_32_bytes_and_one_row_less(xdt):
    elt = 4 if xdt == L.X_F32 else 2
    n_at = (1 << 32) // (BIG * elt)                                              # N * 2^20 * elt = 2^32: the first size refused
    assert n_at * BIG * elt == 1 << 32 and (n_at - 1) * BIG * elt < 1 << 32
    span = [b"bag 1: N * ldx * %d must stay below 2^32" % elt]
    for call in ("infer", "infer_dsmil"):
        _expect(call, [64, n_at], BIG, xdt, None)
        _expect(call, [64, n_at - 1], BIG, xdt, None)
    for call in ("pure_window", "ragged_window"):
        _expect(call, [64, n_at], BIG, xdt, span)
        _expect(call, [64, n_at - 1], BIG, xdt, None)


@pytest.mark.parametrize("xdt", [L.X_F32, L.X_F16])
def test_one_row_above_the_window_calls_bag_limit(xdt):
    ns = [64, 64, SMR + 1]
    _expect("infer", ns, D, xdt, None)
    _expect("infer_dsmil", ns, D, xdt, None)
    _expect("pure_window", ns, D, xdt, [b"bag 2: N must be in 1..%d" % SMR])
    _expect("ragged_window", ns, D, xdt, [b"bag 2 (N = %d)" % (SMR + 1)])
    for call in ("pure_window", "ragged_window"):
        _expect(call, [64, 64, SMR], D, xdt, None)
    assert L.INFER_MAX_ROWS > SMR + 1
    for call in ("infer", "infer_dsmil"):                                        # their own limit: a bag, and a call
        _expect(call, [64, L.INFER_MAX_ROWS + 1], D, xdt, [b"bag 1: N must be in 1..%d" % L.INFER_MAX_ROWS])
        _expect(call, [64, L.INFER_MAX_ROWS - 63], D, xdt, [b"more than %d rows in one call" % L.INFER_MAX_ROWS])
        _expect(call, [64, L.INFER_MAX_ROWS - 64], D, xdt, None)


@pytest.mark.parametrize("xdt", [L.X_F32, L.X_BF16])
def test_a_row_space_one_tile_over_the_limit_in_the_last_of_three_bags(xdt):
    assert L.PURE_WINDOW_MAX_ROWS == L.RAGGED_WINDOW_MAX_ROWS == 2 * SMR
    # pure_window: a bag takes N rounded up to 32
    _expect("pure_window", [SMR, SMR - 32, 1], D, xdt, None)
    _expect("pure_window", [SMR, SMR - 31, 1], D, xdt, [b"%d rows in the window's row space" % (2 * SMR + 32)])
    # ragged_window: a bag takes N + k (k = 5) rounded up to 32; the bag that crosses the limit is named
    k = H.K
    slot = lambda N: (N + k + 31) // 32 * 32
    at, over = [SMR - 32, SMR - 128, 64], [SMR - 32, SMR - 96, 64]
    assert sum(map(slot, at)) == 2 * SMR and sum(map(slot, over)) == 2 * SMR + 32
    _expect("ragged_window", at, D, xdt, None)
    _expect("ragged_window", over, D, xdt, [b"bag 2: %d rows in the window's row space up to this bag" % (2 * SMR + 32)])
    # N + k, not N: the last bag's slot stays at 96 rows up to N = 96 - k
    _expect("ragged_window", [SMR - 32, SMR - 128, 96 - k], D, xdt, None)
    _expect("ragged_window", [SMR - 32, SMR - 128, 96 - k + 1], D, xdt, [b"bag 2: %d rows" % (2 * SMR + 32)])
    # the inference calls pad nothing
    for call in ("infer", "infer_dsmil"):
        _expect(call, over, D, xdt, None)


def test_an_unknown_element_type():
    for call in CALLS:
        _expect(call, [64], D, 3, [b"x_dtype 3"])
