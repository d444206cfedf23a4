"""mhimx_topk_many (csrc/topk.hip) without a GPU: the workspace query, every refusal of the argument check (it runs before any device
call: pointers are made-up addresses), the Python mirror ops.topk_segs_ok against the C check, and MHIM.infer_topk's own argument
errors."""
import ctypes as C
import os
import re

import pytest

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE, IDX, VAL, WS = 0x7F0000000000, 0x7F1000000000, 0x7F2000000000, 0x7F3000000000        # never dereferenced
CALL = b"mhimx_topk_many"


def _tab(segs):
    return (L.TopkSeg * max(len(segs), 1))(*[L.TopkSeg(row0=r, N=n) for r, n in segs])


def _ws_bytes(segs, k):
    return L.lib().mhimx_topk_many_ws_bytes(len(segs), _tab(segs), k)


def _run(segs, k, score=SCORE, idx=IDX, tab=True, ws=WS, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = 1 << 40
    r = lib.mhimx_topk_many(None, score, len(segs), _tab(segs) if tab else None, k, 1, idx, VAL, ws, ws_bytes)
    return r, lib.mhimx_last_error()


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    assert int(re.search(r"#define MHIMX_TOPK_MAX_K (\d+)", hdr).group(1)) == L.TOPK_MAX_K == 4096
    assert C.sizeof(L.TopkSeg) == 16 and L.TopkSeg.row0.offset == 0 and L.TopkSeg.N.offset == 8
    lib = L.lib()
    for name in ("mhimx_topk_many", "mhimx_topk_many_ws_bytes"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert "CLAM/create_heatmaps.py:53" in hdr and "mhim_modules/masking.py:62" in hdr        # the reference lines the call replaces


def test_ws_bytes_is_positive_and_monotone():
    prev_n = 0
    for N in (1, 64, 16384, 16385, 40000, 200000, L.INFER_MAX_ROWS):
        prev_k = 0
        for k in (1, 7, 64, 1000, 4096):
            b = _ws_bytes([(0, 500), (500, N)], k)
            assert b > 0 and b >= prev_k, (N, k, b)
            prev_k = b
        assert prev_k >= prev_n, N
        prev_n = prev_k
    one = _ws_bytes([(0, 40000)], 64)
    assert _ws_bytes([(0, 40000)] * 32, 64) >= one and _ws_bytes([(3, 40000)], 64) == one     # (row0 does not matter)


REFUSED = [
    ("n_segs 0", dict(segs=[], k=8), [b"n_segs=0"]),
    ("n_segs 33", dict(segs=[(0, 10)] * 33, k=8), [b"n_segs=33"]),
    ("k 0", dict(segs=[(0, 10)], k=0), [b"k=0"]),
    ("k 4097", dict(segs=[(0, 10)], k=4097), [b"k=4097"]),
    ("N 0", dict(segs=[(0, 10), (10, 0)], k=8), [b"segment 1", b"N must be in 1.."]),
    ("N max + 1", dict(segs=[(0, 10), (10, 5), (15, L.INFER_MAX_ROWS + 1)], k=8), [b"segment 2", b"N must be in 1.."]),
    ("row0 < 0", dict(segs=[(-1, 10)], k=8), [b"segment 0", b"row0"]),
]


@pytest.mark.parametrize("what,kw,words", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_tables(what, kw, words):
    r, msg = _run(**kw)
    assert r < 0 and msg.startswith(CALL + b":"), (what, r, msg)
    for w in words:
        assert w in msg, (what, msg)
    assert _ws_bytes(kw["segs"], kw["k"]) < 0                              # the query refuses the same shapes ...
    assert L.lib().mhimx_last_error().startswith(CALL + b"_ws_bytes:")       # ... under its own name


def test_refused_pointers_and_workspace():
    segs = [(0, 700), (700, 40000)]
    for kw in (dict(score=None), dict(idx=None), dict(tab=False)):
        r, msg = _run(segs, 8, **kw)
        assert r < 0 and msg.startswith(CALL + b":") and b"null" in msg, (kw, msg)
    assert L.lib().mhimx_topk_many_ws_bytes(2, None, 8) < 0
    r, msg = _run(segs, 8, ws=None)
    assert r < 0 and msg.startswith(CALL + b":") and b"workspace" in msg
    r, msg = _run(segs, 8, ws=WS + 16)
    assert r < 0 and msg.startswith(CALL + b":") and b"256-byte aligned" in msg
    need = _ws_bytes(segs, 8)
    r, msg = _run(segs, 8, ws_bytes=need - 1)
    assert r < 0 and msg.startswith(CALL + b":") and b"workspace too small" in msg
    # val may be NULL: with everything else in order the call gets as far as the workspace's size, the last thing it checks
    lib = L.lib()
    assert lib.mhimx_topk_many(None, SCORE, 2, _tab(segs), 8, 0, IDX, None, WS, need - 1) < 0
    assert b"workspace too small" in lib.mhimx_last_error()


# (row0, N) tables and k: valid ones and one broken rule each
MIRROR = [([(0, 1)], 1), ([(0, 16384)], 4096), ([(5, 16385), (0, 3)], 64), ([(0, L.INFER_MAX_ROWS)], 1), ([(7, 9)] * 32, 17),
          ([(1 << 40, 9)], 3), ([], 5), ([(7, 9)] * 33, 17), ([(0, 1)], 0), ([(0, 1)], -1), ([(0, 1)], 4097), ([(0, 0)], 1),
          ([(0, 5), (5, -2)], 1), ([(0, L.INFER_MAX_ROWS + 1)], 1), ([(-1, 5)], 1), ([(0, 5), (-7, 5)], 4096)]


@pytest.mark.parametrize("segs,k", MIRROR)
def test_python_mirror_agrees_with_the_c_check(segs, k):
    from mhim_mil_amd import ops
    need = _ws_bytes(segs, k)
    assert ops.topk_segs_ok(segs, k) == (need > 0), (segs[:3], k, need)
    assert ops.topk_many_ws_bytes(segs, k) == need
    r, msg = _run(segs, k, ws_bytes=1)
    assert r < 0 and (b"workspace too small" in msg) == ops.topk_segs_ok(segs, k), msg


def test_offsets_become_segments():
    from mhim_mil_amd import ops
    assert ops.topk_segs([0, 257, 258, 770]) == [(0, 257), (257, 1), (258, 512)]
    assert ops.topk_segs([(9, 4), [0, 3]]) == [(9, 4), (0, 3)]
    assert ops.topk_segs([0]) == [] and ops.topk_segs([]) == []


@pytest.mark.parametrize("k", [0, -3, 4097])
def test_infer_topk_refuses_k_before_any_device_call(k):
    import torch
    from mhim_mil_amd.mhim import MHIM
    try:
        m = MHIM(baseline="attn", n_classes=2, input_dim=256, merge_enable=False).eval()
    except Exception as e:                                                  # (a build whose model construction needs the device)
        pytest.skip(f"MHIM cannot be constructed without a device: {e}")
    with pytest.raises(L.MhimxError, match=r"infer_topk: k="):
        m.infer_topk([torch.zeros(10, 256)], k)
