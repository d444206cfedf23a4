"""mhimx_select_rows_many (csrc/select_many.hip) without a GPU: header / binding / export agreement, the table struct, the workspace query,
every refusal of the argument check (it runs before any device call: pointers are made-up addresses) with the bag named, the Python mirror
ops.select_bags_ok against the C check, and MHIM.student_rows_many's own argument errors."""
import ctypes as C
import os
import re

import pytest

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE, ROWS, TICK, WS = 0x7F0000000000, 0x7F1000000000, 0x7F2000000000, 0x7F3000000000        # never dereferenced
CALL = b"mhimx_select_rows_many"
SMR = L.STEP_MAX_ROWS


def _bag(N, k=None, n_sel=None, merge_R=None, row0=0, out0=0, seed=1):
    """(row0, N, k, n_sel, merge_R, out0, seed) with the default recipe's counts where none are given"""
    k = max(1, min(N, 4096 if N <= 16384 else 16384, -(-N * 6 // 100))) if k is None else k
    n_sel = k // 2 if n_sel is None else n_sel
    merge_R = (N - n_sel) // 10 if merge_R is None else merge_R
    return (row0, N, k, n_sel, merge_R, out0, seed)


def _packed(bags):
    """the same bags one behind the other in the score and the output vector"""
    out, r, o = [], 0, 0
    for b in bags:
        out.append((r, b[1], b[2], b[3], b[4], o, b[6]))
        r += b[1]
        o += max(b[1] - b[3], 0)
    return out


def _tab(bags):
    from mhim_mil_amd import ops
    return ops.select_bags(bags)


def _ws_bytes(bags):
    return L.lib().mhimx_select_rows_many_ws_bytes(len(bags), _tab(bags))


def _run(bags, score=SCORE, rows=ROWS, tab=True, ws=WS, ws_bytes=1 << 40, tick=TICK):
    lib = L.lib()
    r = lib.mhimx_select_rows_many(None, score, len(bags), _tab(bags) if tab else None, tick, rows, ws, ws_bytes, 1)
    return r, lib.mhimx_last_error()


def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    m = re.search(r"typedef struct \{ int64_t ([a-zA-Z0-9_, ]+); uint64_t seed; \} mhimx_select_bag;", hdr)
    assert m and [f.strip() for f in m.group(1).split(",")] == ["row0", "N", "k", "n_sel", "merge_R", "out0"]
    assert [n for n, _ in L.SelectBag._fields_] == ["row0", "N", "k", "n_sel", "merge_R", "out0", "seed"]
    assert C.sizeof(L.SelectBag) == 56
    assert [getattr(L.SelectBag, n).offset for n, _ in L.SelectBag._fields_] == [0, 8, 16, 24, 32, 40, 48]
    lib = L.lib()
    for name in ("mhimx_select_rows_many", "mhimx_select_rows_many_ws_bytes"):
        assert hasattr(lib, name) and name in L.SYMBOLS and re.search(rf"\b{name}\(", hdr)
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == 620         # additions only
    assert int(re.search(r"#define MHIMX_STEP_MAX_ROWS (\d+)", hdr).group(1)) == SMR
    assert "masking.py:9-88" in hdr and "merge.py:158-176" in hdr                                       # the reference lines the call replaces


def test_ws_bytes_small_tables_large_tables_and_offsets():
    small = _ws_bytes(_packed([_bag(1, k=1, n_sel=0, merge_R=0), _bag(64), _bag(4097), _bag(16384)]))
    assert 0 <= small <= 4096 and small % 256 == 0
    assert _ws_bytes(_packed([_bag(16384)] * 32)) == small                      # (the small bags take no workspace, however many)
    prev = small
    for N in (16385, 20000, 100000, SMR):                                       # monotone in the largest large bag
        b = _ws_bytes(_packed([_bag(500), _bag(N), _bag(97)]))
        assert b > prev and b % 256 == 0, (N, b, prev)
        assert b >= 256 + 8 * N + L.lib().mhimx_select_ws_bytes(N)              # the id list and the select's own scratch
        assert _ws_bytes(_packed([_bag(16385), _bag(N), _bag(N - 1)])) == b     # the maximum over the large bags, not their sum
        prev = b
    one = _ws_bytes([_bag(40000)])
    assert _ws_bytes([_bag(40000, row0=12345, out0=777)]) == one                # row0 / out0 do not matter
    assert _ws_bytes([_bag(40000, row0=1 << 40, out0=3)]) == one


REFUSED = [
    ("n_bags 0", [], [b"n_bags=0"]),
    ("n_bags 33", [_bag(10)] * 33, [b"n_bags=33"]),
    ("N 0", _packed([_bag(10), _bag(0, k=1, n_sel=0, merge_R=0)]), [b"bag 1", b"N=0"]),
    ("N max + 1", _packed([_bag(10), _bag(5), _bag(SMR + 1, k=100)]), [b"bag 2", b"N="]),
    ("k 0", _packed([_bag(10, k=0, n_sel=0, merge_R=0)]), [b"bag 0", b"k=0"]),
    ("k > N", _packed([_bag(64), _bag(10, k=11, n_sel=2, merge_R=1)]), [b"bag 1", b"k=11"]),
    ("k 4097 at 16384 rows", _packed([_bag(16384, k=4097)]), [b"bag 0", b"k=4097"]),
    ("k 16385 above 16384 rows", _packed([_bag(64), _bag(64), _bag(20000, k=16385)]), [b"bag 2", b"k=16385"]),
    ("n_sel < 0", _packed([_bag(64, k=8, n_sel=-1, merge_R=0)]), [b"bag 0", b"n_sel=-1"]),
    ("n_sel > k", _packed([_bag(64), _bag(64, k=8, n_sel=9, merge_R=0)]), [b"bag 1", b"n_sel=9"]),
    ("merge_R < 0", _packed([_bag(64, k=8, n_sel=4, merge_R=-1)]), [b"bag 0", b"merge_R=-1"]),
    ("merge_R > N - n_sel", _packed([_bag(64), _bag(64, k=8, n_sel=4, merge_R=61)]), [b"bag 1", b"merge_R=61"]),
    ("row0 < 0", [_bag(64), _bag(64, row0=-1, out0=100)], [b"bag 1", b"row0"]),
    ("out0 < 0", [_bag(64, out0=-1)], [b"bag 0", b"out0"]),
    ("overlap", [_bag(64, k=8, n_sel=4, out0=0), _bag(64, row0=64, out0=200), _bag(64, row0=128, out0=59)], [b"bag 2", b"overlap", b"bag 0"]),
]


@pytest.mark.parametrize("what,bags,words", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_tables(what, bags, words):
    r, msg = _run(bags)
    assert r < 0 and msg.startswith(CALL + b":"), (what, r, msg)
    for w in words:
        assert w in msg, (what, msg)
    assert _ws_bytes(bags) < 0                                               # the query refuses the same tables ...
    assert L.lib().mhimx_last_error().startswith(CALL + b"_ws_bytes:")       # ... under its own name


def test_refused_pointers_and_workspace():
    bags = _packed([_bag(700), _bag(40000)])
    for kw in (dict(score=None), dict(rows=None), dict(tab=False)):
        r, msg = _run(bags, **kw)
        assert r < 0 and msg.startswith(CALL + b":") and b"null" in msg, (kw, msg)
    assert L.lib().mhimx_select_rows_many_ws_bytes(2, None) < 0
    r, msg = _run(bags, ws=None)
    assert r < 0 and msg.startswith(CALL + b":") and b"workspace" in msg
    r, msg = _run(bags, ws=WS + 16)
    assert r < 0 and msg.startswith(CALL + b":") and b"256-byte aligned" in msg
    need = _ws_bytes(bags)
    r, msg = _run(bags, ws_bytes=need - 1)
    assert r < 0 and msg.startswith(CALL + b":") and b"workspace too small" in msg
    # tick may be NULL (as in mhimx_select_rows): with everything else in order the call gets as far as the workspace's size
    r, msg = _run(bags, tick=None, ws_bytes=need - 1)
    assert r < 0 and b"workspace too small" in msg


# valid tables and one broken rule each
MIRROR = [
    [_bag(1, k=1, n_sel=0, merge_R=0)], [_bag(1, k=1, n_sel=1, merge_R=0)], _packed([_bag(16384, k=4096)]), _packed([_bag(16385, k=16384)]),
    _packed([_bag(SMR)]), _packed([_bag(64)] * 32), [_bag(64, k=8, n_sel=8, merge_R=56)], [_bag(64, k=8, n_sel=0, merge_R=64)],
    [_bag(64, row0=1 << 40, out0=1 << 41)], [_bag(64, k=8, n_sel=4, out0=60), _bag(64, k=8, n_sel=4, out0=0)],      # (touching ranges, any order)
    [_bag(64, out0=5), _bag(64, k=64, n_sel=64, merge_R=0, out0=20)],                                              # (an empty range overlaps nothing)
    [], _packed([_bag(64)] * 33), [_bag(0, k=1, n_sel=0, merge_R=0)], [_bag(SMR + 1, k=9)], [_bag(64, k=0, n_sel=0)], [_bag(64, k=65)],
    [_bag(16384, k=4097)], [_bag(16385, k=16385)], [_bag(64, k=8, n_sel=9)], [_bag(64, k=8, n_sel=-1)], [_bag(64, k=8, n_sel=4, merge_R=61)],
    [_bag(64, merge_R=-1)], [_bag(64, row0=-1)], [_bag(64, out0=-1)], [_bag(64, k=8, n_sel=4, out0=59), _bag(64, k=8, n_sel=4, out0=0)],
    [_bag(64), _bag(64)],
]


@pytest.mark.parametrize("bags", MIRROR, ids=[str(i) for i in range(len(MIRROR))])
def test_python_mirror_agrees_with_the_c_check(bags):
    from mhim_mil_amd import ops
    need = _ws_bytes(bags)
    assert ops.select_bags_ok(bags) == (need >= 0), (bags[:3], need, L.lib().mhimx_last_error())
    assert ops.select_rows_many_ws_bytes(bags) == need
    r, msg = _run(bags, ws_bytes=1)                 # a 1-byte workspace: its size is the last thing the call checks
    assert r < 0 and (b"workspace too small" in msg) == ops.select_bags_ok(bags), msg


def test_the_mirror_saw_both_answers():
    from mhim_mil_amd import ops
    got = [ops.select_bags_ok(b) for b in MIRROR]
    assert got[:11] == [True] * 11 and not any(got[11:]), got


def test_student_rows_many_refuses_bad_arguments_before_any_device_call():
    import torch
    from mhim_mil_amd.mhim import MHIM
    m = MHIM(baseline="attn", n_classes=2, input_dim=256)
    step = m._step
    v = torch.zeros(100)
    for attns, kw in ((v, {}), ([], {}), ([v, torch.zeros(0)], {}), ([v, 3], {}), ([v], dict(offsets=[0, 100])), (v.view(10, 10), dict(offsets=[0, 100])),
                      (v, dict(offsets=[0])), (v, dict(offsets=[0, 50, 50])), (v, dict(offsets=[0, 50, 101])), (v, dict(offsets=[-1, 50]))):
        with pytest.raises(L.MhimxError, match=r"student_rows_many: "):
            m.student_rows_many(attns, **kw)
    assert m._step == step                                                  # no seed drawn by a refused call


def test_student_rows_many_with_a_ratio_schedule_and_no_iteration_takes_the_loop(monkeypatch):
    """student_rows indexes mrh_sche[i] whatever i is: with a schedule and i = None the loop raises, so the many-form must not quietly
    select with the base ratio - it goes to the loop (and raises what the loop raises), without a seed drawn or a many-select made."""
    import torch
    from mhim_mil_amd import ops
    from mhim_mil_amd.mhim import MHIM
    m = MHIM(baseline="attn", n_classes=2, input_dim=256, mask_ratio_h=0.03, mask_ratio_hr=0.5)
    m.mrh_sche = [0.03, 0.02]
    monkeypatch.setattr(ops, "select_rows_many", lambda *a, **kw: pytest.fail("the many-select must not run"))
    step = m._step
    with pytest.raises(TypeError):
        m.student_rows(100, None, torch.zeros(100))
    with pytest.raises(TypeError):
        m.student_rows_many([torch.zeros(100), torch.zeros(64)])
    assert m._step == step
