"""The ragged train call of the full MHIM(DSMIL) model (mhimx_dsmil_mhim_window_layout_of / _ws_bytes / _run, csrc/dsmil_mhim.hip) without
a GPU: the entry points are declared, exported and bound, the layout is pure host arithmetic over two row spaces, every refusal is an
error status raised before any device call that names the call and the bag, and the trainer's mirrored shape check agrees with the C
checks.  Pointers handed over here are made-up addresses: a refused call never touches them."""
import ctypes as C
import os
import re

import pytest

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
X0, LAB0, WS = FAKE + (1 << 41), FAKE + (1 << 42), FAKE + (1 << 40)
TWELVE, SIX = L._DSMIL_NAMES, L._DSMIL_MERGE_NAMES
WHO = b"dsmil_mhim_window"


def _counts(N, h=0.03, hr=0.5, mr=0.9):
    c = L.StepCounts()
    assert L.lib().mhimx_step_counts_of(N, h, hr, mr, C.byref(c)) == 0
    return c


def _cfg(D=1024, E=512, Cc=2, k=5, param=TWELVE, teacher=TWELVE, grad=TWELVE, merge=SIX, merge_grad=SIX, tick=True, shift=None, q=True,
         drop_t=0.25):
    def twelve(cls, names, base):
        o = cls()
        for j, n in enumerate(names):
            setattr(o, n, FAKE + 0x1000000 * (j + base) + (4 if n == shift else 0))
        return o
    base = L.DsmilTrainCfg(D=D, E=E, C=Cc, act=2, drop_p=0.25, main_alpha=1.0, param=twelve(L.DsmilParams, param, 1),
                           grad=twelve(L.DsmilGrads, grad, 20), tick=FAKE + 4096 if tick else None, p=FAKE + (1 << 36), g=FAKE + (2 << 36),
                           m=FAKE + (3 << 36), v=FAKE + (4 << 36), n_train=1 << 20, n_all=1 << 20)
    return L.DsmilMhimCfg(base=base, teacher=twelve(L.DsmilParams, teacher, 40), merge=twelve(L.DsmilMergeParams, merge, 60),
                          merge_grad=twelve(L.DsmilMergeGrads, merge_grad, 70), q=FAKE + 0x1000000 * 80 if q else None, q_out=None, k=k,
                          cls_attn=0, drop_p_teacher=drop_t, merge_drop_p=0.1, merge_mm=0.9998, temp_t=0.1, aux_alpha=0.5, ema_mm=0.9997,
                          p_teacher=FAKE + (5 << 36))


def _bags(ns, ldx=1024, x=X0, lab=LAB0, counts=None):
    n = len(ns)
    ldx = ldx if isinstance(ldx, (list, tuple)) else [ldx] * n
    tab = (L.RaggedWindowBag * max(n, 1))()
    for b in range(n):
        tab[b].X, tab[b].ldx, tab[b].N = (x + (b << 33)) if x else None, ldx[b], ns[b]
        tab[b].label_dev = (lab + 64 * b) if lab else None
        tab[b].cnt = (counts[b] if counts is not None else _counts(max(ns[b], 64)))
        tab[b].seeds = L.StepSeeds(drop_teacher=4 * b + 1, drop_student=4 * b + 2, select=4 * b + 3, mca=4 * b + 4)
    return tab


def _layout(ns, D=1024, **kw):
    lay = L.DsmilMhimWindowLayout()
    r = L.lib().mhimx_dsmil_mhim_window_layout_of(C.byref(_cfg(D, **kw)), len(ns), _bags(ns, ldx=D), C.byref(lay))
    return r, lay


def _run(cfg, ns, bags=None, ws=WS, ws_bytes=1 << 44, update=1, ldx=None, xdt=L.X_F32):
    lib = L.lib()
    if bags is None:
        bags = _bags(ns, ldx=ldx if ldx is not None else cfg.base.D)
    r = lib.mhimx_dsmil_mhim_window_run(None, C.byref(cfg), len(ns), bags, 1, ws, ws_bytes, update, xdt)
    return r, lib.mhimx_last_error()


# ------------------------------------------------------------------------------------------------------------------ 1
def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in ("mhimx_dsmil_mhim_window_layout_of", "mhimx_dsmil_mhim_window_ws_bytes", "mhimx_dsmil_mhim_window_run"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert int(re.search(r"#define MHIMX_DSMIL_MHIM_WINDOW_MAX (\d+)", hdr).group(1)) == L.DSMIL_MHIM_WINDOW_MAX == L.INFER_MAX
    assert int(re.search(r"#define MHIMX_DSMIL_MHIM_WINDOW_MAX_ROWS (\d+)", hdr).group(1)) == L.DSMIL_MHIM_WINDOW_MAX_ROWS
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == lib.mhimx_version() == 620
    # no existing struct changed; the new ones have the header's sizes
    assert C.sizeof(L.DsmilTrainCfg) == 24 + 16 + 96 + 96 + 32 + 16 + 24 + 16 + 16
    assert C.sizeof(L.RaggedWindowBag) == 32 + 40 + 32
    assert C.sizeof(L.DsmilMergeParams) == C.sizeof(L.DsmilMergeGrads) == 48
    assert C.sizeof(L.DsmilMhimCfg) == C.sizeof(L.DsmilTrainCfg) + 96 + 48 + 48 + 16 + 8 + 8 + 24 + 8 + 16
    assert C.sizeof(L.DsmilMhimWindowLayout) == 8 * (16 + 2 * L.DSMIL_MHIM_WINDOW_MAX)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("ns,D,Cc,k", [([64, 97, 257, 2100], 256, 2, 5), ([2100, 64], 256, 5, 5), ([97], 256, 1, 1), ([257, 64, 97], 1024, 16, 6),
                                       ([1000 + 121 * j for j in range(32)], 1536, 2, 5)])
def test_layout_is_host_arithmetic_aligned_and_disjoint(ns, D, Cc, k):
    r, lay = _layout(ns, D, Cc=Cc, k=k)
    assert r == 0, L.lib().mhimx_last_error()
    n, E = len(ns), 512
    cnts = [_counts(N) for N in ns]
    assert lay.total > 0 and lay.total % 256 == 0
    # both row spaces start every bag at a multiple of 32, and a bag's rows end before the next bag's begin
    assert lay.rows == sum((N + 31) // 32 * 32 for N in ns)
    assert lay.tok_rows == sum((c.Lk + k + 31) // 32 * 32 for c in cnts)
    row0, tok0 = list(lay.row0)[:n], list(lay.tok0)[:n]
    assert row0[0] == 0 and tok0[0] == 0 and all(r0 % 32 == 0 for r0 in row0 + tok0)
    assert all(row0[b + 1] >= row0[b] + ns[b] for b in range(n - 1)) and row0[-1] + ns[-1] <= lay.rows
    assert all(tok0[b + 1] >= tok0[b] + cnts[b].Lk + k for b in range(n - 1)) and tok0[-1] + cnts[-1].Lk + k <= lay.tok_rows
    sizes = {"logits": 4 * n * Cc, "losses": 4 * n * 3, "logits_bag": 4 * n * Cc, "logits_ins": 4 * n * Cc, "B": 4 * n * Cc * E,
             "crit": 8 * n * Cc, "B_teacher": 4 * n * Cc * E, "H_teacher": lay.rows * E * 4, "H_student": lay.rows * E * 4,
             "dact": lay.rows * E * 2, "score": lay.rows * 4, "rows_all": lay.rows * 8, "tokens": lay.tok_rows * E * 4}
    spans = []
    for name, nbytes in sizes.items():
        off = getattr(lay, name)
        assert off >= 0 and off % 256 == 0 and off + nbytes <= lay.total, (name, off, lay.total)
        spans.append((off, off + nbytes))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans            # no two of them overlap
    # total equals _ws_bytes
    assert L.lib().mhimx_dsmil_mhim_window_ws_bytes(C.byref(_cfg(D, Cc=Cc, k=k)), n, _bags(ns, ldx=D)) == lay.total


def test_total_is_monotone_and_the_headers_bytes_per_row_bound_it():
    """``total`` grows with the bags; per bag row it stays below the header's worst case (7 905 + 8 C per bag row + 8 673 + 8 C per token
    row + 16 900 per row to merge, token rows + rows to merge <= N + k + 31) plus the part that does not depend on the rows, and the cap
    keeps it below mhimx_ragged_window_run's workspace at its cap (7 273 bytes per row there)."""
    prev = 0
    for N in (64, 65, 97, 257, 2100, 4097, 16384, 16385, 100000, L.DSMIL_MHIM_WINDOW_MAX_ROWS):
        r, lay = _layout([N])
        assert r == 0, (N, L.lib().mhimx_last_error())
        assert lay.total > prev
        prev = lay.total
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    m = re.search(r"Workspace bytes: (\d) (\d{3}) \+ 8 C per row of the bag space.*?(\d) (\d{3}) \+ 8 C per row of the token space.*?at most (\d+) (\d{3}) per row to merge",
                  hdr, re.S)
    bag_row, tok_row, mrg_row = int(m.group(1) + m.group(2)), int(m.group(3) + m.group(4)), int(m.group(5) + m.group(6))
    D, rows = 256, L.DSMIL_MHIM_WINDOW_MAX_ROWS
    for Cc, mr in ((2, 0.9), (16, 0.9), (2, 0.75)):
        ns = [rows // 8] * 8
        cn = [_counts(N, mr=mr) for N in ns]
        lay = L.DsmilMhimWindowLayout()
        assert L.lib().mhimx_dsmil_mhim_window_layout_of(C.byref(_cfg(D, Cc=Cc)), 8, _bags(ns, ldx=D, counts=cn), C.byref(lay)) == 0
        assert lay.rows == rows
        per_rows = (bag_row + 8 * Cc) * rows + (tok_row + 8 * Cc) * lay.tok_rows + mrg_row * sum(c.R for c in cn)
        # the fixed part: weight images, split-K slabs, per-bag heads and Merge workspace heads (< 1 MiB each), 256-byte granules
        fixed = 4 * (10 * 512 * D + 20 * 512 * 512 + 70 * 128 * 512 + 70 * 128 * 128) + 8 * (1 << 20) + 8 * 4 * (Cc * Cc * 512 + 80 * 512) + 100 * 256
        assert lay.total <= per_rows + fixed, (Cc, mr, lay.total, per_rows, fixed)
        assert lay.total >= 0.9 * per_rows, (Cc, mr, lay.total, per_rows)
    # the worst case the count rule allows (every kept row but one merged: 25 KB per bag row) at the cap, against the ragged ABMIL call's cap
    assert (bag_row + 8 * 16 + mrg_row) * rows <= 7273 * L.RAGGED_WINDOW_MAX_ROWS


# ------------------------------------------------------------------------------------------------------------------ 3
def _bad_counts(**kw):
    c = _counts(2100)
    for f, v in kw.items():
        setattr(c, f, v)
    return [_counts(64), c]


@pytest.mark.parametrize("what, ckw, ns, ldx, counts, word", [
    ("n = 0", {}, [], 1024, None, b"1..32 bags"),
    ("n = 33", {}, [64] * 33, 1024, None, b"1..32 bags"),
    ("C = 0", {"Cc": 0}, [64], 1024, None, b"shapes"),
    ("C = 17", {"Cc": 17}, [64], 1024, None, b"shapes"),
    ("E != 512", {"E": 256}, [64], 1024, None, b"shapes"),
    ("D % 256 != 0", {"D": 320}, [64], 320, None, b"shapes"),
    ("D > 2^20", {"D": (1 << 20) + 256}, [64], (1 << 20) + 256, None, b"shapes"),
    ("merge_k = 0", {"k": 0}, [64], 1024, None, b"merge_k"),
    ("merge_k = 7", {"k": 7}, [64], 1024, None, b"merge_k"),
    ("N = 0", {}, [64, 0, 64], 1024, None, b"bag 1: N must be"),
    ("N < 64", {}, [64, 63], 1024, None, b"bag 1 (N = 63): row counts"),
    ("k_top = 0", {}, [64, 2100], 1024, _bad_counts(k_top=0), b"bag 1 (N = 2100): row counts"),
    ("k_top > 4096", {}, [64, 2100], 1024, _bad_counts(k_top=4097), b"bag 1 (N = 2100): row counts"),
    ("n_sel > k_top", {}, [64, 2100], 1024, _bad_counts(n_sel=127), b"bag 1 (N = 2100): row counts"),
    ("len_keep != N - n_sel", {}, [64, 2100], 1024, _bad_counts(len_keep=2000), b"bag 1 (N = 2100): row counts"),
    ("Lk + R != len_keep", {}, [64, 2100], 1024, _bad_counts(R=100), b"bag 1 (N = 2100): row counts"),
    ("Lk = 0", {}, [64, 2100], 1024, _bad_counts(Lk=0, R=2037), b"bag 1 (N = 2100): row counts"),
    ("ldx < D", {}, [64, 64], [1024, 512], None, b"bag 1: row pitch"),
    ("ldx % 4 != 0", {}, [64, 64, 64], [1024, 1024, 1026], None, b"bag 2: row pitch"),
    ("too many rows in the window", {"D": 256}, [L.DSMIL_MHIM_WINDOW_MAX_ROWS, 64], 256, None, b"bag 1: 131136 rows in the window"),
    ("a NULL student parameter", {"param": TWELVE[:3] + TWELVE[4:]}, [64], 1024, None, b"null student parameter"),
    ("a NULL teacher parameter", {"teacher": TWELVE[:8] + TWELVE[9:]}, [64], 1024, None, b"null teacher parameter"),
    ("a NULL gradient view", {"grad": TWELVE[1:]}, [64], 1024, None, b"null gradient view"),
    ("a NULL Merge parameter", {"merge": SIX[:2] + SIX[3:]}, [64], 1024, None, b"null Merge parameter"),
    ("no global queries", {"q": False}, [64], 1024, None, b"null Merge parameter"),
    ("a NULL Merge gradient view", {"merge_grad": SIX[:5]}, [64], 1024, None, b"null Merge gradient view"),
    ("a misaligned weight", {"shift": "wq0"}, [64], 1024, None, b"16-byte aligned"),
    ("a misaligned Merge weight", {"shift": "wkv"}, [64], 1024, None, b"16-byte aligned"),
    ("a dropout probability of 1", {"drop_t": 1.0}, [64], 1024, None, b"dropout probability"),
    ("no tick", {"tick": False}, [64], 1024, None, b"tick"),
])
def test_refusals_are_errors_in_every_entry_point_before_any_device_call(what, ckw, ns, ldx, counts, word):
    lib = L.lib()
    cfg, lay = _cfg(**ckw), L.DsmilMhimWindowLayout()
    bags = _bags(ns, ldx=ldx, counts=counts)
    assert lib.mhimx_dsmil_mhim_window_layout_of(C.byref(cfg), len(ns), bags, C.byref(lay)) < 0, what
    err = lib.mhimx_last_error()
    assert WHO in err and word in err, (what, err)
    assert lib.mhimx_dsmil_mhim_window_ws_bytes(C.byref(cfg), len(ns), bags) < 0, what
    r, err = _run(cfg, ns, bags=bags)
    assert r < 0 and WHO in err and word in err, (what, err)


def test_run_only_refusals_name_the_call_and_the_bag():
    cfg = _cfg()
    r, err = _run(cfg, [64, 64], bags=_bags([64, 64], x=X0 + 4))                 # a misaligned bag pointer
    assert r < 0 and WHO + b": bag 0: null or unaligned rows" in err, err
    bags = _bags([64, 64])
    bags[1].X = None
    r, err = _run(cfg, [64, 64], bags=bags)
    assert r < 0 and WHO + b": bag 1: null or unaligned rows" in err, err
    bags = _bags([64, 64])
    bags[1].label_dev = None
    r, err = _run(cfg, [64, 64], bags=bags)
    assert r < 0 and WHO + b": bag 1: null label" in err, err
    r, err = _run(cfg, [64], ldx=1028, xdt=L.X_BF16)                             # a 2-byte pitch that is no multiple of 8
    assert r < 0 and WHO + b": bag 0: row pitch" in err and b"8 two-byte" in err, err
    r, err = _run(cfg, [64], xdt=3)
    assert r < 0 and WHO + b": x_dtype 3" in err, err
    lay = _layout([64, 700])[1]
    r, err = _run(cfg, [64, 700], ws_bytes=lay.total - 1)
    assert r < 0 and WHO + b": workspace too small" in err, err
    r, err = _run(cfg, [64, 700], ws=WS + 16, ws_bytes=lay.total)
    assert r < 0 and WHO + b": the workspace must be 256-byte aligned" in err, err
    nopt = _cfg()
    nopt.base.p = None
    r, err = _run(nopt, [64])
    assert r < 0 and WHO + b": update needs the flat optimiser buffers" in err, err


# ------------------------------------------------------------------------------------------------------------------ 4
def _cnt(N, **kw):
    c = _counts(max(N, 64))
    t = dict(k_top=c.k_top, n_sel=c.n_sel, len_keep=c.len_keep, Lk=c.Lk, R=c.R)
    t.update(kw)
    return (t["k_top"], t["n_sel"], t["len_keep"], t["Lk"], t["R"])


MIRROR = [
    # (bags as (N, D, pitch, inner, ptr, counts), model D, merge_k, kwargs of the mirror; C's verdict is computed from the same numbers)
    ([(64, 256, 256, 1, X0, _cnt(64)), (97, 256, 256, 1, X0 + (1 << 20), _cnt(97))], 256, 5, {}),
    ([(2100, 1024, 1024, 1, X0, _cnt(2100))], 1024, 6, {"C": 16}),
    ([(2100, 1024, 1024, 1, X0, _cnt(2100))], 1024, 5, {"C": 17}),
    ([(2100, 1024, 1024, 1, X0, _cnt(2100))], 1024, 5, {"C": 0}),
    ([(2100, 1024, 1024, 1, X0, _cnt(2100))], 1024, 5, {"E": 256}),
    ([(2100, 1024, 1024, 1, X0, _cnt(2100))], 1024, 7, {}),
    ([(2100, 1024, 1024, 1, X0, _cnt(2100))], 1024, 0, {}),
    ([(64, 320, 320, 1, X0, _cnt(64))], 320, 5, {}),
    ([(63, 256, 256, 1, X0, _cnt(63))], 256, 5, {}),
    ([(0, 256, 256, 1, X0, _cnt(0))], 256, 5, {}),
    ([(64, 256, 258, 1, X0, _cnt(64))], 256, 5, {}),
    ([(64, 256, 128, 1, X0, _cnt(64))], 256, 5, {}),
    ([(64, 256, 256, 1, X0 + 4, _cnt(64))], 256, 5, {}),
    ([(64, 256, 256, 1, 0, _cnt(64))], 256, 5, {}),
    ([(64, 256, 260, 1, X0, _cnt(64))], 256, 5, {"elem": 2}),
    ([(64, 256, 264, 1, X0, _cnt(64))], 256, 5, {"elem": 2}),
    ([(2100, 256, 256, 1, X0, _cnt(2100, k_top=0))], 256, 5, {}),
    ([(2100, 256, 256, 1, X0, _cnt(2100, k_top=4097))], 256, 5, {}),
    ([(20000, 256, 256, 1, X0, _cnt(20000, k_top=4097))], 256, 5, {}),
    ([(20000, 256, 256, 1, X0, _cnt(20000, k_top=16385))], 256, 5, {}),
    ([(2100, 256, 256, 1, X0, _cnt(2100, n_sel=0, len_keep=2100, Lk=1890, R=210))], 256, 5, {}),
    ([(2100, 256, 256, 1, X0, _cnt(2100, len_keep=2036))], 256, 5, {}),
    ([(2100, 256, 256, 1, X0, _cnt(2100, Lk=0, R=2037))], 256, 5, {}),
    ([(2100, 256, 256, 1, X0, _cnt(2100, Lk=2037, R=0))], 256, 5, {}),
    ([(100000, 256, 256, 1, X0, _cnt(100000, Lk=97000 - 32769, R=32769))], 256, 5, {}),
    ([(L.DSMIL_MHIM_WINDOW_MAX_ROWS, 256, 256, 1, X0, _cnt(L.DSMIL_MHIM_WINDOW_MAX_ROWS))], 256, 5, {}),
    ([(L.DSMIL_MHIM_WINDOW_MAX_ROWS, 256, 256, 1, X0, _cnt(L.DSMIL_MHIM_WINDOW_MAX_ROWS)), (64, 256, 256, 1, X0 + (1 << 33), _cnt(64))], 256, 5, {}),
    ([(64, 256, 256, 1, X0 + (b << 20), _cnt(64)) for b in range(33)], 256, 5, {}),
    ([(64, 256, 256, 1, X0 + (b << 20), _cnt(64)) for b in range(32)], 256, 5, {}),
    ([(200000, 1024, 8192, 1, X0, _cnt(200000))], 1024, 5, {}),
]


@pytest.mark.parametrize("bags,D,k,kw", MIRROR)
def test_the_trainers_mirror_agrees_with_the_c_checks(bags, D, k, kw):
    from mhim_mil_amd.engine import FusedTrainer
    elem = kw.get("elem", 4)
    cfg = _cfg(D=D, E=kw.get("E", 512), Cc=kw.get("C", 2), k=k)
    tab = (L.RaggedWindowBag * len(bags))()
    for b, (N, _, pitch, _, ptr, cnt) in enumerate(bags):
        tab[b].X, tab[b].ldx, tab[b].N, tab[b].label_dev = ptr or None, pitch, N, LAB0
        tab[b].cnt = L.StepCounts(k_top=cnt[0], n_sel=cnt[1], len_keep=cnt[2], Lk=cnt[3], R=cnt[4])
    r = L.lib().mhimx_dsmil_mhim_window_run(None, C.byref(cfg), len(bags), tab, 1, WS, 0, 0, L.X_F32 if elem == 4 else L.X_BF16)
    err = L.lib().mhimx_last_error()
    c_takes = r < 0 and b"workspace too small" in err                            # every check but the workspace's passed
    mirror = FusedTrainer.dsmil_mhim_window_shapes_ok(bags, D, k, row_cap=L.DSMIL_MHIM_WINDOW_MAX_ROWS, **kw)
    assert mirror == c_takes, (mirror, r, err)
    assert (len(bags) != 1 or bags[0][0] != 2100 or k != 6) or mirror            # (the grid has accepted windows too)
