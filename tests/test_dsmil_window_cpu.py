"""The ragged train call of the teacher-free DSMIL model (mhimx_dsmil_window_layout_of / mhimx_dsmil_window_run, csrc/dsmil_window.hip)
without a GPU: the entry points are declared, exported and bound, the layout is pure host arithmetic, every refusal is an error status
raised before any device call that names the call and the bag, and the trainer's mirrored shape check agrees with the C checks.
Pointers handed over here are made-up addresses: a refused call never touches them."""
import ctypes as C
import os
import re

import pytest

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
X0, LAB0, WS = FAKE + (1 << 41), FAKE + (1 << 42), FAKE + (1 << 40)
TWELVE = L._DSMIL_NAMES


def _cfg(D=1024, E=512, Cc=2, param=TWELVE, grad=TWELVE, tick=True, shift=None):
    p, g = L.DsmilParams(), L.DsmilGrads()
    for k, n in enumerate(param):
        setattr(p, n, FAKE + 0x1000000 * (k + 1) + (4 if n == shift else 0))
    for k, n in enumerate(grad):
        setattr(g, n, FAKE + 0x1000000 * (k + 20))
    return L.DsmilTrainCfg(D=D, E=E, C=Cc, act=2, drop_p=0.25, main_alpha=1.0, param=p, grad=g, tick=FAKE + 4096 if tick else None,
                           p=FAKE + (1 << 36), g=FAKE + (2 << 36), m=FAKE + (3 << 36), v=FAKE + (4 << 36), n_train=1 << 20, n_all=1 << 20)


def _bags(ns, ldx=1024, x=X0, lab=LAB0):
    n = len(ns)
    ldx = ldx if isinstance(ldx, (list, tuple)) else [ldx] * n
    return (L.PureWindowBag * max(n, 1))(*[L.PureWindowBag(X=(x + (b << 33)) if x else None, ldx=ldx[b], N=ns[b],
                                                           label_dev=(lab + 64 * b) if lab else None, drop_seed=b + 1) for b in range(n)])


def _layout(ns, D=1024, **kw):
    lay = L.DsmilWindowLayout()
    r = L.lib().mhimx_dsmil_window_layout_of(C.byref(_cfg(D, **kw)), len(ns), _bags(ns, ldx=D), C.byref(lay))
    return r, lay


def _run(cfg, ns, bags=None, ws=WS, ws_bytes=1 << 44, update=1, ldx=None, xdt=L.X_F32):
    lib = L.lib()
    if bags is None:
        bags = _bags(ns, ldx=ldx if ldx is not None else cfg.D)
    r = lib.mhimx_dsmil_window_run(None, C.byref(cfg), len(ns), bags, 1, ws, ws_bytes, update, xdt)
    return r, lib.mhimx_last_error()


# ------------------------------------------------------------------------------------------------------------------ 1
def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in ("mhimx_dsmil_window_layout_of", "mhimx_dsmil_window_run"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert int(re.search(r"#define MHIMX_DSMIL_WINDOW_MAX (\d+)", hdr).group(1)) == L.DSMIL_WINDOW_MAX == L.INFER_MAX
    assert int(re.search(r"#define MHIMX_DSMIL_WINDOW_MAX_ROWS (\d+)", hdr).group(1)) == L.DSMIL_WINDOW_MAX_ROWS
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == lib.mhimx_version() == 620
    assert C.sizeof(L.DsmilParams) == C.sizeof(L.DsmilGrads) == 96
    assert C.sizeof(L.DsmilTrainCfg) == 24 + 16 + 96 + 96 + 32 + 16 + 24 + 16 + 16
    assert C.sizeof(L.DsmilWindowLayout) == 8 * (10 + L.DSMIL_WINDOW_MAX)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("ns,D,Cc", [([70, 1, 513, 33, 257, 64], 256, 2), ([300, 31, 65], 256, 5), ([1], 256, 1), ([3, 5], 1024, 16),
                                     ([2000 + 255 * j for j in range(32)], 1536, 2)])
def test_layout_is_host_arithmetic_aligned_and_disjoint(ns, D, Cc):
    r, lay = _layout(ns, D, Cc=Cc)
    assert r == 0, L.lib().mhimx_last_error()
    n, E = len(ns), 512
    assert lay.total > 0 and lay.total % 256 == 0
    assert lay.rows == sum((N + 31) // 32 * 32 for N in ns)
    row0 = list(lay.row0)[:n]
    assert row0[0] == 0 and all(r0 % 32 == 0 for r0 in row0)
    assert all(row0[b + 1] >= row0[b] + ns[b] for b in range(n - 1)) and row0[-1] + ns[-1] <= lay.rows
    sizes = {"logits": 4 * n * Cc, "losses": 4 * n * 3, "logits_bag": 4 * n * Cc, "logits_ins": 4 * n * Cc, "B": 4 * n * Cc * E,
             "crit": 8 * n * Cc, "H": lay.rows * E * 4, "dact": lay.rows * E * 2}
    spans = []
    for name, nbytes in sizes.items():
        off = getattr(lay, name)
        assert off >= 0 and off % 256 == 0 and off + nbytes <= lay.total, (name, off, lay.total)
        spans.append((off, off + nbytes))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans            # no two of them overlap


def test_total_is_monotone_in_every_n_and_the_headers_bytes_per_row_hold():
    """``total`` never shrinks when a bag grows and grows whenever the row space does; per row of the row space it takes what the header
    comment says (9 761 + 8 C bytes) up to the part that does not depend on the rows: 256-byte granules of ~45 buffers and the split-K
    slabs, weight images and per-bag partials, bounded here by the layout of a one-row call with the most slabs."""
    prev = None
    for N in (1, 32, 33, 64, 500, 512, 513, 4096, 4097, 16384, 100000, 262144):
        r, lay = _layout([N])
        assert r == 0
        if prev is not None:
            assert lay.rows >= prev[0] and lay.total >= prev[1]
            if lay.rows > prev[0]:
                assert lay.total > prev[1], (N, lay.total, prev)
        prev = (lay.rows, lay.total)
    for b in range(3):                                          # monotone in every bag's N, whatever the others are
        last = 0
        for N in (1, 31, 32, 33, 255, 256, 257, 3000):
            ns = [100, 257, 64]
            ns[b] = N
            t = _layout(ns, 256)[1].total
            assert t >= last
            last = t
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    m = re.search(r"(\d) (\d{3}) \+ 8 C bytes per row", hdr)
    per_row = int(m.group(1) + m.group(2))
    for Cc in (1, 2, 16):
        D = 256
        rows = L.DSMIL_WINDOW_MAX_ROWS
        big = _layout([rows // 2, rows // 2], D, Cc=Cc)[1]
        assert big.rows == rows
        # the fixed part: images (2 E D + 2 E E + 4 * 128 E ...), slabs (at most 8 E D + 16 E E + 64 * 128 E + 64 * 128 * 128 floats), per-bag buffers
        fixed = 4 * (10 * 512 * D + 18 * 512 * 512 + 66 * 128 * 512 + 66 * 128 * 128) + 2 * 4 * (Cc * Cc * 512 + 40 * 512) + 64 * 256
        assert (per_row + 8 * Cc) * rows - 64 * 256 <= big.total <= (per_row + 8 * Cc) * rows + fixed, (Cc, big.total, (per_row + 8 * Cc) * rows)
    # no larger at its cap than mhimx_pure_window_run's workspace at its cap (5 716 bytes per row there)
    assert (per_row + 8 * 16) * L.DSMIL_WINDOW_MAX_ROWS <= 5716 * L.PURE_WINDOW_MAX_ROWS


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("what, ckw, ns, ldx, word", [
    ("n = 0", {}, [], 1024, b"1..32 bags"),
    ("n = 33", {}, [64] * 33, 1024, b"1..32 bags"),
    ("C = 0", {"Cc": 0}, [64], 1024, b"shapes"),
    ("C = 17", {"Cc": 17}, [64], 1024, b"shapes"),
    ("E != 512", {"E": 256}, [64], 1024, b"shapes"),
    ("D % 256 != 0", {"D": 320}, [64], 320, b"shapes"),
    ("N = 0", {}, [64, 0, 64], 1024, b"bag 1: N must be"),
    ("ldx < D", {}, [64, 64], [1024, 512], b"bag 1: row pitch"),
    ("ldx % 4 != 0", {}, [64, 64, 64], [1024, 1024, 1026], b"bag 2: row pitch"),
    ("too many rows in the window", {"D": 256}, [L.STEP_MAX_ROWS, 32], 256, b"rows in the window"),
    ("a NULL parameter", {"param": TWELVE[:3] + TWELVE[4:]}, [64], 1024, b"null parameter"),
    ("a NULL gradient view", {"grad": TWELVE[1:]}, [64], 1024, b"null gradient view"),
    ("a misaligned weight", {"shift": "wq0"}, [64], 1024, b"16-byte aligned"),
    ("no tick", {"tick": False}, [64], 1024, b"tick"),
])
def test_refusals_are_errors_in_both_entry_points_before_any_device_call(what, ckw, ns, ldx, word):
    lib = L.lib()
    cfg, lay = _cfg(**ckw), L.DsmilWindowLayout()
    bags = _bags(ns, ldx=ldx)
    assert lib.mhimx_dsmil_window_layout_of(C.byref(cfg), len(ns), bags, C.byref(lay)) < 0, what
    err = lib.mhimx_last_error()
    assert b"dsmil_window" in err and word in err, (what, err)
    r, err = _run(cfg, ns, bags=bags)
    assert r < 0 and b"dsmil_window" in err and word in err, (what, err)


def test_run_only_refusals_name_the_call_and_the_bag():
    cfg = _cfg()
    r, err = _run(cfg, [64, 64], bags=_bags([64, 64], x=X0 + 4))                 # a misaligned bag pointer
    assert r < 0 and b"dsmil_window: bag 0: null or unaligned rows" in err, err
    bags = _bags([64, 64])
    bags[1].X = None
    r, err = _run(cfg, [64, 64], bags=bags)
    assert r < 0 and b"dsmil_window: bag 1: null or unaligned rows" in err, err
    bags = _bags([64, 64])
    bags[1].label_dev = None
    r, err = _run(cfg, [64, 64], bags=bags)
    assert r < 0 and b"dsmil_window: bag 1: null label" in err, err
    r, err = _run(cfg, [64], ldx=1028, xdt=L.X_BF16)                             # a 2-byte pitch that is no multiple of 8
    assert r < 0 and b"dsmil_window: bag 0: row pitch" in err and b"8 two-byte" in err, err
    r, err = _run(cfg, [64], xdt=3)
    assert r < 0 and b"dsmil_window: x_dtype 3" in err, err
    lay = _layout([64, 700])[1]
    r, err = _run(cfg, [64, 700], ws_bytes=lay.total - 1)
    assert r < 0 and b"dsmil_window: workspace too small" in err, err
    r, err = _run(cfg, [64, 700], ws=WS + 16, ws_bytes=lay.total)
    assert r < 0 and b"dsmil_window: the workspace must be 256-byte aligned" in err, err
    nopt = _cfg()
    nopt.p = None
    r, err = _run(nopt, [64])
    assert r < 0 and b"dsmil_window: update needs the flat optimiser buffers" in err, err


# ------------------------------------------------------------------------------------------------------------------ 4
MIRROR = [
    # (bags as (N, D, pitch, inner, ptr), model D, kwargs of the mirror, C's verdict is computed from the same numbers)
    ([(70, 256, 256, 1, X0), (1, 256, 256, 1, X0 + 4096)], 256, {}),
    ([(64, 1024, 1024, 1, X0)], 1024, {"C": 16}),
    ([(64, 1024, 1024, 1, X0)], 1024, {"C": 17}),
    ([(64, 1024, 1024, 1, X0)], 1024, {"C": 0}),
    ([(64, 1024, 1024, 1, X0)], 1024, {"E": 256}),
    ([(64, 320, 320, 1, X0)], 320, {}),
    ([(0, 256, 256, 1, X0)], 256, {}),
    ([(64, 256, 258, 1, X0)], 256, {}),
    ([(64, 256, 128, 1, X0)], 256, {}),
    ([(64, 256, 256, 1, X0 + 4)], 256, {}),
    ([(64, 256, 256, 1, 0)], 256, {}),
    ([(64, 256, 260, 1, X0)], 256, {"elem": 2}),
    ([(64, 256, 264, 1, X0)], 256, {"elem": 2}),
    ([(L.STEP_MAX_ROWS, 256, 256, 1, X0), (32, 256, 256, 1, X0 + (1 << 33))], 256, {}),
    ([(L.STEP_MAX_ROWS, 256, 256, 1, X0)], 256, {}),
    ([(64, 256, 256, 1, X0 + (b << 20)) for b in range(33)], 256, {}),
    ([(200000, 1024, 8192, 1, X0)], 1024, {}),
]


@pytest.mark.parametrize("bags,D,kw", MIRROR)
def test_the_trainers_mirror_agrees_with_the_c_checks(bags, D, kw):
    from mhim_mil_amd.engine import FusedTrainer
    elem = kw.get("elem", 4)
    cfg = _cfg(D=D, E=kw.get("E", 512), Cc=kw.get("C", 2))
    tab = (L.PureWindowBag * len(bags))(*[L.PureWindowBag(X=ptr or None, ldx=pitch, N=N, label_dev=LAB0, drop_seed=1) for N, _, pitch, _, ptr in bags])
    r = L.lib().mhimx_dsmil_window_run(None, C.byref(cfg), len(bags), tab, 1, WS, 0, 0, L.X_F32 if elem == 4 else L.X_BF16)
    err = L.lib().mhimx_last_error()
    c_takes = r < 0 and b"workspace too small" in err                            # every check but the workspace's passed
    mirror = FusedTrainer.dsmil_window_shapes_ok(bags, D, **kw)
    assert mirror == c_takes, (mirror, r, err)
