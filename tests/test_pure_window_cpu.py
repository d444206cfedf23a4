"""The ragged accumulation window of the teacher-free ABMIL model (mhimx_pure_window_layout_of / mhimx_pure_window_run,
csrc/pure_window.hip) without a GPU: the entry points are declared, exported and bound, the layout is pure host arithmetic, every refusal
is an error status raised before any device call and names the bag, and the trainer's mirrored shape check agrees with the C checks.
Pointers handed over here are made-up addresses: a refused call never touches them."""
import ctypes as C
import os
import re

import pytest

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
SIX = ("w1", "b1", "wa", "wc", "wp", "bp")
X0, LAB0, WS = FAKE + (1 << 41), FAKE + (1 << 42), FAKE + (1 << 40)


def _cfg(D=1024, E=512, A=128, Cc=2, student=SIX, grad=SIX, tick=True):
    p, g = L.StepParams(), L.StepGrads()
    for k, n in enumerate(student):
        setattr(p, n, FAKE + 0x1000000 * (k + 1))
    for k, n in enumerate(grad):
        setattr(g, n, FAKE + 0x1000000 * (k + 20))
    return L.StepCfg(D=D, E=E, A=A, C=Cc, k=0, act=2, da_act=1, student=p, grad=g, tick=FAKE + 4096 if tick else None,
                     p=FAKE + (1 << 36), g=FAKE + (2 << 36), m=FAKE + (3 << 36), v=FAKE + (4 << 36), n_train=1 << 20, n_all=1 << 20)


def _bags(ns, ldx=1024, x=X0, lab=LAB0):
    n = len(ns)
    ldx = ldx if isinstance(ldx, (list, tuple)) else [ldx] * n
    return (L.PureWindowBag * max(n, 1))(*[L.PureWindowBag(X=(x + (b << 33)) if x else None, ldx=ldx[b], N=ns[b],
                                                           label_dev=(lab + 64 * b) if lab else None, drop_seed=b + 1) for b in range(n)])


def _layout(ns, D=1024, **kw):
    lay = L.PureWindowLayout()
    r = L.lib().mhimx_pure_window_layout_of(C.byref(_cfg(D, **kw)), len(ns), _bags(ns, ldx=D), C.byref(lay))
    return r, lay


# ------------------------------------------------------------------------------------------------------------------ 1
def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in ("mhimx_pure_window_layout_of", "mhimx_pure_window_run"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhimx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(L.SYMBOLS) and all(hasattr(lib, n) for n in declared)            # header, export list and binding, name by name
    assert int(re.search(r"#define MHIMX_PURE_WINDOW_MAX (\d+)", hdr).group(1)) == L.PURE_WINDOW_MAX == L.INFER_MAX
    assert int(re.search(r"#define MHIMX_PURE_WINDOW_MAX_ROWS (\d+)", hdr).group(1)) == L.PURE_WINDOW_MAX_ROWS
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == lib.mhimx_version() == 620
    assert C.sizeof(L.PureWindowBag) == 40 and C.sizeof(L.PureWindowLayout) == 8 * (10 + L.PURE_WINDOW_MAX)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("ns,D", [([512] * 8, 1024), ([1, 31, 33, 160, 257, 700, 2999, 16385], 512), ([1], 256), ([3, 5], 1024),
                                  ([9000 + 255 * j for j in range(32)], 1536)])
def test_layout_is_host_arithmetic_aligned_and_disjoint(ns, D):
    r, lay = _layout(ns, D)
    assert r == 0, L.lib().mhimx_last_error()
    n, E, Cc = len(ns), 512, 2
    assert lay.total > 0 and lay.total % 256 == 0
    assert lay.rows == sum((N + 31) // 32 * 32 for N in ns)
    row0 = list(lay.row0)[:n]
    assert row0[0] == 0 and all(r0 % 32 == 0 for r0 in row0)
    assert all(row0[b + 1] >= row0[b] + ns[b] for b in range(n - 1)) and row0[-1] + ns[-1] <= lay.rows
    sizes = {"logits": 4 * n * Cc, "losses": 4 * n * 3, "H": lay.rows * E * 4, "dact": lay.rows * E * 2, "s": lay.rows * 4, "stats": 4 * n * 2,
             "z": 4 * n * E, "g_z": 4 * n * E}
    spans = []
    for name, nbytes in sizes.items():
        off = getattr(lay, name)
        assert off >= 0 and off % 256 == 0 and off + nbytes <= lay.total, (name, off, lay.total)
        spans.append((off, off + nbytes))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans            # no two of them overlap


def test_layout_grows_with_rows_and_with_bags_and_one_bag_beside_the_single_bag_step(capsys):
    """``total`` is strictly growing in the rows of the call's row space (layout.rows: a bag grows in steps of 32 rows there, so N -> N + 1
    inside one 32-row step leaves it as it is and N -> N + 32 must grow it) and in the number of bags.  The bytes of a one-bag window beside
    mhimx_pure_step_layout_of's for the same N are printed (DESIGN.md quotes them; no bound is set on the ratio)."""
    lib = L.lib()
    prev = None
    for N in (1, 32, 33, 64, 500, 512, 513, 4096, 4097, 16384, 100000, 262144):
        r, lay = _layout([N])
        assert r == 0
        if prev is not None:
            assert lay.rows >= prev[0] and lay.total >= prev[1]
            if lay.rows > prev[0]:
                assert lay.total > prev[1], (N, lay.total, prev)
            else:
                assert lay.total == prev[1]
        prev = (lay.rows, lay.total)
    totals = [_layout([700] * n)[1].total for n in range(1, 33)]
    assert all(b > a for a, b in zip(totals, totals[1:]))
    with capsys.disabled():
        for N in (64, 512, 10000, 59745):
            one, step = _layout([N])[1], L.StepLayout()
            assert lib.mhimx_pure_step_layout_of(C.byref(_cfg()), N, C.byref(step)) == 0
            print(f"\n[pure_window layout] N = {N} x 1024: one-bag window {one.total} bytes, mhimx_pure_step_layout_of {step.total} bytes, "
                  f"ratio {one.total / step.total:.3f}", end="")
        r, lay = _layout([512] * 8)
        print(f"\n[pure_window layout] 8 x 512 x 1024: {lay.total} bytes")


# ------------------------------------------------------------------------------------------------------------------ 3
def _run(cfg, ns, bags=None, ws=WS, ws_bytes=1 << 44, update=1, ldx=None):
    lib = L.lib()
    if bags is None:
        bags = _bags(ns, ldx=ldx if ldx is not None else (cfg.D if cfg is not None else 1024))
    r = lib.mhimx_pure_window_run(None, C.byref(cfg) if cfg is not None else None, len(ns), bags, 1, ws, ws_bytes, update)
    return r, lib.mhimx_last_error()


@pytest.mark.parametrize("what, ckw, ns, ldx, word", [
    ("n = 0", {}, [], 1024, b"1..32 bags"),
    ("n = 33", {}, [64] * 33, 1024, b"1..32 bags"),
    ("N = 0", {}, [64, 0, 64], 1024, b"bag 1: N must be"),
    ("N above the per-bag limit", {}, [64, 64, L.STEP_MAX_ROWS + 1], 1024, b"bag 2: N must be"),
    ("ldx < D", {}, [64, 64], [1024, 512], b"bag 1: row pitch"),
    ("ldx % 4 != 0", {}, [64, 64, 64], [1024, 1024, 1026], b"bag 2: row pitch"),
    ("N ldx 4 >= 2^32", {}, [64, 200000], [1024, 8192], b"bag 1: N * ldx * 4"),
    ("too many rows in the window", {"D": 256}, [L.STEP_MAX_ROWS, L.STEP_MAX_ROWS, 32], 256, b"rows in the window"),
    ("D % 256 != 0", {"D": 1000}, [64], 1000, b"shapes"),
    ("E != 512", {"E": 256}, [64], 1024, b"shapes"),
    ("A != 128", {"A": 64}, [64], 1024, b"shapes"),
    ("C = 5", {"Cc": 5}, [64], 1024, b"shapes"),
    ("C = 0", {"Cc": 0}, [64], 1024, b"shapes"),
    ("a NULL student parameter", {"student": SIX[:3] + SIX[4:]}, [64], 1024, b"null student parameter"),
    ("a NULL gradient view", {"grad": SIX[1:]}, [64], 1024, b"null gradient view"),
    ("no tick", {"tick": False}, [64], 1024, b"tick"),
])
def test_refusals_are_errors_in_both_entry_points_before_any_device_call(what, ckw, ns, ldx, word):
    lib = L.lib()
    cfg, lay = _cfg(**ckw), L.PureWindowLayout()
    bags = _bags(ns, ldx=ldx)
    assert lib.mhimx_pure_window_layout_of(C.byref(cfg), len(ns), bags, C.byref(lay)) < 0, what
    msg = lib.mhimx_last_error()
    assert msg.startswith(b"pure_window:") and word in msg, (what, msg)
    for update in (0, 1):
        r, msg = _run(cfg, ns, bags=bags, update=update)
        assert r < 0 and msg.startswith(b"pure_window:") and word in msg, (what, msg)


def test_run_refusals_of_its_own_arguments_without_a_device():
    lib = L.lib()
    ns = [700, 1, 33]
    r, lay = _layout(ns)
    assert r == 0
    cfg = _cfg()
    no_opt = _cfg()
    no_opt.m = None
    b_nox, b_nolab, b_odd = _bags(ns), _bags(ns), _bags(ns)
    b_nox[1].X = None
    b_nolab[2].label_dev = None
    b_odd[2].X = X0 + 4
    for kw, word in [
        (dict(cfg=None), b"null configuration"),
        (dict(bags=b_nox), b"bag 1: null or unaligned rows"),
        (dict(bags=b_odd), b"bag 2: null or unaligned rows"),
        (dict(bags=b_nolab), b"bag 2: null label"),
        (dict(cfg=no_opt), b"flat optimiser buffers"),
        (dict(ws=None), b"256-byte aligned"),
        (dict(ws=WS + 64), b"256-byte aligned"),
        (dict(ws_bytes=lay.total - 1), b"workspace too small"),
    ]:
        a = dict(cfg=cfg, ns=ns, ws_bytes=lay.total)
        a.update(kw)
        r, msg = _run(**a)
        assert r < 0 and msg.startswith(b"pure_window") and word in msg, (kw, r, msg)
    r, msg = _run(no_opt, ns, update=0, ws_bytes=lay.total - 1)
    assert r < 0 and b"workspace too small" in msg                  # update = 0 does not need the optimiser's buffers
    assert lib.mhimx_pure_window_layout_of(C.byref(cfg), 3, _bags(ns), None) < 0
    assert lib.mhimx_pure_window_layout_of(C.byref(cfg), 3, None, C.byref(L.PureWindowLayout())) < 0
    assert lib.mhimx_pure_window_layout_of(None, 3, _bags(ns), C.byref(L.PureWindowLayout())) < 0


# ------------------------------------------------------------------------------------------------------------------ 4
def test_the_trainers_shape_check_mirrors_the_c_refusals():
    """FusedTrainer.pure_window_shapes_ok says no exactly where check_pw or mhimx_pure_window_run's own argument checks do: such a window
    takes the bag-after-bag route and never raises."""
    from mhim_mil_amd.engine import FusedTrainer
    lib = L.lib()
    ok = FusedTrainer.pure_window_shapes_ok
    big = L.STEP_MAX_ROWS
    cases = [
        dict(ns=[512] * 8), dict(ns=[1]), dict(ns=[1, 31, 33, 160, 257, 700, 2999, 16385], D=512), dict(ns=[64] * 32), dict(ns=[3, 5], C=4),
        dict(ns=[700], C=1), dict(ns=[big, big], D=256), dict(ns=[700, 700], pitch=[1024, 1028]),
        dict(ns=[]), dict(ns=[64] * 33), dict(ns=[64, 0]), dict(ns=[big + 1], D=256), dict(ns=[big, big, 1], D=256), dict(ns=[64], E=256),
        dict(ns=[64], A=64), dict(ns=[64], C=5), dict(ns=[64], C=0), dict(ns=[64], D=1000), dict(ns=[64, 64], pitch=[1024, 1026]),
        dict(ns=[64, 64], pitch=[512, 1024]), dict(ns=[64, 200000], pitch=[1024, 8192]), dict(ns=[64, 64], ptr_off=[0, 4]),
        dict(ns=[64, 64], ptr_null=1), dict(ns=[64, 64], inner=[1, 2]), dict(ns=[64, 64], bagD=[1024, 512]),
    ]
    seen = set()
    for kw in cases:
        a = dict(D=1024, E=512, A=128, C=2, pitch=None, ptr_off=None, ptr_null=None, inner=None, bagD=None)
        a.update(kw)
        ns, n = a["ns"], len(a["ns"])
        pitch = a["pitch"] or [a["D"]] * n
        ptrs = [X0 + (b << 33) + (a["ptr_off"][b] if a["ptr_off"] else 0) for b in range(n)]
        if a["ptr_null"] is not None:
            ptrs[a["ptr_null"]] = 0
        inner = a["inner"] or [1] * n
        bagD = a["bagD"] or [a["D"]] * n
        cfg, lay = _cfg(D=a["D"], E=a["E"], A=a["A"], Cc=a["C"]), L.PureWindowLayout()
        bags = (L.PureWindowBag * max(n, 1))(*[L.PureWindowBag(X=ptrs[b] or None, ldx=pitch[b], N=ns[b], label_dev=LAB0, drop_seed=1)
                                               for b in range(n)])
        took = False
        # (the C call takes rows of contiguous floats of the model's width: a strided inner dimension or another width has no C twin)
        if all(i == 1 for i in inner) and all(d == a["D"] for d in bagD):
            r = lib.mhimx_pure_window_layout_of(C.byref(cfg), n, bags, C.byref(lay))
            if r == 0:
                r = lib.mhimx_pure_window_run(None, C.byref(cfg), n, bags, 1, WS, lay.total - 1, 1)
                took = r < 0 and b"workspace too small" in lib.mhimx_last_error()      # every check before the workspace's passed
        got = ok([(ns[b], bagD[b], pitch[b], inner[b], ptrs[b]) for b in range(n)], a["D"], E=a["E"], A=a["A"], C=a["C"], max_rows=big,
                 row_cap=L.PURE_WINDOW_MAX_ROWS, max_bags=L.PURE_WINDOW_MAX)
        assert got == took, (kw, got, took, lib.mhimx_last_error())
        seen.add(got)
    assert seen == {True, False}
