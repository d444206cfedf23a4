"""The one-call teacher-free ABMIL step (mhimx_pure_step_layout_of / _run / _run_many, csrc/step.hip) without a GPU: the entry points are
declared, exported and bound, the layout is pure host arithmetic, and every refusal is an error status raised before any device call.
Pointers handed over here are made-up addresses: a refused call never touches them."""
import ctypes as C
import os
import re

import pytest

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
SIX = ("w1", "b1", "wa", "wc", "wp", "bp")
MERGE = ("ln_w", "ln_b", "wkv", "wq", "wo", "bo")


def _cfg(D=1024, E=512, A=128, Cc=2, student=SIX, grad=SIX, tick=True):
    """A pure step's configuration: the student's six parameters and gradient views, the tick - teacher and merge.* fields stay NULL."""
    p, g = L.StepParams(), L.StepGrads()
    for k, n in enumerate(student):
        setattr(p, n, FAKE + 0x1000000 * (k + 1))
    for k, n in enumerate(grad):
        setattr(g, n, FAKE + 0x1000000 * (k + 20))
    return L.StepCfg(D=D, E=E, A=A, C=Cc, k=0, act=2, da_act=1, student=p, grad=g, tick=FAKE + 4096 if tick else None,
                     p=FAKE + (1 << 36), g=FAKE + (2 << 36), m=FAKE + (3 << 36), v=FAKE + (4 << 36), n_train=1 << 20, n_all=1 << 20)


def _mhim_cfg(D):
    """The same trainer's mhim configuration (teacher, merge.* fields, k = 5): what mhimx_step_layout_of is asked with."""
    c = _cfg(D)
    c.k, c.attn2score = 5, 1
    for n in ("q",) + MERGE:
        setattr(c.student, n, FAKE + 0x40000000)
    for n in MERGE:
        setattr(c.grad, n, FAKE + 0x50000000)
    for n in SIX:
        setattr(c.teacher, n, FAKE + 0x60000000)
    return c


def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in ("mhimx_pure_step_layout_of", "mhimx_pure_step_run", "mhimx_pure_step_run_many"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert int(re.search(r"#define MHIMX_STEP_MAX_ROWS (\d+)", hdr).group(1)) == L.STEP_MAX_ROWS
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == lib.mhimx_version()


@pytest.mark.parametrize("N,D", [(512, 1024), (10000, 1024), (200000, 1536)])
def test_layout_is_aligned_inside_total_and_smaller_than_the_mhim_step(N, D):
    lib = L.lib()
    lay = L.StepLayout()
    assert lib.mhimx_pure_step_layout_of(C.byref(_cfg(D)), N, C.byref(lay)) == 0, lib.mhimx_last_error()
    assert lay.total > 0
    E = 512
    sizes = {"logits": 4 * 2, "losses": 4 * 3, "H_student": N * E * 4, "dact": N * E * 2, "z_student": E * 4, "g_z": E * 4, "dH": N * E * 4}
    spans = []
    for name, nbytes in sizes.items():
        off = getattr(lay, name)
        assert off >= 0 and off % 256 == 0 and off + nbytes <= lay.total, (name, off, lay.total)
        spans.append((off, off + nbytes))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans            # no two of them overlap
    for name in ("score", "rows_all", "H_teacher", "z_teacher"):               # no teacher, no row list
        assert getattr(lay, name) == -1, name
    cnt, full = L.StepCounts(), L.StepLayout()
    assert lib.mhimx_step_counts_of(N, .03, .5, .9, C.byref(cnt)) == 0
    assert lib.mhimx_step_layout_of(C.byref(_mhim_cfg(D)), N, C.byref(cnt), C.byref(full)) == 0, lib.mhimx_last_error()
    assert lay.total < full.total
    assert lay.total / full.total < 0.6, lay.total / full.total                 # (include/mhimx.h states 0.45 / 0.53 / 0.54)


def test_null_teacher_and_merge_fields_are_accepted_where_the_mhim_step_refuses_them():
    lib = L.lib()
    cfg, lay, cnt = _cfg(), L.StepLayout(), L.StepCounts()
    assert not cfg.teacher.w1 and not cfg.student.q and not cfg.grad.wkv and cfg.k == 0
    assert lib.mhimx_pure_step_layout_of(C.byref(cfg), 512, C.byref(lay)) == 0
    assert lib.mhimx_step_counts_of(512, .03, .5, .9, C.byref(cnt)) == 0
    assert lib.mhimx_step_layout_of(C.byref(cfg), 512, C.byref(cnt), C.byref(lay)) < 0          # check_cfg is what it was


@pytest.mark.parametrize("what, kw, N, word", [
    ("N = 63", {}, 63, b"row count"),
    ("N above the row limit", {}, L.STEP_MAX_ROWS + 1, b"row count"),
    ("E = 256", {"E": 256}, 512, b"shapes"),
    ("A = 64", {"A": 64}, 512, b"shapes"),
    ("C = 5", {"Cc": 5}, 512, b"shapes"),
    ("C = 0", {"Cc": 0}, 512, b"shapes"),
    ("D = 1000", {"D": 1000}, 512, b"shapes"),
    ("a NULL student parameter", {"student": SIX[:3] + SIX[4:]}, 512, b"null student parameter"),
    ("a NULL gradient view", {"grad": SIX[1:]}, 512, b"null gradient view"),
    ("no tick", {"tick": False}, 512, b"tick"),
])
def test_refusals_are_errors_in_every_entry_point(what, kw, N, word):
    lib = L.lib()
    cfg, lay = _cfg(**kw), L.StepLayout()
    ws, x, lab = FAKE + (1 << 40), FAKE + (1 << 41), FAKE + (1 << 42)
    ld = max(cfg.D, 4)
    assert lib.mhimx_pure_step_layout_of(C.byref(cfg), N, C.byref(lay)) < 0, what
    msg = lib.mhimx_last_error()
    assert msg.startswith(b"pure_step:") and word in msg, (what, msg)
    for update in (0, 1):
        assert lib.mhimx_pure_step_run(None, C.byref(cfg), x, ld, N, lab, 7, 1, ws, 1 << 44, update) < 0, what
        assert lib.mhimx_last_error().startswith(b"pure_step:") and word in lib.mhimx_last_error(), what
    Xp, ldp, Np, lp, sd = (C.c_void_p * 1)(x), (C.c_int64 * 1)(ld), (C.c_int64 * 1)(N), (C.c_void_p * 1)(lab), (C.c_uint64 * 1)(7)
    assert lib.mhimx_pure_step_run_many(None, C.byref(cfg), 1, Xp, ldp, Np, lp, sd, 1, ws, 1 << 44) < 0, what
    assert word in lib.mhimx_last_error(), what


def test_run_refusals_of_its_own_arguments_without_a_device():
    lib = L.lib()
    cfg, lay, N = _cfg(), L.StepLayout(), 512
    assert lib.mhimx_pure_step_layout_of(C.byref(cfg), N, C.byref(lay)) == 0
    ws, x, lab = FAKE + (1 << 40), FAKE + (1 << 41), FAKE + (1 << 42)

    def run(cfg=cfg, x=x, ld=1024, N=N, lab=lab, ws=ws, ws_bytes=lay.total, update=1):
        r = lib.mhimx_pure_step_run(None, C.byref(cfg) if cfg is not None else None, x, ld, N, lab, 7, 1, ws, ws_bytes, update)
        return r, lib.mhimx_last_error()

    no_opt = _cfg()
    no_opt.m = None
    for kw, word in [
        (dict(cfg=None), b"null configuration"),
        (dict(x=None), b"null bag"),
        (dict(lab=None), b"null bag"),
        (dict(ws=None), b"null bag"),
        (dict(x=x + 4), b"row pitch"),                       # a bag that is not 16-byte aligned
        (dict(ld=1026), b"row pitch"),                       # a pitch that is not a multiple of 4 floats
        (dict(ld=512), b"row pitch"),                        # a pitch below D
        (dict(N=200000, ld=8192), b"row pitch"),             # N * ldx * 4 >= 2^32
        (dict(cfg=no_opt), b"flat optimiser buffers"),
        (dict(ws=ws + 64), b"256-byte aligned"),
        (dict(ws_bytes=lay.total - 1), b"workspace too small"),
    ]:
        r, msg = run(**kw)
        assert r < 0 and msg.startswith(b"pure_step") and word in msg, (kw, r, msg)
    assert lib.mhimx_pure_step_layout_of(C.byref(cfg), N, None) < 0
    assert lib.mhimx_pure_step_run_many(None, C.byref(cfg), 0, None, None, None, None, None, 1, ws, lay.total) < 0
    assert b"pure_step_run_many" in lib.mhimx_last_error()


def test_the_trainers_shape_check_mirrors_the_c_refusals():
    """FusedTrainer.pure_exec_shapes_ok - the tensor-free part of _exec_ok's pure branch - says no exactly where check_pure_cfg or
    mhimx_pure_step_run's own argument checks do: such a bag takes the Python path and never raises."""
    from mhim_mil_amd.engine import FusedTrainer
    lib = L.lib()
    ok = FusedTrainer.pure_exec_shapes_ok
    x0 = FAKE + (1 << 41)
    cases = [
        dict(), dict(N=64), dict(N=L.STEP_MAX_ROWS, D=256, pitch=256), dict(N=40000, D=1536, pitch=1536), dict(pitch=1028), dict(C=4), dict(C=1),
        dict(N=63), dict(N=L.STEP_MAX_ROWS + 1, D=256, pitch=256), dict(E=256), dict(A=64), dict(C=5), dict(C=0), dict(D=1000, pitch=1000),
        dict(D=0, pitch=4), dict(pitch=1026), dict(pitch=512), dict(N=200000, D=1024, pitch=8192), dict(ptr=x0 + 4), dict(inner=2),
    ]
    seen = set()
    for kw in cases:
        a = dict(N=512, D=1024, pitch=None, inner=1, ptr=x0, E=512, A=128, C=2)
        a.update(kw)
        if a["pitch"] is None:
            a["pitch"] = a["D"]
        cfg, lay = _cfg(D=a["D"], E=a["E"], A=a["A"], Cc=a["C"]), L.StepLayout()
        r = lib.mhimx_pure_step_layout_of(C.byref(cfg), a["N"], C.byref(lay))
        if r == 0 and a["inner"] == 1:             # (the C call takes rows of contiguous floats: a strided inner dimension has no C twin)
            r = lib.mhimx_pure_step_run(None, C.byref(cfg), a["ptr"], a["pitch"], a["N"], FAKE, 7, 1, FAKE + (1 << 40), lay.total - 1, 1)
            took = r < 0 and b"workspace too small" in lib.mhimx_last_error()      # every check before the workspace's passed
        else:
            took = False
        got = ok(a["N"], a["D"], a["pitch"], a["inner"], a["ptr"], E=a["E"], A=a["A"], C=a["C"], max_rows=L.STEP_MAX_ROWS)
        assert got == took, (kw, got, took, lib.mhimx_last_error())
        seen.add(got)
    assert seen == {True, False}
