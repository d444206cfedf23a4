"""The ragged accumulation window of the full MHIM(ABMIL) model (mhimx_ragged_window_layout_of / mhimx_ragged_window_run,
csrc/ragged_window.hip) without a GPU: the entry points are declared, exported and bound, the layout is pure host arithmetic, every refusal
is an error status raised before any device call and names the bag, the trainer's mirrored shape check agrees with the C checks, and
window_step's routing decision is the documented one.  Pointers handed over here are made-up addresses: a refused call never touches them."""
import ctypes as C
import os
import re

import pytest
import torch

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
X0, LAB0, WS = FAKE + (1 << 41), FAKE + (1 << 42), FAKE + (1 << 40)
K = 5
# bytes per row of the call's row space and per 256-row pool partial of the teacher (include/mhimx.h)
ROW_BYTES, PART_BYTES = 7265, 2056


def _cfg(D=1024, E=512, A=128, Cc=2, k=K, **over):
    p, t, g = L.StepParams(), L.StepParams(), L.StepGrads()
    for j, (n, _) in enumerate(L.StepParams._fields_):
        setattr(p, n, FAKE + 0x1000000 * (j + 1))
    for j, n in enumerate(("w1", "b1", "wa", "wc", "wp", "bp")):
        setattr(t, n, FAKE + 0x1000000 * (j + 40))
    for j, (n, _) in enumerate(L.StepGrads._fields_):
        setattr(g, n, FAKE + 0x1000000 * (j + 20))
    cfg = L.StepCfg(D=D, E=E, A=A, C=Cc, k=k, act=2, da_act=1, attn2score=1, student=p, teacher=t, grad=g, tick=FAKE + 4096,
                    p=FAKE + (1 << 36), g=FAKE + (2 << 36), m=FAKE + (3 << 36), v=FAKE + (4 << 36), n_train=1 << 22, n_all=1 << 22,
                    merge_mm=0.9999, temp_t=0.1, main_alpha=1.0, aux_alpha=0.5)
    for n, v in over.items():
        setattr(cfg, n, v)
    return cfg


def _counts(N):
    c = L.StepCounts()
    assert L.lib().mhimx_step_counts_of(N, 0.03, 0.5, 0.9, C.byref(c)) == 0, N
    return c


def _bags(ns, ldx=1024, x=X0, lab=LAB0, cnts=None):
    n = len(ns)
    ldx = ldx if isinstance(ldx, (list, tuple)) else [ldx] * n
    out = (L.RaggedWindowBag * max(n, 1))()
    for b in range(n):
        out[b].X, out[b].ldx, out[b].N = (x + (b << 33)) if x else None, ldx[b], ns[b]
        out[b].label_dev = (lab + 64 * b) if lab else None
        out[b].cnt = cnts[b] if cnts is not None else (_counts(ns[b]) if ns[b] >= 40 else L.StepCounts(1, 1, ns[b] - 1, 1, 1))
        out[b].seeds = L.StepSeeds(4 * b + 1, 4 * b + 2, 4 * b + 3, 4 * b + 4)
    return out


def _layout(ns, D=1024, **kw):
    lay = L.RaggedWindowLayout()
    r = L.lib().mhimx_ragged_window_layout_of(C.byref(_cfg(D, **kw)), len(ns), _bags(ns, ldx=D), C.byref(lay))
    return r, lay


# ------------------------------------------------------------------------------------------------------------------ 1
def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in ("mhimx_ragged_window_layout_of", "mhimx_ragged_window_run"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert int(re.search(r"#define MHIMX_RAGGED_WINDOW_MAX (\d+)", hdr).group(1)) == L.RAGGED_WINDOW_MAX == L.INFER_MAX
    assert int(re.search(r"#define MHIMX_RAGGED_WINDOW_MAX_ROWS (\d+)", hdr).group(1)) == L.RAGGED_WINDOW_MAX_ROWS
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == lib.mhimx_version() == 620
    assert C.sizeof(L.RaggedWindowBag) == 32 + C.sizeof(L.StepCounts) + C.sizeof(L.StepSeeds) == 104
    assert C.sizeof(L.RaggedWindowLayout) == 8 * (12 + L.RAGGED_WINDOW_MAX)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("ns,D", [([64, 257, 2100, 97], 256), ([64], 1024), ([91, 92, 96, 123, 124, 128], 512), ([16385, 64, 2100], 256),
                                  ([9000 + 255 * j for j in range(32)], 1536)])
def test_layout_is_host_arithmetic_slots_hold_the_bag_and_its_tokens(ns, D):
    r, lay = _layout(ns, D)
    assert r == 0, L.lib().mhimx_last_error()
    n, E = len(ns), 512
    assert lay.total > 0 and lay.total % 256 == 0
    slots = [(N + K + 31) // 32 * 32 for N in ns]
    assert lay.rows == sum(slots)
    row0 = list(lay.row0)[:n]
    assert row0[0] == 0 and all(r0 % 32 == 0 for r0 in row0)
    assert all(row0[b + 1] == row0[b] + slots[b] for b in range(n - 1)) and row0[-1] + ns[-1] + K <= lay.rows      # room for N + k rows
    sizes = {"logits": 4 * n * 16, "losses": 4 * n * 4, "score": lay.rows * 4, "rows_all": lay.rows * 8, "H_teacher": lay.rows * E * 4,
             "H_student": lay.rows * E * 4, "dact": lay.rows * E * 2, "dpre": lay.rows * E * 4, "z_teacher": 4 * n * E, "z_student": 4 * n * E}
    spans = []
    for name, nbytes in sizes.items():
        off = getattr(lay, name)
        assert off >= 0 and off % 256 == 0 and off + nbytes <= lay.total, (name, off, lay.total)
        spans.append((off, off + nbytes))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans            # no two of them overlap


def test_total_grows_by_the_documented_bytes_per_row_and_one_bag_beside_the_single_bag_step(capsys):
    """Beside a large bag (which sizes the per-bag scratch and saturates the split-K slab count) a second bag that grows by 16 384 rows -
    64 pool partials - adds exactly 16 384 x ROW_BYTES + 64 x PART_BYTES bytes: what include/mhimx.h and DESIGN.md state per row.  ``total``
    never shrinks when a bag grows.  The bytes of a one-bag window beside mhimx_step_layout_of's for the same bag are printed (DESIGN.md
    quotes them; no bound is set on the ratio)."""
    lib = L.lib()
    a, b = _layout([200000, 1024 - K])[1], _layout([200000, 1024 - K + 16384])[1]
    assert b.rows - a.rows == 16384
    assert b.total - a.total == 16384 * ROW_BYTES + 64 * PART_BYTES, (b.total - a.total) / 16384
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    assert "7 265 bytes per row" in hdr and "2 056 per 256-row pool partial" in hdr
    prev = 0
    for N in (64, 65, 91, 92, 500, 4096, 16384, 16385, 100000, 262144):
        r, lay = _layout([N])
        assert r == 0 and lay.total >= prev, N
        prev = lay.total
    totals = [_layout([700] * n)[1].total for n in range(1, 33)]
    assert all(y > x for x, y in zip(totals, totals[1:]))
    with capsys.disabled():
        for N in (64, 512, 10000, 59745):
            one, step = _layout([N])[1], L.StepLayout()
            assert lib.mhimx_step_layout_of(C.byref(_cfg()), N, C.byref(_counts(N)), C.byref(step)) == 0
            print(f"\n[ragged_window layout] N = {N} x 1024: one-bag window {one.total} bytes, mhimx_step_layout_of {step.total} bytes, "
                  f"ratio {one.total / step.total:.3f}", end="")
        print(f"\n[ragged_window layout] 8 x 10000 x 1024: {_layout([10000] * 8)[1].total} bytes")


# ------------------------------------------------------------------------------------------------------------------ 3
def _run(cfg, ns, bags, ws=WS, ws_bytes=1 << 44, update=1):
    lib = L.lib()
    r = lib.mhimx_ragged_window_run(None, C.byref(cfg) if cfg is not None else None, len(ns), bags, 1, ws, ws_bytes, update)
    return r, lib.mhimx_last_error()


def _bad_cnt(N, **kw):
    c = _counts(N)
    for n, v in kw.items():
        setattr(c, n, v)
    return c


@pytest.mark.parametrize("what, ckw, ns, ldx, cnts, word", [
    ("n = 0", {}, [], 1024, None, b"1..32 bags"),
    ("n = 33", {}, [64] * 33, 1024, None, b"1..32 bags"),
    ("N = 63", {}, [64, 63, 64], 1024, None, b"bag 1"),
    ("N above the per-bag limit", {"D": 256}, [64, 64, L.STEP_MAX_ROWS + 1], 256, [_counts(64), _counts(64), _counts(L.STEP_MAX_ROWS)], b"bag 2"),
    ("len_keep != N - n_sel", {}, [700, 700], 1024, [_counts(700), _bad_cnt(700, len_keep=600)], b"bag 1"),
    ("Lk + R != len_keep", {}, [700, 700], 1024, [_bad_cnt(700, R=3), _counts(700)], b"bag 0"),
    ("n_sel > k_top", {}, [700, 700, 700], 1024, [_counts(700), _counts(700), _bad_cnt(700, n_sel=50, len_keep=650, Lk=585, R=65)], b"bag 2"),
    ("k_top above the one-workgroup select's", {}, [9000], 1024, [_bad_cnt(9000, k_top=5000)], b"bag 0"),
    ("ldx < D", {}, [64, 64], [1024, 512], None, b"bag 1: row pitch"),
    ("ldx % 4 != 0", {}, [64, 64, 64], [1024, 1024, 1026], None, b"bag 2: row pitch"),
    ("N ldx 4 >= 2^32", {}, [64, 200000], [1024, 8192], None, b"bag 1: N * ldx * 4"),
    ("too many rows in the window", {"D": 256}, [L.STEP_MAX_ROWS - 32, L.STEP_MAX_ROWS - 32, 64], 256, None, b"bag 2: "),
    ("a non-NULL q_out", {"q_out": FAKE + 8192}, [64], 1024, None, b"q_out"),
    ("a side stream", {"side_stream": FAKE + 8192}, [64], 1024, None, b"side_stream"),
    ("time_project", {"time_project": 1}, [64], 1024, None, b"time_project"),
    ("D % 256 != 0", {"D": 1000}, [64], 1000, None, b"bag 0"),
    ("E != 512", {"E": 256}, [64], 1024, None, b"bag 0"),
    ("C = 5", {"Cc": 5}, [64], 1024, None, b"bag 0"),
    ("8 k > 48", {"k": 7}, [64], 1024, None, b"bag 0"),
])
def test_refusals_are_errors_in_both_entry_points_before_any_device_call(what, ckw, ns, ldx, cnts, word):
    lib = L.lib()
    cfg, lay = _cfg(**ckw), L.RaggedWindowLayout()
    bags = _bags(ns, ldx=ldx, cnts=cnts)
    assert lib.mhimx_ragged_window_layout_of(C.byref(cfg), len(ns), bags, C.byref(lay)) < 0, what
    msg = lib.mhimx_last_error()
    assert msg.startswith(b"ragged_window:") and word in msg, (what, msg)
    for update in (0, 1):
        r, msg = _run(cfg, ns, bags, update=update)
        assert r < 0 and msg.startswith(b"ragged_window:") and word in msg, (what, msg)


def test_run_refusals_of_its_own_arguments_without_a_device():
    lib = L.lib()
    ns = [700, 64, 97]
    r, lay = _layout(ns)
    assert r == 0
    cfg, no_opt = _cfg(), _cfg()
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
        a = dict(cfg=cfg, ns=ns, bags=_bags(ns), ws_bytes=lay.total)
        a.update(kw)
        r, msg = _run(**a)
        assert r < 0 and msg.startswith(b"ragged_window") and word in msg, (kw, r, msg)
    r, msg = _run(no_opt, ns, _bags(ns), update=0, ws_bytes=lay.total - 1)
    assert r < 0 and b"workspace too small" in msg                  # update = 0 does not need the optimiser's buffers
    assert lib.mhimx_ragged_window_layout_of(C.byref(cfg), 3, _bags(ns), None) < 0
    assert lib.mhimx_ragged_window_layout_of(C.byref(cfg), 3, None, C.byref(L.RaggedWindowLayout())) < 0
    assert lib.mhimx_ragged_window_layout_of(None, 3, _bags(ns), C.byref(L.RaggedWindowLayout())) < 0


# ------------------------------------------------------------------------------------------------------------------ 4
def test_the_trainers_shape_check_mirrors_the_c_refusals():
    """FusedTrainer.ragged_window_shapes_ok says no exactly where check_rw (check_cfg per bag) or mhimx_ragged_window_run's own argument
    checks do: such a window takes today's route and never raises."""
    from mhim_mil_amd.engine import FusedTrainer
    lib = L.lib()
    ok = FusedTrainer.ragged_window_shapes_ok
    big = L.STEP_MAX_ROWS
    cases = [
        dict(ns=[64, 257, 2100, 97], D=256), dict(ns=[64]), dict(ns=[700] * 32), dict(ns=[16385, 64], D=256), dict(ns=[700], C=4), dict(ns=[700], C=1),
        dict(ns=[big - 32, big - 32], D=256), dict(ns=[700, 700], pitch=[1024, 1028]), dict(ns=[700], k=6),
        dict(ns=[]), dict(ns=[64] * 33), dict(ns=[64, 63]), dict(ns=[big + 1], D=256, cnt={0: _counts(big)}), dict(ns=[big - 32, big - 32, 64], D=256),
        dict(ns=[64], E=256), dict(ns=[64], A=64), dict(ns=[64], C=5), dict(ns=[64], C=0), dict(ns=[64], D=1000), dict(ns=[64], k=7), dict(ns=[64], k=0),
        dict(ns=[64, 64], pitch=[1024, 1026]), dict(ns=[64, 64], pitch=[512, 1024]), dict(ns=[64, 200000], pitch=[1024, 8192]),
        dict(ns=[64, 64], ptr_off=[0, 4]), dict(ns=[64, 64], ptr_null=1), dict(ns=[64, 64], inner=[1, 2]), dict(ns=[64, 64], bagD=[1024, 512]),
        dict(ns=[700, 700], cnt={1: _bad_cnt(700, len_keep=600)}), dict(ns=[700], cnt={0: _bad_cnt(700, R=3)}),
        dict(ns=[9000], cnt={0: _bad_cnt(9000, k_top=5000)}), dict(ns=[700], cnt={0: _bad_cnt(700, n_sel=50, len_keep=650, Lk=585, R=65)}),
        dict(ns=[700], cnt={0: _bad_cnt(700, n_sel=0, len_keep=700, Lk=630, R=70)}),
    ]
    seen = set()
    for kw in cases:
        a = dict(D=1024, E=512, A=128, C=2, k=K, pitch=None, ptr_off=None, ptr_null=None, inner=None, bagD=None, cnt={})
        a.update(kw)
        ns, n = a["ns"], len(a["ns"])
        pitch = a["pitch"] or [a["D"]] * n
        ptrs = [X0 + (b << 33) + (a["ptr_off"][b] if a["ptr_off"] else 0) for b in range(n)]
        if a["ptr_null"] is not None:
            ptrs[a["ptr_null"]] = 0
        inner = a["inner"] or [1] * n
        bagD = a["bagD"] or [a["D"]] * n
        cnts = [a["cnt"].get(b) or (_counts(ns[b]) if ns[b] >= 40 else L.StepCounts(1, 1, ns[b] - 1, 1, 1)) for b in range(n)]
        cfg, lay = _cfg(D=a["D"], E=a["E"], A=a["A"], Cc=a["C"], k=a["k"]), L.RaggedWindowLayout()
        bags = _bags(ns, ldx=pitch, cnts=cnts)
        for b in range(n):
            bags[b].X = ptrs[b] or None
        took = False
        # (the C call takes rows of contiguous floats of the model's width: a strided inner dimension or another width has no C twin)
        if all(i == 1 for i in inner) and all(d == a["D"] for d in bagD):
            r = lib.mhimx_ragged_window_layout_of(C.byref(cfg), n, bags, C.byref(lay))
            if r == 0:
                r = lib.mhimx_ragged_window_run(None, C.byref(cfg), n, bags, 1, WS, lay.total - 1, 1)
                took = r < 0 and b"workspace too small" in lib.mhimx_last_error()      # every check before the workspace's passed
        got = ok([(ns[b], bagD[b], pitch[b], inner[b], ptrs[b], (cnts[b].k_top, cnts[b].n_sel, cnts[b].len_keep, cnts[b].Lk, cnts[b].R))
                  for b in range(n)], a["D"], a["k"], E=a["E"], A=a["A"], C=a["C"], max_rows=big, row_cap=L.RAGGED_WINDOW_MAX_ROWS,
                 max_bags=L.RAGGED_WINDOW_MAX)
        assert got == took, (kw, got, took, lib.mhimx_last_error())
        seen.add(got)
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------------------------ 5
class _FakeBag:
    """What window_step's routing reads of a bag: shape and strides."""

    def __init__(self, n, d=256):
        self.shape, self._stride = (n, d), (d, 1)

    def stride(self, j=None):
        return self._stride if j is None else self._stride[j]

    def dim(self):
        return 2


def _trainer(accum=3):
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    cfg = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999,
               merge_ratio=0.9, temp_t=0.1, dropout=0.0)
    s, t = (MHIM(input_dim=256, n_classes=2, baseline="attn", **cfg).train() for _ in range(2))
    tr = FusedTrainer(s, t, accumulation_steps=accum)
    s._check_x = lambda b: b
    calls = []
    tr._exec_ragged_window = lambda xs, labels, i, update: calls.append(("ragged", len(xs))) or ([], [])
    tr._exec_window = lambda xs, labels, i, update: calls.append(("window", len(xs))) or ([], [])
    tr.train_step = lambda b, l, i=None, **kw: calls.append(("bag", sorted(kw))) or (None, None)
    tr.window_ok = lambda xs, i=None: True
    tr._exec_window_ok = lambda xs, labels, i=None: True
    return tr, calls


def test_window_step_routing_decision(monkeypatch):
    """Different-sized bags and a shorter last window take mhimx_ragged_window_run; a full window of same-shaped bags keeps
    mhimx_window_run; injected draws keep the bag-after-bag route; so does MHIMX_STEP_EXEC=0 (the trainer's use_executor), decided by the
    real _ragged_window_ok before it looks at any tensor.  The runs themselves are stubs: no device."""
    from mhim_mil_amd import engine as EN
    labels = [0, 1, 0]
    tr, calls = _trainer()
    tr._ragged_window_ok = lambda xs, labels, i=None: True
    tr.window_step([_FakeBag(64), _FakeBag(257), _FakeBag(97)], labels)
    tr.window_step([_FakeBag(64), _FakeBag(257)], labels[:2])                                # a shorter last window
    tr.window_step([_FakeBag(300)] * 3, labels)                                              # one shape, a full window
    tr.window_step([_FakeBag(64), _FakeBag(257), _FakeBag(97)], labels, perms=[None] * 3, shuffles=[None] * 3)
    assert calls == [("ragged", 3), ("ragged", 2), ("window", 3)] + [("bag", ["ids_shuffle", "perm"])] * 3, calls
    # MHIMX_STEP_EXEC=0 is read when a trainer is made
    monkeypatch.setenv("MHIMX_STEP_EXEC", "0")
    tr0, calls0 = _trainer()
    assert tr0.use_executor is False
    tr0.window_ok = lambda xs, i=None: False                                                  # (today's route for such a window: bag after bag)
    tr0.window_step([_FakeBag(64), _FakeBag(257), _FakeBag(97)], labels)
    assert calls0 == [("bag", [])] * 3, calls0
    # and the real check also says no to: a kernel event hook, a ratio schedule, several processes, merge_k > 6, prec = "f32"
    monkeypatch.delenv("MHIMX_STEP_EXEC")
    tr1, _ = _trainer()
    assert tr1.use_executor is True
    xs = [torch.zeros(64, 256), torch.zeros(97, 256)]
    assert tr1._ragged_window_ok(xs, labels[:2]) is False                                    # (host tensors: not a device window)
    monkeypatch.setattr(EN.ops, "KERNEL_EVENT_HOOK", lambda *a: None)
    assert tr1._ragged_window_ok(xs, labels[:2]) is False
