"""TransMIL attention maps and instance scores from the ragged call (mhimx_infer_transmil_attn_ws_bytes / mhimx_infer_transmil_run_attn,
csrc/infer_transmil.hip) without a GPU: the entry points exist and are bound, the workspace size is host arithmetic with the plain call's
layout as its prefix, every refusal is an error status raised before any device call (pointers handed over here are made-up addresses: a
refused call never touches them), the ops mirror agrees with the C checks case by case, ops.infer_transmil_many without the new keywords
makes the old call (stubbed library), and MHIM.infer_cls_attn / infer_cls_topk take the routes and keep the books they promise (stubbed
ops, shape-only bags)."""
import ctypes as C
import itertools
import os
import re
import types

import pytest
import torch

from mhim_mil_amd import _lib as L
from mhim_mil_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
PARAMS = ("w1", "b1", "cls_token", "w7", "w5", "w3", "b7", "b5", "b3", "norm_w", "norm_b", "wp", "bp")
LAYER = ("ln_w", "ln_b", "w_qkv", "w_out", "b_out", "conv_w")
NEW = ("mhimx_infer_transmil_attn_ws_bytes", "mhimx_infer_transmil_run_attn")
ATTN, PSCORE = FAKE + (1 << 38), FAKE + (1 << 39)


def _cfg(D=256, Cc=2, act=2, params=True, layer_kw=None, **kw):
    p = {n: FAKE + 0x1000000 * (k + 1) for k, n in enumerate(PARAMS)} if params else {}
    p.update(kw)
    cfg = L.InferTransmilCfg(D=D, C=Cc, act=act, **p)
    for j in range(2):
        ly = {n: FAKE + 0x100000000 + 0x1000000 * (6 * j + k) for k, n in enumerate(LAYER)} if params else {}
        if layer_kw and j == 1:
            ly.update(layer_kw)
        cfg.layer[j] = L.TransmilLayer(**ly)
    return cfg


def _bags(ns, ldx=256, x=FAKE + 0x200000000):
    return (L.InferBag * max(len(ns), 1))(*[L.InferBag(X=x + 0x10000000 * j if x else None, ldx=ldx, N=n) for j, n in enumerate(ns)])


def _ws(cfg, ns, pscore=None, **kw):
    lib = L.lib()
    if pscore is None:
        return lib.mhimx_infer_transmil_ws_bytes(C.byref(cfg), len(ns), _bags(ns, **kw))
    return lib.mhimx_infer_transmil_attn_ws_bytes(C.byref(cfg), len(ns), _bags(ns, **kw), pscore)


def _run(cfg, ns, bags=None, x_dtype=0, ws=FAKE + (1 << 36), ws_bytes=1 << 44, labels=None, logits=FAKE + 4096, loss=None, attn=ATTN, pscore=None):
    lib = L.lib()
    r = lib.mhimx_infer_transmil_run_attn(None, C.byref(cfg) if cfg is not None else None, len(ns), _bags(ns) if bags is None else bags, labels,
                                          logits, loss, None, attn, pscore, ws, ws_bytes, x_dtype)
    return r, lib.mhimx_last_error()


def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert L.ABI_VERSION == 620 and lib.mhimx_version() == 620
    sec = hdr[hdr.index("TransMIL attention maps and instance scores from the ragged call"):hdr.index("int64_t mhimx_infer_transmil_attn_ws_bytes")]
    for cite in ("nystrom_attention.py:143-150", "baseline.py:244-288", "scoring.py:9-34", "mhim.py:207-227,250-260", "96 + 4 (+ 4 with pscore)",
                 "MHIMX_VERSION stays 620"):
        assert cite in sec, cite


def test_the_workspace_has_the_plain_layout_as_its_prefix_and_grows_with_the_pseudo_score():
    for cc, ns in ((2, [1]), (2, [1, 255, 256, 2100]), (5, [600, 7]), (16, [4200] * 32)):
        cfg = _cfg(Cc=cc)
        base, attn, both = _ws(cfg, ns), _ws(cfg, ns, 0), _ws(cfg, ns, 1)
        nb, R = len(ns), sum(ns)
        rows = max(R, 32)
        al = lambda b: (b + 255) // 256 * 256
        assert base > 0 and attn == base + 2 * al(nb * 8 * 256 * 4), (cc, ns)
        assert both == attn + 2 * al(rows * 512 * 4) + al(rows * cc * 4) and both > attn >= base, (cc, ns)
        assert both % 256 == 0 and attn % 256 == 0
        lo = L.InferTransmilLayout()
        assert L.lib().mhimx_infer_transmil_layout_of(C.byref(cfg), nb, _bags(ns), C.byref(lo)) == 0 and lo.total == base
    assert ops.infer_transmil_attn_ws_bytes(_cfg(), [types.SimpleNamespace(data_ptr=lambda: FAKE, stride=lambda k: 256, shape=(7, 256))], True) \
        == _ws(_cfg(), [7], 1)


@pytest.mark.parametrize("what, cfg_kw, ns, bag_kw, x_dtype, word", [
    ("C = 17", {"Cc": 17}, [10], {}, 0, b"shapes outside"),
    ("C = 0", {"Cc": 0}, [10], {}, 0, b"shapes outside"),
    ("D = 1000", {"D": 1000}, [10], {"ldx": 1000}, 0, b"shapes outside"),
    ("N = 0", {}, [10, 0, 10], {}, 0, b"bag 1"),
    ("33 bags", {}, [10] * 33, {}, 0, b"bags per call"),
    ("no bags", {}, [], {}, 0, b"bags per call"),
    ("pitch below D", {}, [10], {"ldx": 128}, 0, b"bag 0"),
    ("half pitch not a multiple of 8", {}, [10, 10], {"ldx": 260}, 1, b"bag 0"),
    ("null X", {}, [10], {"x": 0}, 0, b"bag 0: null or unaligned"),
    ("misaligned X", {}, [10, 10], {"x": FAKE + 4}, 0, b"bag 0: null or unaligned"),
    ("bad x_dtype", {}, [10], {}, 3, b"x_dtype 3"),
    ("activation code", {"act": 9}, [10], {}, 0, b"activation"),
])
def test_everything_the_plain_call_refuses_is_refused_before_any_device_call(what, cfg_kw, ns, bag_kw, x_dtype, word):
    lib = L.lib()
    cfg = _cfg(**cfg_kw)
    bags = _bags(ns, **bag_kw)
    r, msg = _run(cfg, ns, bags=bags, x_dtype=x_dtype, pscore=PSCORE)
    assert r < 0 and msg.startswith(b"infer_transmil_attn:") and word in msg, (what, r, msg)
    if x_dtype == 0 and "x" not in bag_kw:          # the host-only entry point sees neither the element type nor the pointers
        assert lib.mhimx_infer_transmil_attn_ws_bytes(C.byref(cfg), len(ns), bags, 1) < 0 and word in lib.mhimx_last_error(), what


RUN_CASES = [
    (dict(cfg=None), b"null"),
    (dict(cfg=_cfg(params=False)), b"null parameter"),
    (dict(cfg=_cfg(wp=0)), b"null parameter"),
    (dict(cfg=_cfg(layer_kw={"conv_w": 0})), b"null parameter"),
    (dict(cfg=_cfg(w1=FAKE + 8)), b"16-byte aligned"),
    (dict(cfg=_cfg(layer_kw={"w_qkv": FAKE + 4})), b"16-byte aligned"),
    (dict(logits=None), b"logits output is required"),
    (dict(loss=FAKE + 8192), b"needs labels"),
    (dict(attn=None), b"attention output is required"),
    (dict(attn=None, pscore=PSCORE), b"attention output is required"),
    (dict(attn=ATTN + 4), b"outputs must be 16-byte aligned"),
    (dict(pscore=PSCORE + 8), b"outputs must be 16-byte aligned"),
    (dict(ws=None), b"256-byte aligned"),
    (dict(ws=FAKE + 64), b"256-byte aligned"),
    (dict(ws_bytes=-1), b"workspace too small"),                  # (-1: one byte below what THIS call needs)
    (dict(ws_bytes=-1, pscore=PSCORE), b"workspace too small"),
    (dict(ws_bytes="plain"), b"workspace too small"),            # (the plain call's size does not hold the tail's buffers)
]


def test_run_refusals_without_a_device():
    lib = L.lib()
    cfg, ns = _cfg(), [100, 7]
    for kw, word in RUN_CASES:
        args = dict(cfg=cfg, ns=ns)
        args.update(kw)
        need = _ws(cfg, ns, int(args.get("pscore") is not None))
        wb = args.get("ws_bytes", need)
        args["ws_bytes"] = need - 1 if wb == -1 else _ws(cfg, ns) if wb == "plain" else wb
        r, msg = _run(**args)
        assert r < 0 and word in msg and msg.startswith(b"infer_transmil_attn:"), (kw, r, msg)
    assert lib.mhimx_infer_transmil_attn_ws_bytes(None, 1, _bags([1]), 0) < 0
    assert lib.mhimx_infer_transmil_attn_ws_bytes(C.byref(cfg), 1, None, 1) < 0


def test_the_ops_mirror_agrees_with_the_c_checks_case_by_case():
    """ops.infer_transmil_attn_args_ok says no exactly where the C call's own checks (behind the plain call's) do.  The probe: a workspace
    one byte short - "workspace too small" is the call's LAST check, so that message means every check before it passed (and no call made
    here goes on to a launch)."""
    cfg, ns = _cfg(), [100, 7]
    seen = set()
    for attn, pscore in itertools.product((ATTN, 0, ATTN + 4, ATTN + 8, ATTN + 16), (0, PSCORE, PSCORE + 4, PSCORE + 8, PSCORE + 32)):
        need = _ws(cfg, ns, int(pscore != 0))
        r, msg = _run(cfg, ns, attn=attn or None, pscore=pscore or None, ws_bytes=need - 1)
        assert r < 0
        took = b"workspace too small" in msg
        assert ops.infer_transmil_attn_args_ok(attn, pscore, need, need) == took, (attn, pscore, msg)
        assert not ops.infer_transmil_attn_args_ok(attn, pscore, need - 1, need)
        seen.add(took)
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------ ops.infer_transmil_many over a stubbed library
class _Lib:
    """Records every call; the two workspace queries answer ``need``."""

    def __init__(self, need):
        self.calls, self.need = [], need

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return self.need if name.endswith("ws_bytes") else 0
        return call


def _stubbed(monkeypatch, ns, need=4096):
    lib = _Lib(need)
    fronts = []
    ws = torch.zeros(need, dtype=torch.uint8)

    def front(who, query, cfg, xs, labels, ws_, ws_args=()):
        fronts.append((who, query, tuple(ws_args)))
        return len(ns), L.X_F16, "table", ws, torch.device("cpu"), [0] + list(itertools.accumulate(ns))
    monkeypatch.setattr(L, "lib", lambda: lib)
    monkeypatch.setattr(ops, "_infer_front", front)
    monkeypatch.setattr(ops, "_stream", lambda: "stream")
    return lib, fronts, ws


def test_without_the_new_keywords_the_wrapper_makes_the_old_call(monkeypatch):
    ns = [5, 300, 1]
    lib, fronts, ws = _stubbed(monkeypatch, ns)
    cfg = _cfg(Cc=3)
    labels = torch.zeros(3, dtype=torch.int64)
    r = ops.infer_transmil_many(cfg, ["x"] * 3, labels=labels, want_z=True)
    assert fronts == [("infer_transmil_many", "mhimx_infer_transmil_ws_bytes", ())]
    assert [c[0] for c in lib.calls] == ["mhimx_infer_transmil_layout_of", "mhimx_infer_transmil_run"]
    args = lib.calls[1][1]
    assert len(args) == 11 and args[0] == "stream" and args[2] == 3 and args[3] == "table" and args[9] == ws.numel() and args[10] == L.X_F16
    assert [a.value for a in args[4:9]] == [t.data_ptr() for t in (labels, r.logits, r.loss, r.z, ws)]
    assert r.attn is None and r.pscore is None and r.offsets == [0, 5, 305, 306] and r.logits.shape == (3, 3)
    with pytest.raises(L.MhimxError, match="without want_attn"):
        ops.infer_transmil_many(cfg, ["x"] * 3, attn=torch.zeros(16 * 306))


@pytest.mark.parametrize("pseudo", [False, True])
def test_with_them_it_calls_the_new_entry_point(monkeypatch, pseudo):
    ns = [5, 300, 1]
    lib, fronts, ws = _stubbed(monkeypatch, ns)
    cfg = _cfg()
    r = ops.infer_transmil_many(cfg, ["x"] * 3, want_attn=True, want_pscore=pseudo)
    assert fronts == [("infer_transmil_many", "mhimx_infer_transmil_attn_ws_bytes", (int(pseudo),))]
    assert [c[0] for c in lib.calls] == ["mhimx_infer_transmil_layout_of", "mhimx_infer_transmil_attn_ws_bytes", "mhimx_infer_transmil_run_attn"]
    assert lib.calls[1][1][3] == int(pseudo)
    args = lib.calls[2][1]
    assert len(args) == 13 and args[0] == "stream" and args[2] == 3 and args[11] == ws.numel() and args[12] == L.X_F16
    assert args[8].value == r.attn.data_ptr() and r.attn.shape == (2, 8, 306) and r.offsets == [0, 5, 305, 306]
    assert (args[9].value == r.pscore.data_ptr() and r.pscore.shape == (306,)) if pseudo else (args[9] is None and r.pscore is None)
    # want_pscore alone implies the maps; the mirror refuses a workspace below the call's size before the library sees the call
    r2 = ops.infer_transmil_many(cfg, ["x"] * 3, want_pscore=True)
    assert r2.attn.shape == (2, 8, 306) and r2.pscore.shape == (306,)
    lib.need = 8192
    del lib.calls[:]
    with pytest.raises(L.MhimxError, match="workspace hold 8192 bytes"):
        ops.infer_transmil_many(cfg, ["x"] * 3, want_attn=True)
    assert "mhimx_infer_transmil_run_attn" not in [c[0] for c in lib.calls]


# ------------------------------------------------------------------------------------------------ MHIM.infer_cls_attn / infer_cls_topk over stubbed ops
D, CC = 256, 3
ROWS = (64, 257, 97)


class _FakeBag:
    """Shape-only stand-in for a GPU bag: what _infer_bags, _infer_ok, infer_chunks and the routes read."""
    is_cuda = True

    def __init__(self, n, d=D, dtype=torch.float32, ptr=FAKE, pitch=None):
        self.shape, self.dtype, self.device, self._ptr, self._pitch = (n, d), dtype, torch.device("cpu"), ptr, pitch or d

    def dim(self):
        return 2

    def stride(self, k):
        return self._pitch if k == 0 else 1

    def data_ptr(self):
        return self._ptr

    def element_size(self):
        return 4 if self.dtype == torch.float32 else 2

    def float(self):
        return self if self.dtype == torch.float32 else _FakeBag(self.shape[0], self.shape[1], torch.float32, FAKE + 0x1000)

    def contiguous(self):
        return self


def _build(monkeypatch, state="eval", baseline="selfattn"):
    from mhim_mil_amd.mhim import MHIM
    torch.manual_seed(0)
    m = MHIM(n_classes=CC, input_dim=D, merge_enable=False, baseline=baseline, **({"prec": "f32"} if state == "f32" else {}))
    m.train(state == "train")
    m.merge_test = state == "merge_test"
    calls = []

    def forward_test(x, return_attn=False, no_norm=False, return_act=False, **kw):
        assert not kw and return_attn and not no_norm
        calls.append(("forward_test", x.dtype, return_act))
        for _ in range(3):
            m._next_seed()
        n = x.shape[0] + (5 if m.merge_test else 0)               # (merge_test scores N + k tokens)
        maps = [torch.full((1, 8, n), float(l + 1)) for l in range(2)]
        return torch.zeros(1, CC), ([maps, torch.zeros(1, 8, n, 64)] if return_act else maps)

    def trans_score(v, attn0):
        calls.append(("trans_score", tuple(v.shape), tuple(attn0.shape)))
        m._next_seed()
        return torch.arange(v.shape[0], dtype=torch.float32)
    m.forward_test, m._trans_score = forward_test, trans_score

    def infer_transmil_many(cfg, xs, labels=None, **kw):
        assert labels is None or (labels.dtype == torch.int64 and labels.is_contiguous())
        calls.append(("infer_transmil_many", cfg, len(xs), tuple(x.dtype for x in xs), tuple(sorted(kw.items())), None if labels is None else labels.numel()))
        offs = [0] + list(itertools.accumulate(int(x.shape[0]) for x in xs))
        R = offs[-1]
        return types.SimpleNamespace(logits=torch.zeros(len(xs), CC), loss=None if labels is None else torch.zeros(len(xs)), offsets=offs,
                                     attn=torch.arange(16 * R, dtype=torch.float32).view(2, 8, R),
                                     pscore=torch.arange(R, dtype=torch.float32) if kw.get("want_pscore") else None)

    def topk_many(score, offsets, k, largest=True):
        calls.append(("topk_many", score.data_ptr(), score.numel(), list(offsets), k, largest))
        return torch.zeros(len(offsets) - 1, k, dtype=torch.int64), torch.zeros(len(offsets) - 1, k)
    monkeypatch.setattr(ops, "infer_transmil_many", infer_transmil_many)
    monkeypatch.setattr(ops, "infer_transmil_cfg", lambda *a: "transmil_cfg")
    monkeypatch.setattr(ops, "topk_many", topk_many)
    if state == "hook":
        monkeypatch.setattr(ops, "KERNEL_EVENT_HOOK", lambda *a: None)
    return m, calls


def _xs(count, dtype=torch.float32, **kw):
    return [_FakeBag(ROWS[j % 3], dtype=dtype, ptr=FAKE + 0x10000000 * j, **kw) for j in range(count)]


@pytest.mark.parametrize("pseudo", [False, True])
def test_the_native_route_and_its_books(monkeypatch, pseudo):
    m, calls = _build(monkeypatch)
    m._step = 1000
    labels = torch.arange(3) % CC
    logits, attn, ps, loss = m.infer_cls_attn(_xs(3, torch.float16), labels=labels, pseudo=pseudo)
    assert calls == [("infer_transmil_many", "transmil_cfg", 3, (torch.float16,) * 3, (("want_attn", True), ("want_pscore", pseudo)), 3)]
    assert m._step == 1009 and m.last["infer_native"] is True and m.last["infer_calls"] == 1
    assert logits.shape == (3, CC) and loss.shape == (3,) and [tuple(a.shape) for a in attn] == [(2, 8, n) for n in ROWS]
    packed, pp, offs = m.last["infer_attn"]
    assert offs == [0, 64, 321, 418] and packed.shape == (2, 8, 418) and (pp is None) == (not pseudo)
    for j, a in enumerate(attn):                                   # views of the call's own buffer
        assert a.data_ptr() == packed[:, :, offs[j]:].data_ptr() and torch.equal(a, packed[:, :, offs[j]:offs[j + 1]])
    if pseudo:
        assert [tuple(p.shape) for p in ps] == [(n,) for n in ROWS] and torch.equal(torch.cat(ps), pp)
    else:
        assert ps is None
    # 33 bags: two calls, the packed rows of both, offsets over all bags; without labels three results
    del calls[:]
    out = m.infer_cls_attn(_xs(33), pseudo=pseudo)
    assert len(out) == 3 and [c[2] for c in calls] == [32, 1] and m.last["infer_calls"] == 2 and m._step == 1009 + 99
    packed, pp, offs = m.last["infer_attn"]
    assert len(offs) == 34 and packed.shape == (2, 8, offs[-1]) and len(out[1]) == 33 and out[1][32].shape == (2, 8, ROWS[32 % 3])
    with pytest.raises(L.MhimxError, match="2 labels for 3 bags"):
        m.infer_cls_attn(_xs(3), labels=torch.zeros(2, dtype=torch.int64))
    empty = m.infer_cls_attn([], pseudo=pseudo)
    assert empty[0].shape == (0, CC) and empty[1] == [] and m.last["infer_native"] is False and m.last["infer_attn"][2] == [0]


@pytest.mark.parametrize("state", ["train", "merge_test", "f32", "hook", "mixed", "pitch"])
@pytest.mark.parametrize("pseudo", [False, True])
def test_what_the_call_refuses_takes_the_loop_and_returns_the_same_shapes(monkeypatch, state, pseudo):
    m, calls = _build(monkeypatch, state if state not in ("mixed", "pitch") else "eval")
    xs = _xs(3)
    if state == "mixed":
        xs[1] = _FakeBag(ROWS[1], dtype=torch.float16)
    if state == "pitch":
        xs[1] = _FakeBag(ROWS[1], pitch=128)
    m._step = 1000
    logits, attn, ps = m.infer_cls_attn(xs, pseudo=pseudo)
    assert [c[0] for c in calls] == (["forward_test", "trans_score"] if pseudo else ["forward_test"]) * 3
    assert all(c[1] == torch.float32 and c[2] == pseudo for c in calls if c[0] == "forward_test") or state == "pitch"
    assert m._step == 1009 and m.last["infer_native"] is False and m.last["infer_calls"] == 0
    assert logits.shape == (3, CC) and [tuple(a.shape) for a in attn] == [(2, 8, n) for n in ROWS]
    assert all(torch.equal(a[l], torch.full((8, a.shape[2]), float(l + 1))) for a in attn for l in range(2))
    packed, pp, offs = m.last["infer_attn"]
    assert offs == [0, 64, 321, 418] and packed.shape == (2, 8, 418) and packed.is_contiguous()
    if pseudo:
        assert [c[1:] for c in calls if c[0] == "trans_score"] == [((n, 512), (8, n)) for n in ROWS]
        assert [tuple(p.shape) for p in ps] == [(n,) for n in ROWS] and pp.shape == (418,)
    else:
        assert ps is None and pp is None


def test_a_model_that_is_not_transmil_is_refused(monkeypatch):
    for baseline in ("attn", "dsmil"):
        m, calls = _build(monkeypatch, baseline=baseline)
        with pytest.raises(L.MhimxError, match="infer_many\\(return_attn=True\\)"):
            m.infer_cls_attn(_xs(2))
        with pytest.raises(L.MhimxError, match="infer_many\\(return_attn=True\\)"):
            m.infer_cls_topk(_xs(2), 2)
        assert calls == []


def test_infer_cls_topk_ranks_on_the_chunk_s_own_buffers(monkeypatch):
    m, calls = _build(monkeypatch)
    m._step = 1000
    logits, idx, val, loss = m.infer_cls_topk(_xs(33), 4, largest=False, labels=torch.zeros(33, dtype=torch.int64))
    native = [c for c in calls if c[0] == "infer_transmil_many"]
    tk = [c for c in calls if c[0] == "topk_many"]
    assert [c[4] for c in native] == [(("want_attn", True), ("want_pscore", True))] * 2 and len(tk) == 2
    assert [(c[2], len(c[3]) - 1, c[4], c[5]) for c in tk] == [(sum(ROWS[j % 3] for j in range(32)), 32, 4, False), (ROWS[32 % 3], 1, 4, False)]
    assert idx.shape == (33, 4) and val.shape == (33, 4) and idx.dtype == torch.int64 and logits.shape == (33, CC) and loss.shape == (33,)
    assert m._step == 1099 and m.last["infer_topk"][0] is idx and m.last["infer_native"] is True
    del calls[:]
    logits, idx, val = m.infer_cls_topk(_xs(3), 2, by="heads", layer=1)
    native = [c for c in calls if c[0] == "infer_transmil_many"]
    tk = [c for c in calls if c[0] == "topk_many"]
    assert [c[4] for c in native] == [(("want_attn", True), ("want_pscore", False))] and len(tk) == 8
    R = sum(ROWS)
    assert all(c[2] == R and c[3] == [0, 64, 321, 418] and c[4] == 2 and c[5] is True for c in tk)
    assert [c[1] - tk[0][1] for c in tk] == [4 * R * h for h in range(8)]          # head h of ONE layer of the chunk's buffer, in place
    assert idx.shape == (3, 8, 2) and val.shape == (3, 8, 2)
    for kw, word in ((dict(k=0), "k=0"), (dict(k=L.TOPK_MAX_K + 1), "must be in"), (dict(k=2, by="attn"), "by='attn'"), (dict(k=2, layer=2), "layer=2")):
        with pytest.raises(L.MhimxError, match=word):
            m.infer_cls_topk(_xs(3), **kw)
    # the loop's packs are ranked the same way
    mt, calls = _build(monkeypatch, "train")
    _, idx, val = mt.infer_cls_topk(_xs(3), 2, by="heads")
    assert idx.shape == (3, 8, 2) and len([c for c in calls if c[0] == "topk_many"]) == 8 and mt.last["infer_native"] is False
    # infer_topk itself keeps refusing TransMIL
    with pytest.raises(L.MhimxError, match="one attention map per layer"):
        m.infer_topk(_xs(3), 2)
