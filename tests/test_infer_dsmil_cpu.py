"""Ragged multi-bag DSMIL inference (mhimx_infer_dsmil_ws_bytes / mhimx_infer_dsmil_run, csrc/infer_dsmil.hip) without a GPU: the entry
points exist and are bound, the workspace size is pure host arithmetic, every refusal is an error status raised before any device call
(pointers handed over here are made-up addresses: a refused call never touches them), MHIM._infer_ok mirrors the C checks, and the seeds
the GPU parity test uses meet its arg-max gap condition on the oracle's own data."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from mhim_mil_amd import _lib as L
from tests import test_infer_dsmil_gpu as DD          # (the parity test's data: built on the CPU, no device touched at import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
PARAMS = ("w1", "b1", "wi", "bi", "wq0", "bq0", "wq2", "bq2", "wv", "bv", "wfcc", "bfcc")


def _cfg(D=256, E=512, Cc=2, act=2, params=True, **kw):
    p = {n: FAKE + 0x1000000 * (k + 1) for k, n in enumerate(PARAMS)} if params else {}
    p.update(kw)
    return L.InferDsmilCfg(D=D, E=E, C=Cc, act=act, cls_attn=1, no_norm=0, **p)


def _bags(ns, ldx=256, x=FAKE + 0x100000000):
    return (L.InferBag * max(len(ns), 1))(*[L.InferBag(X=x + 0x10000000 * j if x else None, ldx=ldx, N=n) for j, n in enumerate(ns)])


def _ws(cfg, ns, **kw):
    return L.lib().mhimx_infer_dsmil_ws_bytes(C.byref(cfg), len(ns), _bags(ns, **kw))


def _out(**kw):
    o = dict(logits_bag=FAKE, logits_ins=FAKE + 4096, logits=FAKE + 8192)
    o.update(kw)
    return L.InferDsmilOut(**o)


def _run(cfg, ns, bags=None, out=None, x_dtype=0, ws=FAKE + (1 << 33), ws_bytes=1 << 40, labels=None):
    lib = L.lib()
    r = lib.mhimx_infer_dsmil_run(None, C.byref(cfg) if cfg is not None else None, len(ns), _bags(ns) if bags is None else bags, labels,
                                  C.byref(out if out is not None else _out()), ws, ws_bytes, x_dtype)
    return r, lib.mhimx_last_error()


def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in ("mhimx_infer_dsmil_ws_bytes", "mhimx_infer_dsmil_run"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert L.ABI_VERSION == 620 and lib.mhimx_version() == 620
    # the header cites the reference lines the call replaces, as every other entry point does
    for cite in ("modules/mhim.py:229-272", "mhim_modules/baseline.py:112-194", "engines/common_mil.py:56-68"):
        assert cite in hdr[hdr.index("Ragged multi-bag inference for MHIM(DSMIL)"):hdr.index("mhimx_infer_dsmil_run")], cite


def test_ws_bytes_needs_no_device_and_grows_with_rows():
    cfg = _cfg()
    sizes = [_ws(cfg, ns) for ns in ([1], [100], [1000], [1000, 1], [1000, 1000], [1000] * 32, [200000, 50, 60, 70])]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # per row: h 2048 + V 2048 + Q 512 + classes 64 bytes; the images: W1, v.1, q.0, q.2
    images = (512 * 256 + 512 * 512 + 128 * 512 + 128 * 128) * 4
    assert sizes[2] >= 1000 * 4672 + images
    assert sizes[2] - sizes[1] >= 900 * 4672
    assert _ws(cfg, [70, 200000, 60, 50]) == sizes[-1]            # the order of the bags does not change the size
    assert _ws(_cfg(Cc=16), [1000]) > sizes[2]                    # the pool partials are C x 2 KiB per chunk


def test_the_dsmil_row_cap_keeps_the_workspace_under_the_abmil_call_s():
    from mhim_mil_amd.mhim import MHIM
    lib = L.lib()
    for d in (256, 1024, 1536):
        for cc in (2, 3, 16):
            m = MHIM.__new__(MHIM)
            m.__dict__.update(baseline="dsmil", n_classes=cc)
            cap = m.infer_rows_per_call()
            assert MHIM.infer_row_cap * 2 // 5 < cap < MHIM.infer_row_cap // 2          # "about half the rows"
            p = L.StepParams()
            ab = lib.mhimx_infer_ws_bytes(C.byref(L.InferCfg(D=d, E=512, A=128, C=cc, act=2, da_act=1, p=p)), 1,
                                          _bags([MHIM.infer_row_cap], ldx=d))
            for ns in ([cap], [cap // 32] * 32, [cap - 31 * 1] + [1] * 31):
                assert sum(ns) <= cap
                ds = lib.mhimx_infer_dsmil_ws_bytes(C.byref(_cfg(D=d, Cc=cc)), len(ns), _bags(ns, ldx=d))
                assert 0 < ds <= ab, (d, cc, ns[0], ds, ab)
    m = MHIM.__new__(MHIM)
    m.__dict__.update(baseline="dsmil", n_classes=2)
    cap = m.infer_rows_per_call()
    mk = lambda n: types.SimpleNamespace(shape=(n, 256))
    assert m.infer_chunks([mk(5)] * 70) == [(0, 32), (32, 64), (64, 70)]
    ns = [cap - 10, 10, 1, cap + 5, 3, cap, 1]
    assert m.infer_chunks([mk(n) for n in ns]) == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]


@pytest.mark.parametrize("what, cfg_kw, ns, bag_kw, x_dtype, word", [
    ("C = 17", {"Cc": 17}, [10], {}, 0, b"shapes outside"),
    ("C = 0", {"Cc": 0}, [10], {}, 0, b"shapes outside"),
    ("D = 384", {"D": 384}, [10], {"ldx": 384}, 0, b"shapes outside"),
    ("E = 256", {"E": 256}, [10], {}, 0, b"shapes outside"),
    ("N = 0", {}, [10, 0, 10], {}, 0, b"bag 1"),
    ("N < 0", {}, [3, 4, -5], {}, 0, b"bag 2"),
    ("33 bags", {}, [10] * 33, {}, 0, b"bags per call"),
    ("no bags", {}, [], {}, 0, b"bags per call"),
    ("rows of the call above the limit", {}, [L.INFER_MAX_ROWS // 2 + 1] * 2, {}, 0, b"rows in one call"),
    ("pitch below D", {}, [10], {"ldx": 128}, 0, b"bag 0"),
    ("pitch not a multiple of 4 floats", {}, [10], {"ldx": 258}, 0, b"bag 0"),
    ("half pitch not a multiple of 8", {}, [10], {"ldx": 260}, 1, b"bag 0"),
    ("misaligned X", {}, [10, 10], {"x": FAKE + 4}, 0, b"bag 0: null or unaligned"),
    ("null X", {}, [10], {"x": 0}, 0, b"bag 0: null or unaligned"),
    ("bad x_dtype", {}, [10], {}, 3, b"x_dtype 3"),
    ("negative x_dtype", {}, [10], {}, -1, b"x_dtype -1"),
    ("activation code", {"act": 9}, [10], {}, 0, b"activation"),
])
def test_every_refusal_is_an_error_before_any_device_call(what, cfg_kw, ns, bag_kw, x_dtype, word):
    lib = L.lib()
    cfg = _cfg(**cfg_kw)
    bags = _bags(ns, **bag_kw)
    r, msg = _run(cfg, ns, bags=bags, x_dtype=x_dtype)
    assert r < 0 and msg.startswith(b"infer_dsmil:") and word in msg, (what, r, msg)
    shape_only = x_dtype == 0 and "x" not in bag_kw           # mhimx_infer_dsmil_ws_bytes sees neither the element type nor the pointers
    w = lib.mhimx_infer_dsmil_ws_bytes(C.byref(cfg), len(ns), bags)
    if shape_only:
        assert w < 0 and word in lib.mhimx_last_error(), what
    elif what != "half pitch not a multiple of 8":
        assert w > 0, what


def test_run_refusals_without_a_device():
    lib = L.lib()
    cfg, ns = _cfg(), [100, 7]
    need = _ws(cfg, ns)
    for kw, word in [
        (dict(cfg=None), b"null"),
        (dict(cfg=_cfg(params=False)), b"null parameter"),
        (dict(cfg=_cfg(wq2=0)), b"null parameter"),
        (dict(cfg=_cfg(wv=FAKE + 8)), b"16-byte aligned"),
        (dict(out=L.InferDsmilOut(logits=FAKE)), b"outputs are required"),
        (dict(out=_out(loss=FAKE + 12288)), b"needs labels"),
        (dict(ws=None), b"256-byte aligned"),
        (dict(ws=FAKE + 64), b"256-byte aligned"),
        (dict(ws_bytes=need - 1), b"workspace too small"),
    ]:
        args = dict(cfg=cfg, ns=ns, ws_bytes=need)
        args.update(kw)
        r, msg = _run(**args)
        assert r < 0 and word in msg, (kw, r, msg)
    assert lib.mhimx_infer_dsmil_ws_bytes(None, 1, _bags([1])) < 0
    assert lib.mhimx_infer_dsmil_ws_bytes(C.byref(cfg), 1, None) < 0


# ------------------------------------------------------------------------------------------------ MHIM._infer_ok mirrors the C checks
class _FakeBag:
    """Shape-only stand-in for a GPU bag: what _infer_ok reads."""

    def __init__(self, n, d, dtype=torch.float32, ptr=FAKE, pitch=None, dev=torch.device("cpu")):
        self.shape, self.dtype, self.device, self._ptr, self._pitch = (n, d), dtype, dev, ptr, pitch or d

    def dim(self):
        return 2

    def stride(self, k):
        return self._pitch if k == 0 else 1

    def data_ptr(self):
        return self._ptr

    def element_size(self):
        return 4 if self.dtype == torch.float32 else 2


def _model(d=256, cc=2, **kw):
    from mhim_mil_amd.mhim import MHIM
    torch.manual_seed(0)
    return MHIM(baseline="dsmil", n_classes=cc, input_dim=d, merge_enable=False, **kw).eval()


def test_infer_ok_admits_dsmil_and_mirrors_the_c_checks():
    from mhim_mil_amd import ops
    m = _model()
    ok = [_FakeBag(10, 256), _FakeBag(1, 256)]
    assert m._infer_ok(ok)
    assert m._infer_ok([_FakeBag(10, 256, torch.float16, pitch=264)]) and m._infer_ok([_FakeBag(10, 256, torch.bfloat16)])
    # what C refuses, Python routes to the loop (False), it does not raise
    assert not m._infer_ok([_FakeBag(0, 256)])                                   # N = 0
    assert not m._infer_ok([_FakeBag(10, 256, ptr=FAKE + 4)])                    # misaligned X
    assert not m._infer_ok([_FakeBag(10, 256, pitch=258)])                       # pitch rule
    assert not m._infer_ok([_FakeBag(10, 256, torch.float16, pitch=260)])
    assert not m._infer_ok([_FakeBag(10, 256, torch.float64)])                   # bad element type
    assert not m._infer_ok([_FakeBag(10, 256), _FakeBag(10, 256, torch.float16)])
    assert not m._infer_ok([_FakeBag(10, 128)])                                  # D of the bag is not the model's
    assert not _model(d=384)._infer_ok([_FakeBag(10, 384)])                      # D % 256
    assert not _model(mlp_dim=256)._infer_ok(ok)                                 # E != 512
    # the conditions shared with ABMIL
    assert not _model(prec="f32")._infer_ok(ok)
    assert not _model().train()._infer_ok(ok)
    mt = _model()
    mt.merge_test = True
    assert not mt._infer_ok(ok)
    hook, ops.KERNEL_EVENT_HOOK = ops.KERNEL_EVENT_HOOK, (lambda *a: None)
    try:
        assert not m._infer_ok(ok)
    finally:
        ops.KERNEL_EVENT_HOOK = hook
    m16 = _model(cc=16)
    assert m16._infer_ok(ok)
    # a parameter that is not a contiguous fp32 tensor
    md = _model()
    md.online_encoder.b_classifier.q[2].weight.data = md.online_encoder.b_classifier.q[2].weight.data.double()
    assert not md._infer_ok(ok)
    # 17 classes: the module itself refuses (its kernels handle 16), so no model reaches the call with C = 17
    with pytest.raises(L.MhimxError):
        _model(cc=17)


def test_infer_many_no_longer_raises_for_dsmil_on_the_cpu_side():
    """The refusal the parent raised ("DSMIL returns two logit rows per bag") is gone: a CPU bag still fails, but with the shared
    'CUDA tensor' message of every route."""
    m = _model()
    with pytest.raises(L.MhimxError, match="CUDA tensor"):
        m.infer_many([torch.zeros(4, 256)])


# ------------------------------------------------------------------------------------------------ the parity test's data
@pytest.mark.parametrize("cc", DD.CLASSES)
def test_committed_seeds_meet_the_argmax_gap_on_the_oracle_s_data(cc):
    """The condition of tests/test_infer_dsmil_gpu.py::test_oracle_parity, checked where no GPU is needed: in every bag and class with
    N > 1 the two largest classes[:, c] differ by at least 1e-3 of max |classes|; one bag has a critical row in chunk >= 1 and one in a
    last partial 32-row tile."""
    ref = DD.reference(cc)
    DD.assert_gap_and_coverage(ref)
    assert [r["N"] for r in ref] == list(DD.SIZES) and len(ref) == 11
