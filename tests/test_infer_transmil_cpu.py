"""Ragged multi-bag TransMIL inference (mhimx_infer_transmil_ws_bytes / _layout_of / _run, csrc/infer_transmil.hip) without a GPU: the
entry points exist and are bound, the ctypes structs have the C compiler's sizes and offsets, workspace size and layout are pure host
arithmetic, every refusal is an error status raised before any device call (pointers handed over here are made-up addresses: a refused
call never touches them), and MHIM._infer_ok mirrors the C checks."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
PARAMS = ("w1", "b1", "cls_token", "w7", "w5", "w3", "b7", "b5", "b3", "norm_w", "norm_b", "wp", "bp")
LAYER = ("ln_w", "ln_b", "w_qkv", "w_out", "b_out", "conv_w")
NEW = ("mhimx_infer_transmil_ws_bytes", "mhimx_infer_transmil_layout_of", "mhimx_infer_transmil_run")


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


def _ws(cfg, ns, **kw):
    return L.lib().mhimx_infer_transmil_ws_bytes(C.byref(cfg), len(ns), _bags(ns, **kw))


def _run(cfg, ns, bags=None, x_dtype=0, ws=FAKE + (1 << 36), ws_bytes=1 << 44, labels=None, logits=FAKE + 4096, loss=None):
    lib = L.lib()
    r = lib.mhimx_infer_transmil_run(None, C.byref(cfg) if cfg is not None else None, len(ns), _bags(ns) if bags is None else bags, labels,
                                     logits, loss, None, ws, ws_bytes, x_dtype)
    return r, lib.mhimx_last_error()


def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhimx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(L.SYMBOLS) and all(hasattr(lib, n) for n in declared)
    assert L.ABI_VERSION == 620 and lib.mhimx_version() == 620
    sec = hdr[hdr.index("Ragged multi-bag inference for MHIM(TransMIL)"):hdr.index("mhimx_infer_transmil_run")]
    for cite in ("modules/mhim.py:229-272", "mhim_modules/baseline.py:196-288", "modules/nystrom_attention.py:12-27,65-152",
                 "modules/emb_position.py:85-120", "engines/common_mil.py:56-68", "engines/base_engine.py:234-329", "96 launches",
                 "MHIMX_VERSION stays 620"):
        assert cite in sec, cite


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_ctypes_structs_match_a_c_compile_of_the_header(tmp_path):
    fields = {"mhimx_transmil_layer": (L.TransmilLayer, LAYER),
              "mhimx_infer_transmil_cfg": (L.InferTransmilCfg, ("D", "C", "act") + PARAMS + ("layer",)),
              "mhimx_infer_transmil_layout": (L.InferTransmilLayout, tuple(n for n, _ in L.InferTransmilLayout._fields_))}
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdint.h>", '#include "mhimx.h"', "int main(void) {"]
    for cname, (_, fs) in fields.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f in fs]
    lines.append("  return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, (ct, fs) in fields.items():
        assert int(got[cname]) == C.sizeof(ct), cname
        for f in fs:
            assert int(got[f"{cname}.{f}"]) == getattr(ct, f).offset, (cname, f)


def _layout(cfg, ns):
    lo = L.InferTransmilLayout()
    assert L.lib().mhimx_infer_transmil_layout_of(C.byref(cfg), len(ns), _bags(ns), C.byref(lo)) == 0
    return lo


def test_layout_is_host_arithmetic_aligned_and_free_of_overlap():
    cfg = _cfg()
    ns = [1, 255, 256, 2100]
    lo = _layout(cfg, ns)
    assert lo.n_bags == 4 and lo.total == _ws(cfg, ns) and lo.total % 256 == 0
    tok = 0
    for b, N in enumerate(ns):
        n = N + 1
        T = 256 * ((n + 255) // 256)
        assert (lo.tok0[b], lo.T[b], lo.pad[b]) == (tok, T, T - n), (b, N)
        tok += T
    assert lo.tokens == tok == 256 + 256 + 512 + 2304
    assert [lo.pad[b] for b in range(4)] == [254, 0, 255, 203]
    nb = len(ns)
    regions = []
    for l in range(2):
        regions += [(lo.x[l], tok * 2048), (lo.qkv[l], tok * 6144), (lo.lm[l], nb * 256 * 4096), (lo.a2[l], nb * 8 * 262144),
                    (lo.z[l], nb * 8 * 262144), (lo.a3v[l], nb * 8 * 65536), (lo.lse3[l], nb * 8 * 1024), (lo.w2[l], nb * 8 * 65536),
                    (lo.out[l], tok * 2048), (lo.y[l], tok * 2048)]
    regions.append((lo.cls, nb * 2048))
    assert all(off % 256 == 0 and off >= 0 for off, _ in regions)
    regions.sort()
    for (a, sa), (b, _) in zip(regions, regions[1:]):
        assert a + sa <= b
    assert regions[-1][0] + regions[-1][1] <= lo.total
    # the size grows with the rows and with the bags, and does not depend on the order of the bags
    sizes = [_ws(cfg, s) for s in ([1], [255], [256], [2100], [2100, 1], [2100] * 32)]
    assert sizes[0] == sizes[1] and sizes == sorted(sizes) and len(set(sizes)) == 5
    assert _ws(cfg, [1, 2100]) == sizes[4]


def test_the_transmil_row_cap_and_chunks():
    from mhim_mil_amd.mhim import MHIM
    m = MHIM.__new__(MHIM)
    m.__dict__.update(baseline="selfattn", n_classes=2)
    cap = m.infer_rows_per_call()
    assert cap * 26 * 1024 <= MHIM.infer_row_cap * 2060 < (cap + 1) * 26 * 1024
    mk = lambda n: types.SimpleNamespace(shape=(n, 256))
    assert m.infer_chunks([mk(5)] * 33) == [(0, 32), (32, 33)]
    assert m.infer_chunks([mk(cap - 10), mk(10), mk(1)]) == [(0, 2), (2, 3)]


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
def test_every_refusal_is_an_error_before_any_device_call(what, cfg_kw, ns, bag_kw, x_dtype, word):
    lib = L.lib()
    cfg = _cfg(**cfg_kw)
    bags = _bags(ns, **bag_kw)
    r, msg = _run(cfg, ns, bags=bags, x_dtype=x_dtype)
    assert r < 0 and msg.startswith(b"infer_transmil:") and word in msg, (what, r, msg)
    if x_dtype == 0 and "x" not in bag_kw:          # the two host-only entry points see neither the element type nor the pointers
        assert lib.mhimx_infer_transmil_ws_bytes(C.byref(cfg), len(ns), bags) < 0 and word in lib.mhimx_last_error(), what
        assert lib.mhimx_infer_transmil_layout_of(C.byref(cfg), len(ns), bags, C.byref(L.InferTransmilLayout())) < 0, what


def test_run_refusals_without_a_device():
    lib = L.lib()
    cfg, ns = _cfg(), [100, 7]
    need = _ws(cfg, ns)
    for kw, word in [
        (dict(cfg=None), b"null"),
        (dict(cfg=_cfg(params=False)), b"null parameter"),
        (dict(cfg=_cfg(wp=0)), b"null parameter"),
        (dict(cfg=_cfg(layer_kw={"conv_w": 0})), b"null parameter"),
        (dict(cfg=_cfg(w1=FAKE + 8)), b"16-byte aligned"),
        (dict(cfg=_cfg(layer_kw={"w_qkv": FAKE + 4})), b"16-byte aligned"),
        (dict(logits=None), b"logits output is required"),
        (dict(loss=FAKE + 8192), b"needs labels"),
        (dict(ws=None), b"256-byte aligned"),
        (dict(ws=FAKE + 64), b"256-byte aligned"),
        (dict(ws_bytes=need - 1), b"workspace too small"),
    ]:
        args = dict(cfg=cfg, ns=ns, ws_bytes=need)
        args.update(kw)
        r, msg = _run(**args)
        assert r < 0 and word in msg, (kw, r, msg)
    assert lib.mhimx_infer_transmil_ws_bytes(None, 1, _bags([1])) < 0
    assert lib.mhimx_infer_transmil_ws_bytes(C.byref(cfg), 1, None) < 0
    assert lib.mhimx_infer_transmil_layout_of(C.byref(cfg), 1, _bags([1]), None) < 0


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
    return MHIM(baseline="selfattn", n_classes=cc, input_dim=d, merge_enable=False, **kw).eval()


def test_infer_ok_admits_transmil_and_mirrors_the_c_checks():
    from mhim_mil_amd import ops
    m = _model()
    ok = [_FakeBag(10, 256), _FakeBag(1, 256)]
    assert m._infer_ok(ok)
    assert m._infer_ok([_FakeBag(10, 256, torch.float16, pitch=264)]) and m._infer_ok([_FakeBag(10, 256, torch.bfloat16)])
    # what C refuses, Python routes to the loop (False), it does not raise
    assert not m._infer_ok([_FakeBag(0, 256)])                                   # N = 0
    assert not m._infer_ok([_FakeBag(10, 256, ptr=0)])                           # null X
    assert not m._infer_ok([_FakeBag(10, 256, ptr=FAKE + 4)])                    # misaligned X
    assert not m._infer_ok([_FakeBag(10, 256, pitch=128)])                       # pitch < D
    assert not m._infer_ok([_FakeBag(10, 256, torch.float16, pitch=260)])        # half pitch % 8
    assert not m._infer_ok([_FakeBag(10, 256, torch.float64)])                   # an element type outside MHIMX_X_*
    assert not m._infer_ok([_FakeBag(10, 256), _FakeBag(10, 256, torch.float16)])
    assert not m._infer_ok([_FakeBag(10, 128)])                                  # D of the bag is not the model's
    assert not _model(d=1000)._infer_ok([_FakeBag(10, 1000)])                    # D % 256
    assert _model(cc=16)._infer_ok(ok)
    m17 = _model(cc=16)
    m17.n_classes = 17
    assert not m17._infer_ok(ok)                                                 # C = 17
    m0 = _model()
    m0.n_classes = 0
    assert not m0._infer_ok(ok)                                                  # C = 0
    # eval mode, no merge_test, not the exact-fp32 mode, no event hook
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
    # parameters: dtype, contiguity, alignment
    md = _model()
    md.online_encoder.layer2.attn.to_qkv.weight.data = md.online_encoder.layer2.attn.to_qkv.weight.data.double()
    assert not md._infer_ok(ok)
    mc = _model()
    mc.online_encoder.layer1.attn.to_out[0].weight.data = mc.online_encoder.layer1.attn.to_out[0].weight.data.t()
    assert not mc._infer_ok(ok)
    ma = _model()
    ma.feature[0].weight.data = torch.zeros(512 * 256 + 1)[1:].view(512, 256)    # 4 bytes off a 16-byte boundary
    assert not ma._infer_ok(ok)
    # the chunking of 33 bags: two calls
    assert m.infer_chunks(ok * 16 + [ok[0]]) == [(0, 32), (32, 33)]


def test_infer_topk_still_refuses_transmil():
    with pytest.raises(L.MhimxError, match="one attention map per layer"):
        _model().infer_topk([torch.zeros(4, 256)], 2)
