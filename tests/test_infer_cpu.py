"""Ragged multi-bag inference (mhimx_infer_ws_bytes / mhimx_infer_run, csrc/infer.hip) without a GPU: the entry points exist and are
bound, the workspace size is pure host arithmetic, and every refusal is an error status - raised before any device call, so none of it
needs a device.  Pointers handed over here are made-up addresses: a refused call never touches them."""
import ctypes as C
import re
import os

import pytest

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced


def _cfg(D=1024, E=512, A=128, Cc=2, act=2, da_act=1, params=True):
    p = L.StepParams()
    if params:
        for k, n in enumerate(("w1", "b1", "wa", "wc", "wp", "bp")):
            setattr(p, n, FAKE + 0x1000000 * (k + 1))
    return L.InferCfg(D=D, E=E, A=A, C=Cc, act=act, da_act=da_act, p=p)


def _bags(ns, ldx=1024, x=FAKE + 0x100000000):
    return (L.InferBag * len(ns))(*[L.InferBag(X=x + 0x10000000 * j if x else None, ldx=ldx, N=n) for j, n in enumerate(ns)])


def _ws(cfg, ns, **kw):
    return L.lib().mhimx_infer_ws_bytes(C.byref(cfg), len(ns), _bags(ns, **kw))


def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in ("mhimx_infer_ws_bytes", "mhimx_infer_run"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert int(re.search(r"#define MHIMX_INFER_MAX (\d+)", hdr).group(1)) == L.INFER_MAX >= 32
    assert int(re.search(r"#define MHIMX_INFER_MAX_ROWS (\d+)", hdr).group(1)) == L.INFER_MAX_ROWS
    assert L.ABI_VERSION == 620 and lib.mhimx_version() == 620


def test_ws_bytes_grows_with_rows_and_bags_and_is_aligned():
    cfg = _cfg()
    sizes = [_ws(cfg, ns) for ns in ([1], [100], [1000], [1000, 1], [1000, 1000], [1000] * 32, [200000, 50, 60, 70])]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # the feature rows dominate: 2 KiB per row, plus the two weight images (E*D and A*E floats)
    assert sizes[2] >= 1000 * 512 * 4 + (512 * 1024 + 128 * 512) * 4
    assert sizes[2] - sizes[1] >= 900 * 512 * 4
    # the order of the bags does not change the size
    assert _ws(cfg, [70, 200000, 60, 50]) == sizes[-1]


@pytest.mark.parametrize("what, cfg_kw, ns, bag_kw", [
    ("no bags", {}, [], {}),
    ("too many bags", {}, [10] * 33, {}),
    ("N = 0", {}, [10, 0, 10], {}),
    ("N < 0", {}, [-5], {}),
    ("N above the row limit", {}, [L.INFER_MAX_ROWS + 1], {}),
    ("rows of the call above the limit", {}, [L.INFER_MAX_ROWS // 2 + 1] * 2, {}),
    ("E != 512", {"E": 256}, [10], {}),
    ("A != 128", {"A": 64}, [10], {}),
    ("D % 256", {"D": 1000}, [10], {"ldx": 1000}),
    ("D = 0", {"D": 0}, [10], {}),
    ("C = 0", {"Cc": 0}, [10], {}),
    ("C too large", {"Cc": 17}, [10], {}),
    ("activation code", {"act": 9}, [10], {}),
    ("pitch below D", {}, [10], {"ldx": 512}),
    ("pitch not a multiple of 4 floats", {}, [10], {"ldx": 1026}),
])
def test_shape_refusals_are_errors_in_both_entry_points(what, cfg_kw, ns, bag_kw):
    lib = L.lib()
    cfg = _cfg(**cfg_kw)
    bags = _bags(ns, **bag_kw) if ns else _bags([1])
    assert lib.mhimx_infer_ws_bytes(C.byref(cfg), len(ns), bags) < 0, what
    assert lib.mhimx_last_error().startswith(b"infer:"), what
    out = L.InferOut(logits=FAKE, stats=FAKE + 4096)
    assert lib.mhimx_infer_run(None, C.byref(cfg), len(ns), bags, None, C.byref(out), FAKE + (1 << 33), 1 << 40) < 0, what
    assert lib.mhimx_last_error().startswith(b"infer:"), what


def test_run_refusals_without_a_device():
    lib = L.lib()
    cfg, ns = _cfg(), [100, 7]
    bags = _bags(ns)
    need = lib.mhimx_infer_ws_bytes(C.byref(cfg), 2, bags)
    out = L.InferOut(logits=FAKE, stats=FAKE + 4096)
    ws = FAKE + (1 << 33)

    def run(cfg=cfg, n=2, bags=bags, labels=None, out=out, ws=ws, ws_bytes=need):
        r = lib.mhimx_infer_run(None, C.byref(cfg) if cfg is not None else None, n, bags, labels, C.byref(out) if out is not None else None,
                                ws, ws_bytes)
        return r, lib.mhimx_last_error()

    for kw, word in [
        (dict(cfg=None), b"null"),
        (dict(bags=None), b"null"),
        (dict(cfg=_cfg(params=False)), b"null parameter"),
        (dict(bags=_bags(ns, x=0)), b"null or unaligned"),
        (dict(bags=_bags(ns, x=FAKE + 4)), b"null or unaligned"),
        (dict(out=None), b"outputs are required"),
        (dict(out=L.InferOut(stats=FAKE)), b"outputs are required"),
        (dict(out=L.InferOut(logits=FAKE, stats=FAKE + 4096, loss=FAKE + 8192)), b"needs labels"),
        (dict(ws=None), b"256-byte aligned"),
        (dict(ws=ws + 64), b"256-byte aligned"),
        (dict(ws_bytes=need - 1), b"workspace too small"),
    ]:
        r, msg = run(**kw)
        assert r < 0 and word in msg, (kw, r, msg)
    assert lib.mhimx_infer_ws_bytes(None, 1, bags) < 0
    assert lib.mhimx_infer_ws_bytes(C.byref(cfg), 1, None) < 0


def test_chunking_respects_the_bag_and_row_caps():
    """MHIM.infer_chunks: host arithmetic over the row counts (no device: the bags are shape-only stand-ins)."""
    import types
    from mhim_mil_amd.mhim import MHIM
    m = MHIM.__new__(MHIM)
    cap = MHIM.infer_row_cap
    mk = lambda n: types.SimpleNamespace(shape=(n, 1024))
    assert m.infer_chunks([]) == []
    assert m.infer_chunks([mk(5)] * 70) == [(0, 32), (32, 64), (64, 70)]
    ns = [cap - 10, 10, 1, cap + 5, 3, cap, 1]
    ch = m.infer_chunks([mk(n) for n in ns])
    assert ch == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]
    for lo, hi in ch:
        assert hi - lo <= L.INFER_MAX and (hi - lo == 1 or sum(ns[lo:hi]) <= cap)
