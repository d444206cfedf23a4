"""mhimx_topk_many (csrc/topk.hip) on the GPU: the k most / least attended instances of many score vectors of different lengths in one
launch chain, through ops.topk_many and MHIM.infer_topk.  Every comparison of indices and values is exact - this is an ordering, not
arithmetic; the CPU yardstick is oracle.mhim_oracle.topk_indices (value descending / ascending, then index ascending).  Inputs are
seeded and hold neither NaN nor -0.0.  The small / large threshold of the call is 16 384 rows: the edge table has 16 383, 16 384, 16 385."""
import functools

import numpy as np
import pytest
import torch

from mhim_mil_amd import _lib as L
from mhim_mil_amd import synth
from oracle import mhim_oracle as O
from tests import test_infer_dsmil_gpu as DS
from tests.test_infer_gpu import _bag, _state
from tests.test_mhim_gpu import V2, build

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 2, 63, 64, 65, 700, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 40000)
KS = (1, 7, 64, 1000, 4096)


def _ops():
    from mhim_mil_amd import ops
    return ops


def _offsets(sizes):
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    return off


@functools.lru_cache(maxsize=None)
def _scores(kind, total=sum(SIZES)):
    """One seeded fp32 vector per kind (computed once, never modified): no NaN, no -0.0."""
    rng = np.random.default_rng({"cont": 1, "q8": 2, "equal": 3}[kind])
    if kind == "cont":
        v = rng.standard_normal(total).astype(np.float32) + np.float32(0.0)
    elif kind == "q8":
        v = (np.floor(rng.random(total) * 8) / 8 - 0.5).astype(np.float32) + np.float32(0.0)      # 8 levels, both signs and 0
    else:
        v = np.full(total, 0.25, np.float32)
    assert not np.isnan(v).any() and not (np.signbit(v) & (v == 0)).any()
    v.setflags(write=False)
    return v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(score, segs, k, largest, idx, val):
    """idx / val [n, k] of a call against the oracle on the numpy vector ``score``."""
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert idx.shape == val.shape == (len(segs), k) and idx.dtype == np.int64 and val.dtype == np.float32
    for b, (r0, n) in enumerate(segs):
        v, kb = score[r0:r0 + n], min(k, n)
        want = O.topk_indices(v, kb, largest)
        assert np.array_equal(idx[b, :kb], want), (b, n, k, largest)
        assert np.array_equal(_bits(val[b, :kb]), _bits(v[want])), (b, n, k, largest)
        assert (idx[b, kb:] == -1).all() and (_bits(val[b, kb:]) == 0).all(), (b, n, k)
        assert idx[b, :kb].min() >= 0 and idx[b, :kb].max() < n and len(set(idx[b, :kb].tolist())) == kb, (b, n, k)


def _run(score, offsets, k, largest, **kw):
    ops = _ops()
    idx, val = ops.topk_many(torch.from_numpy(np.array(score)).to(DEV), offsets, k, largest, **kw)
    torch.cuda.synchronize()
    return idx, val


# ------------------------------------------------------------------------------------------------ 1. edges of every path in one call
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", KS)
def test_edges_of_every_path_in_one_call(k, largest):
    off = _offsets(SIZES)
    assert any(o % 4 for o in off)                                          # (the offsets follow: unaligned segments)
    idx, val = _run(_scores("cont"), off, k, largest)
    _check(_scores("cont"), _ops().topk_segs(off), k, largest, idx, val)


# ------------------------------------------------------------------------------------------------ 2. ties
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", KS)
def test_ties_eight_levels(k, largest):
    off = _offsets(SIZES)
    idx, val = _run(_scores("q8"), off, k, largest)
    _check(_scores("q8"), _ops().topk_segs(off), k, largest, idx, val)


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", [7, 1000, 4096])
def test_ties_all_equal(k, largest):
    off = _offsets(SIZES)
    idx, val = _run(_scores("equal"), off, k, largest)
    _check(_scores("equal"), _ops().topk_segs(off), k, largest, idx, val)
    idx = idx.cpu().numpy()
    for b, n in enumerate(SIZES):
        kb = min(k, n)
        assert np.array_equal(idx[b, :kb], np.arange(kb)), (b, n, k)


@pytest.mark.parametrize("largest", [True, False])
def test_tie_across_the_cut(largest):
    """The k-th and (k+1)-th values are equal, all others distinct: the lower index is taken."""
    k, sizes = 64, (3000, 20000)
    rng = np.random.default_rng(9)
    parts = []
    for n in sizes:
        v = (rng.permutation(n).astype(np.float32) - n // 2) / 8                              # distinct, both signs
        order = np.argsort(-v if largest else v, kind="stable")
        a, b = int(order[k - 1]), int(order[k])
        v[b] = v[a]
        parts.append(v + np.float32(0.0))
        assert len(np.unique(parts[-1])) == n - 1
    score, off = np.concatenate(parts), _offsets(sizes)
    idx, val = _run(score, off, k, largest)
    _check(score, _ops().topk_segs(off), k, largest, idx, val)
    for b, n in enumerate(sizes):
        v = score[off[b]:off[b + 1]]
        tied = np.flatnonzero(v == v[int(idx[b, k - 1])])
        assert len(tied) == 2 and int(idx[b, k - 1]) == tied.min()


# ------------------------------------------------------------------------------------------------ 3. the existing device route agrees
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("kind", ["cont", "q8"])
def test_select_mask_gives_the_same_list(kind, largest):
    ops, k = _ops(), 1000
    off = _offsets(SIZES)
    score = torch.from_numpy(np.array(_scores(kind))).to(DEV)
    idx, _ = ops.topk_many(score, off, k, largest)
    for n in (63, 700, 4097, 16384, 16385, 40000):
        b = SIZES.index(n)
        kb = min(k, n)
        ref = ops.select_mask(score[off[b]:off[b + 1]].clone(), kb, kb, largest, None, want_topk=True)[2]
        assert torch.equal(ref.reshape(-1), idx[b, :kb]), (kind, largest, n)


# ------------------------------------------------------------------------------------------------ 4. 32 segments, gaps, any order
@pytest.mark.parametrize("largest", [True, False])
def test_32_segments(largest):
    sizes = [300 + 37 * j for j in range(32)]
    off = _offsets(sizes)
    score = _scores("cont")[:off[-1]]
    idx, val = _run(score, off, 333, largest)
    _check(score, _ops().topk_segs(off), 333, largest, idx, val)
    with pytest.raises(L.MhimxError, match="33 segments"):
        _ops().topk_many(torch.zeros(40, device=DEV), list(range(34)), 3)


@pytest.mark.parametrize("largest", [True, False])
def test_pairs_with_gaps_in_any_order(largest):
    """(row0, N) pairs, not ascending, with gaps; the unused entries hold the value that would win every ranking."""
    segs = [(50001, 700), (3, 17000), (30011, 1), (20000, 4097), (48000, 2000), (17003, 65)]
    score = np.full(50001 + 700 + 5, np.inf if largest else -np.inf, np.float32)
    rng = np.random.default_rng(4)
    for r0, n in segs:
        score[r0:r0 + n] = rng.standard_normal(n).astype(np.float32) + np.float32(0.0)
    for k in (5, 2500):
        idx, val = _run(score, segs, k, largest)
        assert torch.isfinite(val).all()
        _check(score, segs, k, largest, idx, val)
    with pytest.raises(L.MhimxError, match="behind the score vector"):
        _ops().topk_many(torch.zeros(40, device=DEV), [(30, 11)], 3)


# ------------------------------------------------------------------------------------------------ 5. neighbours and workspace
@pytest.mark.parametrize("n", [700, 16385])
def test_a_segment_does_not_depend_on_its_neighbours(n):
    """Alone, first of 32 and last of 32, each time with a workspace of 0xFF bytes and pre-filled outputs: the segment's rows are the same
    bits, and every output element of every call was written."""
    ops, k = _ops(), 300
    vec = lambda m, seed: np.random.default_rng(seed).standard_normal(m).astype(np.float32) + np.float32(0.0)
    mine = vec(n, 77)
    others = [vec(int(m), 100 + j) for j, m in enumerate(np.random.default_rng(n).integers(64, 2001, size=31))]
    got = []
    for parts, b in (([mine], 0), ([mine] + others, 0), (others + [mine], 31)):
        off = _offsets([len(p) for p in parts])
        score = torch.from_numpy(np.concatenate(parts)).to(DEV)
        segs = ops.topk_segs(off)
        ws = torch.full((ops.topk_many_ws_bytes(segs, k),), 255, dtype=torch.uint8, device=DEV)
        idx = torch.full((len(segs), k), -7, dtype=torch.int64, device=DEV)
        val = torch.full((len(segs), k), float("nan"), device=DEV)
        tab = (L.TopkSeg * len(segs))(*[L.TopkSeg(row0=r, N=m) for r, m in segs])
        L.check(L.lib().mhimx_topk_many(ops._stream(), ops._p(score), len(segs), tab, k, 1, ops._p(idx), ops._p(val), ops._p(ws), ws.numel()),
                "mhimx_topk_many")
        torch.cuda.synchronize()
        assert not (idx == -7).any() and not torch.isnan(val).any(), len(parts)
        _check(np.concatenate(parts), segs, k, True, idx, val)
        got.append((idx[b].clone(), val[b].clone()))
    for i, v in got[1:]:
        assert torch.equal(i, got[0][0]) and torch.equal(v.view(torch.int32), got[0][1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6. determinism and capture
def test_determinism_and_graph_replay():
    ops, k = _ops(), 500
    off = _offsets(SIZES)
    score = torch.from_numpy(np.array(_scores("q8"))).to(DEV)
    a = ops.topk_many(score, off, k, True)
    b = ops.topk_many(score, off, k, True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ws = torch.full((ops.topk_many_ws_bytes(ops.topk_segs(off), k),), 255, dtype=torch.uint8, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        idx, val = ops.topk_many(score, off, k, True, ws=ws)
    for _ in range(2):
        idx.fill_(-7)
        val.fill_(float("nan"))
        ws.fill_(255)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, a[0]) and torch.equal(val, a[1])


# ------------------------------------------------------------------------------------------------ 7 - 9. MHIM.infer_topk
def _check_model(m, xs, k, native, calls=None, **kw):
    """infer_topk against the oracle's top-k of the vectors the model's own infer_many(return_attn=True) returns."""
    labels = torch.arange(len(xs), device=DEV) % 2
    step0 = m._step
    ref_logits, attns, ref_loss = m.infer_many(xs, labels=labels, return_attn=True, no_norm=kw.get("no_norm", False))
    last_ref, step_ref = dict(m.last), m._step - step0
    logits, idx, val, loss = m.infer_topk(xs, k, labels=labels, **kw)
    torch.cuda.synchronize()
    assert m._step - step0 == 2 * step_ref
    assert torch.equal(logits, ref_logits) and torch.equal(loss, ref_loss)
    assert m.last["infer_native"] is native and m.last["infer_calls"] == last_ref["infer_calls"]
    if calls is not None:
        assert m.last["infer_calls"] == calls
    assert set(m.last) == set(last_ref) | {"infer_topk"} and m.last["infer_topk"][0] is idx and m.last["infer_topk"][1] is val
    if "infer_parts" in last_ref:
        for a, b in zip(m.last["infer_parts"], last_ref["infer_parts"]):
            assert (a is None and b is None) or torch.equal(a, b)
    score = np.concatenate([a.cpu().numpy() for a in attns])
    assert not np.isnan(score).any() and not (np.signbit(score) & (score == 0)).any()
    segs = _ops().topk_segs(_offsets([int(a.numel()) for a in attns]))
    assert [n for _, n in segs] == [int(x.shape[-2]) for x in xs]
    _check(score, segs, k, kw.get("largest", True), idx, val)
    return idx, val


def test_infer_topk_native_abmil():
    d = 256
    m = build(_state(5, d, merge_k=5), "auto", input_dim=d, **V2).eval()
    rng = np.random.default_rng(12)
    sizes = [1, 3000, 49, 50, 51] + [int(v) for v in rng.integers(1, 3001, size=35)]
    xs = [_bag(400 + j, n, d) for j, n in enumerate(sizes)]
    idx, _ = _check_model(m, xs, 50, True, calls=2)
    _check_model(m, xs, 50, True, calls=2, no_norm=True, largest=False)
    half = [x.half() for x in xs]
    idx_h = m.infer_topk(half, 50)[1]
    idx_w = m.infer_topk([x.float() for x in half], 50)[1]
    assert m.last["infer_native"] and torch.equal(idx_h, idx_w)
    assert m.infer_topk([], 50)[1].shape == (0, 50)


def test_infer_topk_native_dsmil():
    cc = 2
    sseed, bseed = DS.SEEDS[cc]
    m = DS.build(DS.state(sseed, cc), cc)
    rng = np.random.default_rng(13)
    sizes = list(DS.SIZES) + [int(v) for v in rng.integers(1, 2001, size=29)]
    xs = DS._dev(DS.bags_np(bseed, sizes=tuple(sizes)))
    _check_model(m, xs, 50, True, calls=2)
    _check_model(m, xs, 50, True, calls=2, no_norm=True, largest=False)


def test_infer_topk_fallback_and_refusals():
    d = 256
    g = build(synth.mhim_state(3, input_dim=d, merge_k=5, gated=True), "auto", input_dim=d, gated=True, **V2).eval()
    xs = [_bag(500 + j, n, d) for j, n in enumerate([1, 40, 700, 33] + [60 + j for j in range(31)])]          # 35 bags: two packed calls
    _check_model(g, xs, 50, False)
    mt = build(synth.mhim_state(3, input_dim=d, merge_k=5), "auto", input_dim=d, merge_test=True, **V2).eval()
    step0 = mt._step
    with pytest.raises(L.MhimxError, match="merge_test"):
        mt.infer_topk(xs[:3], 5)
    assert mt._step == step0
    from mhim_mil_amd.mhim import MHIM
    sa = MHIM(baseline="selfattn", n_classes=2, input_dim=d, merge_enable=False).to(DEV).eval()
    with pytest.raises(L.MhimxError, match="TransMIL"):
        sa.infer_topk(xs[:3], 5)
    with pytest.raises(L.MhimxError, match="k=4097"):
        g.infer_topk(xs[:3], 4097)
