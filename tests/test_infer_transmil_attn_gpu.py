"""TransMIL attention maps and instance scores from the ragged call (mhimx_infer_transmil_run_attn, csrc/infer_transmil.hip) on the GPU: the
cls token's attention row of both layers and the teacher's pseudo-score for bags of different row counts in one C call, against the plain
call (logits, loss, z: same bits), the single-bag kernels stage by stage through the workspace layout, the CPU oracle
(oracle.mhim_oracle.sattention / pseudo_score_trans per bag), the module's own forward_test loop, and MHIM.infer_cls_attn / infer_cls_topk.

Tolerances: maps against the oracle atol 1e-6, rtol 2e-3 - the bound tests/test_nystrom_gpu.py::test_g8_sattention holds forward_test's
maps to; pseudo-score atol 5e-6, rtol 2e-3 - that file's bound for the teacher's score (test_g9_transmil_teacher); call against loop twice
those (each side is within one of them); u against an fp64 evaluation of the call's own operands 1e-4 of the scale (close() of
tests/test_infer_transmil_gpu.py, its bound for products); the bag-batched cls-row kernel bit for bit against the single-bag kernel.

Bag sizes: those of tests/test_infer_transmil_gpu.py (one row; either side of the PPEG 7 x 7 rule; pad 1, 0 and 255; l = 3; past 32 chunks)
plus one bag of 4200 rows: T = 4352 tokens = 68 tiles of 64, past the cls-row kernel's cap of 64 chunks."""
import functools

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O
from tests.test_infer_transmil_gpu import D, DEV, KW, SEEDS, _dev, bags_np, build, close, state

pytestmark = pytest.mark.gpu
SIZES = (1, 36, 37, 254, 255, 256, 600, 2100, 4200)
MAP_TOL = dict(atol=1e-6, rtol=2e-3)
SCORE_TOL = dict(atol=5e-6, rtol=2e-3)
CC = 2


# ------------------------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def reference():
    """The oracle's maps [2, 8, N_b] and pseudo-scores [N_b] of the nine bags: computed once, shared, never modified."""
    sseed, bseed = SEEDS[CC]
    po = O.as_torch(state(sseed, CC))
    maps, scores = [], []
    with torch.no_grad():
        for x in bags_np(bseed, sizes=SIZES):
            h = O.feature(torch.from_numpy(x), po, KW["act"])
            _, attn, v = O.sattention(h, po, return_attn=True)
            maps.append(torch.stack(attn).numpy())
            scores.append(O.pseudo_score_trans(v, attn[0], po).numpy())
    return maps, scores


@functools.lru_cache(maxsize=None)
def model(cc=CC):
    return build(state(SEEDS[cc][0], cc), cc)


@functools.lru_cache(maxsize=None)
def bags(cc=CC):
    return tuple(_dev(bags_np(SEEDS[cc][1], sizes=SIZES)))


def _ops():
    from mhim_mil_amd import ops
    return ops


def call(m, xs, **kw):
    kw.setdefault("want_pscore", True)
    return _ops().infer_transmil_many(m._infer_transmil_cfg(), list(xs), want_attn=True, **kw)


@functools.lru_cache(maxsize=None)
def base_call():
    """One call over the nine bags (maps and pseudo-score), shared by the tests that only read it."""
    r = call(model(), bags(), labels=torch.tensor([(3 * j + 1) % CC for j in range(len(SIZES))], device=DEV), want_z=True)
    torch.cuda.synchronize()
    return r


def seg(r, j):
    return r.attn[:, :, r.offsets[j]:r.offsets[j + 1]], r.pscore[r.offsets[j]:r.offsets[j + 1]]


# ------------------------------------------------------------------------------------------------ 2. stage by stage (runs first)
@torch.no_grad()
def test_stages_match_the_single_bag_kernel_through_the_layout():
    """One call on a NaN-poisoned workspace into NaN-poisoned outputs with guard floats behind them: u of every bag, layer and head against
    fp64 on the call's own qkv / lm / z; the packed maps bit for bit mhimx_nys_cls_attn fed with the call's own qkv, lm, lse3 and u of that
    bag, columns pad + 1 ..; every entry written, the guards untouched."""
    ops = _ops()
    m, xs = model(), list(bags())
    cfg = m._infer_transmil_cfg()
    nb, R = len(xs), sum(SIZES)
    ws = torch.full((int(ops.infer_transmil_attn_ws_bytes(cfg, xs, True)),), 255, dtype=torch.uint8, device=DEV)
    abuf = torch.full((16 * R + 64,), float("nan"), device=DEV)
    pbuf = torch.full((R + 64,), float("nan"), device=DEV)
    r = ops.infer_transmil_many(cfg, xs, ws=ws, want_attn=True, want_pscore=True, attn=abuf[:16 * R], pscore=pbuf[:R])
    torch.cuda.synchronize()
    assert torch.isnan(abuf[16 * R:]).all() and torch.isnan(pbuf[R:]).all(), "guards"
    assert not torch.isnan(abuf[:16 * R]).any() and not torch.isnan(pbuf[:R]).any(), "every entry is written"
    assert r.attn.data_ptr() == abuf.data_ptr() and r.pscore.data_ptr() == pbuf.data_ptr() and r.attn.shape == (2, 8, R)
    lo, tok = r.layout, int(r.layout.tokens)
    assert int(lo.total) == ops.infer_transmil_ws_bytes(cfg, xs)                  # the plain layout is the prefix: u sits behind it
    scale = m.online_encoder.layer1.attn.scale
    for l in range(2):
        QKV, LM = r.view("qkv", (tok, 1536), l), r.view("lm", (nb, 256, 1024), l)
        Z, LSE3 = r.view("z", (nb, 8, 256, 256), l), r.view("lse3", (nb, 8, 256), l)
        U = ops.ws_view(ws, int(lo.total) + l * nb * 8 * 256 * 4, nb * 8 * 256).view(nb, 8, 256)
        for b, N in enumerate(SIZES):
            t0, T, pad = int(lo.tok0[b]), int(lo.T[b]), int(lo.pad[b])
            what = f"layer {l} bag {b} (N = {N})"
            qkv = QKV[t0:t0 + T]
            q = qkv[pad, :512].double().view(8, 1, 64)
            kl = LM[b][:, 512:].double().view(256, 8, 64).permute(1, 2, 0)            # [8, 64, 256]
            a1c = torch.softmax(scale * (q @ kl), -1)                                 # [8, 1, 256]
            close(U[b], (a1c @ Z[b].double()).view(8, 256), 1e-4, what + " u")
            ref = ops.nys_cls_attn(ops.NysOperands(qkv, LM[b].contiguous(), scale), LSE3[b].contiguous(), U[b].contiguous())
            got = r.attn[l][:, r.offsets[b]:r.offsets[b + 1]]
            assert got.shape == (8, N) and torch.equal(got, ref[:, pad + 1:]), what + " cls row"


# ------------------------------------------------------------------------------------------------ 1. the plain call's outputs
def test_logits_loss_and_z_are_the_plain_call_s_bits():
    ops = _ops()
    m, xs = model(), list(bags())
    labels = torch.tensor([(3 * j + 1) % CC for j in range(len(SIZES))], device=DEV)
    plain = ops.infer_transmil_many(m._infer_transmil_cfg(), xs, labels=labels, want_z=True)
    r = base_call()
    assert torch.equal(r.logits, plain.logits) and torch.equal(r.loss, plain.loss) and torch.equal(r.z, plain.z)
    only_maps = call(m, xs, labels=labels, want_z=True, want_pscore=False)
    assert only_maps.pscore is None and torch.equal(only_maps.attn, r.attn) and torch.equal(only_maps.logits, plain.logits)


# ------------------------------------------------------------------------------------------------ 3. against the oracle
def test_maps_and_pseudo_score_match_the_oracle():
    r = base_call()
    maps, scores = reference()
    for j, N in enumerate(SIZES):
        a, p = seg(r, j)
        a, p = a.cpu().numpy(), p.cpu().numpy()
        print(f"N = {N}: max |map - oracle| {np.abs(a - maps[j]).max():.3e} (max {np.abs(maps[j]).max():.3e}), "
              f"max |score - oracle| {np.abs(p - scores[j]).max():.3e}")
        np.testing.assert_allclose(a, maps[j], err_msg=f"maps of bag {j} (N = {N})", **MAP_TOL)
        np.testing.assert_allclose(p, scores[j], err_msg=f"pseudo-score of bag {j} (N = {N})", **SCORE_TOL)


# ------------------------------------------------------------------------------------------------ 4. against the loop of the same build
def loop(m, x, pseudo=True):
    """forward_test(return_attn=True) + _trans_score of one bag: the route to the same outputs before the call had its tail."""
    from mhim_mil_amd import nystrom as NY
    lg, (attn, v) = m.forward_test(x, return_attn=True, return_act=True)
    N = x.shape[0]
    a = torch.stack([t[0][:, :N] for t in attn])
    p = m._trans_score(v[0].permute(1, 0, 2).reshape(v.shape[2], NY.INNER)[:N], attn[0][0][:, :N]).reshape(-1) if pseudo else None
    return lg.reshape(-1), a, p


def test_call_matches_the_forward_test_loop_and_its_seed_stream():
    m, xs = model(), list(bags())
    m2 = build(state(SEEDS[CC][0], CC), CC)
    m._step = 17
    logits, attn, ps = m.infer_cls_attn(xs, pseudo=True)
    assert m.last["infer_native"] is True and m.last["infer_calls"] == 1 and m._step == 17 + 3 * len(xs)
    packed, pp, offs = m.last["infer_attn"]
    assert offs == [0] + list(np.cumsum(SIZES)) and packed.shape == (2, 8, sum(SIZES)) and pp.shape == (sum(SIZES),)
    for j, (x, N) in enumerate(zip(xs, SIZES)):
        lg, a, p = loop(m2, x)
        assert attn[j].shape == (2, 8, N) and ps[j].shape == (N,)
        print(f"N = {N}: max |map - loop| {(attn[j] - a).abs().max().item():.3e}, max |score - loop| {(ps[j] - p).abs().max().item():.3e}")
        np.testing.assert_allclose(attn[j].cpu().numpy(), a.cpu().numpy(), atol=2 * MAP_TOL["atol"], rtol=2 * MAP_TOL["rtol"], err_msg=f"bag {j}")
        np.testing.assert_allclose(ps[j].cpu().numpy(), p.cpu().numpy(), atol=2 * SCORE_TOL["atol"], rtol=2 * SCORE_TOL["rtol"], err_msg=f"bag {j}")
        assert (logits[j] - lg).abs().max().item() <= 2e-4


# ------------------------------------------------------------------------------------------------ 5. / 6. neighbours, two runs
def test_a_bag_s_bits_do_not_depend_on_its_place_or_its_neighbours_and_two_runs_agree():
    m, xs = model(), list(bags())
    base = base_call()
    again = call(m, xs)
    assert torch.equal(again.attn, base.attn) and torch.equal(again.pscore, base.pscore) and torch.equal(again.logits, base.logits)
    rev = call(m, xs[::-1])
    n = len(xs)
    for j in range(n):                                               # first <-> last, and every bag at another place
        for got, want in zip(seg(rev, n - 1 - j), seg(base, j)):
            assert torch.equal(got, want), ("reversed", j)
    for j in (0, 3, 8):                                              # alone (one row alone: fewer than 17 rows in the call)
        alone = call(m, [xs[j]])
        for got, want in zip(seg(alone, 0), seg(base, j)):
            assert torch.equal(got, want), ("alone", j)
        assert torch.equal(alone.logits[0], base.logits[j])
    other = call(m, [xs[5], xs[0], xs[8], xs[2]])                    # other neighbours
    for k, j in enumerate((5, 0, 8, 2)):
        for got, want in zip(seg(other, k), seg(base, j)):
            assert torch.equal(got, want), ("neighbours", j)


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_a_captured_call_replays_the_eager_bits_on_new_contents():
    m = model()
    sizes = (300, 37, 1, 600)
    xs = _dev(bags_np(900, sizes=sizes))
    labels = torch.tensor([1, 0, 1, 1], device=DEV)
    call(m, xs, labels=labels)                                       # (the first call on the device: outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # one stream, no parallel branches
        r = call(m, xs, labels=labels)
    for x, new in zip(xs, bags_np(950, sizes=sizes)):                # new bag contents in the same buffers
        x.copy_(torch.from_numpy(new))
    eager = call(m, xs, labels=labels)
    want = [t.clone() for t in (eager.logits, eager.loss, eager.attn, eager.pscore)]
    for _ in range(2):
        for t in (r.logits, r.loss, r.attn, r.pscore):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((r.logits, r.loss, r.attn, r.pscore), want))


# ------------------------------------------------------------------------------------------------ 8. half-precision bags
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_bags_give_the_bits_of_the_widened_call(dtype):
    m = model()
    xs = [x.to(dtype) for x in _dev(bags_np(1300, sizes=(1, 37, 255, 300)))]
    lg, attn, ps = m.infer_cls_attn(xs, pseudo=True)
    assert m.last["infer_native"] is True
    packed, pp, _ = m.last["infer_attn"]
    lg2, _, _ = m.infer_cls_attn([x.float() for x in xs], pseudo=True)
    wide, wp, _ = m.last["infer_attn"]
    assert torch.equal(lg, lg2) and torch.equal(packed, wide) and torch.equal(pp, wp)


# ------------------------------------------------------------------------------------------------ 9. top-k
def rank(v, k, largest):
    """idx, val [k] of one vector under the tie contract: value, then lowest index; -1 / 0 behind min(k, N)."""
    v = np.asarray(v)
    order = np.lexsort((np.arange(v.size), -v if largest else v))[:k]
    idx, val = np.full(k, -1, np.int64), np.zeros(k, np.float32)
    idx[:order.size], val[:order.size] = order, v[order]
    return idx, val


@pytest.mark.parametrize("largest", [True, False])
def test_infer_cls_topk_equals_a_cpu_ranking_of_the_returned_vectors(largest):
    m = model()
    sizes = (1, 36, 300, 97)
    raw = bags_np(1600, sizes=sizes)
    raw[1][5] = raw[1][2]                                            # three equal rows: equal layer-1 maps and pseudo-scores (a tie)
    raw[1][30] = raw[1][2]
    xs = _dev(raw)
    k = 40                                                           # > N of the first two bags: padding, and every row of them is ranked
    _, attn, ps = m.infer_cls_attn(xs, pseudo=True)
    assert ps[1][5].item() == ps[1][2].item() == ps[1][30].item() and torch.equal(attn[1][0][:, 5], attn[1][0][:, 2])
    s0 = m._step
    lg, idx, val = m.infer_cls_topk(xs, k, largest=largest)
    assert m._step == s0 + 3 * len(xs) and m.last["infer_native"] is True and m.last["infer_topk"][0] is idx
    assert idx.shape == (4, k) and val.shape == (4, k) and idx.dtype == torch.int64
    for j in range(4):
        ri, rv = rank(ps[j].cpu().numpy(), k, largest)
        assert np.array_equal(idx[j].cpu().numpy(), ri) and np.array_equal(val[j].cpu().numpy(), rv), ("pseudo", j)
    pos = {int(i): p for p, i in enumerate(idx[1].tolist())}
    assert pos[2] + 1 == pos[5] and pos[5] + 1 == pos[30]            # the tie: neighbours in the ranking, lowest index first
    assert idx[1, 36:].eq(-1).all() and val[1, 36:].eq(0).all() and idx[0, 0] == 0 and idx[0, 1:].eq(-1).all()
    for layer in (0, 1):
        lg, idx, val = m.infer_cls_topk(xs, k, largest=largest, by="heads", layer=layer)
        assert idx.shape == (4, 8, k) and val.shape == (4, 8, k)
        for j in range(4):
            for h in range(8):
                ri, rv = rank(attn[j][layer, h].cpu().numpy(), k, largest)
                assert np.array_equal(idx[j, h].cpu().numpy(), ri) and np.array_equal(val[j, h].cpu().numpy(), rv), ("heads", layer, j, h)


# ------------------------------------------------------------------------------------------------ 10. fallbacks
@pytest.mark.parametrize("kind", ["train", "merge_test", "f32"])
def test_what_the_call_refuses_returns_the_loop_s_values_in_the_same_shapes(kind):
    sizes = (40, 300)
    xs = _dev(bags_np(1400, sizes=sizes))
    if kind == "merge_test":
        sd = synth.mhim_state(SEEDS[CC][0], input_dim=D, n_classes=CC, baseline="selfattn", merge_k=5)
        mm = build(sd, CC, merge_enable=True, merge_k=5, merge_test=True)
        mm.merge.dropout = 0.0
    elif kind == "train":
        mm = build(state(SEEDS[CC][0], CC), CC).train()
    else:
        mm = build(state(SEEDS[CC][0], CC), CC, prec="f32")
    s0 = mm._step
    lg, attn, ps = mm.infer_cls_attn(xs, pseudo=True)
    assert mm.last["infer_native"] is False and mm.last["infer_calls"] == 0 and mm._step == s0 + 3 * len(xs)
    packed, pp, offs = mm.last["infer_attn"]
    assert offs == [0, 40, 340] and packed.shape == (2, 8, 340) and pp.shape == (340,)
    mm._step = s0
    for j, (x, N) in enumerate(zip(xs, sizes)):
        s1 = mm._step
        l, a, p = loop(mm, x)
        mm._step = s1 + 3
        assert attn[j].shape == (2, 8, N) and ps[j].shape == (N,)
        assert torch.equal(lg[j], l) and torch.equal(attn[j], a) and torch.equal(ps[j], p), (kind, j)
    _, idx, val = mm.infer_cls_topk(xs, 3)
    assert idx.shape == (2, 3) and mm.last["infer_native"] is False


# ------------------------------------------------------------------------------------------------ 11. more bags than one call takes
@pytest.mark.parametrize("route", ["native", "loop"])
def test_more_bags_than_one_call_takes_on_both_routes(route):
    """33 bags of 1 / 255 / 256 / 300 rows - one more than L.INFER_MAX - through infer_cls_attn(pseudo=True) and infer_cls_topk(k=4,
    by="pseudo"): two native calls (on the merge_test model: the forward_test loop, no call), ``_step`` moves by 99, the packed
    ``infer_attn`` (infer_cls_attn's entry; infer_cls_topk leaves ``infer_topk`` [33, 4]) covers all 33 bags, and every per-bag view
    equals bit for bit what the same method returns for that bag alone.  The loop route is also held to ``loop()`` of each bag bit for
    bit, the bound of test_what_the_call_refuses_returns_the_loop_s_values_in_the_same_shapes (the merge_test model scores N + 5 tokens:
    it is another function than the plain model's, so the two models' values are not compared)."""
    native = route == "native"
    sizes = tuple((1, 255, 256, 300)[j % 4] for j in range(33))
    xs = _dev(bags_np(1700, sizes=sizes))
    if native:
        mm = model()
    else:
        sd = synth.mhim_state(SEEDS[CC][0], input_dim=D, n_classes=CC, baseline="selfattn", merge_k=5)
        mm = build(sd, CC, merge_enable=True, merge_k=5, merge_test=True)
        mm.merge.dropout = 0.0
    s0 = mm._step = 50
    lg, attn, ps = mm.infer_cls_attn(xs, pseudo=True)
    assert mm.last["infer_native"] is native and mm.last["infer_calls"] == (2 if native else 0) and mm._step == s0 + 99
    packed, pp, offs = mm.last["infer_attn"]
    assert len(offs) == 34 and offs == [0] + list(np.cumsum(sizes)) and packed.shape == (2, 8, offs[-1]) and pp.shape == (offs[-1],)
    assert lg.shape == (33, CC) and len(attn) == len(ps) == 33
    mm._step = s0
    tlg, idx, val = mm.infer_cls_topk(xs, 4, by="pseudo")
    assert mm.last["infer_native"] is native and mm.last["infer_calls"] == (2 if native else 0) and mm._step == s0 + 99
    assert idx.shape == (33, 4) and val.shape == (33, 4) and mm.last["infer_topk"][0] is idx and torch.equal(tlg, lg)
    for j, (x, N) in enumerate(zip(xs, sizes)):
        mm._step = s0 + 3 * j                                        # (the stream position the bag had in the list)
        l1, a1, p1 = mm.infer_cls_attn([x], pseudo=True)
        assert mm.last["infer_native"] is native and mm._step == s0 + 3 * j + 3
        assert attn[j].shape == (2, 8, N) and ps[j].shape == (N,)
        assert torch.equal(lg[j], l1[0]) and torch.equal(attn[j], a1[0]) and torch.equal(ps[j], p1[0]), (route, j)
        assert torch.equal(packed[:, :, offs[j]:offs[j + 1]], a1[0]) and torch.equal(pp[offs[j]:offs[j + 1]], p1[0]), (route, j)
        mm._step = s0 + 3 * j
        _, i1, v1 = mm.infer_cls_topk([x], 4, by="pseudo")
        assert torch.equal(idx[j], i1[0]) and torch.equal(val[j], v1[0]), (route, j)
        if not native:
            mm._step = s0 + 3 * j
            l, a, p = loop(mm, x)
            assert torch.equal(lg[j], l) and torch.equal(attn[j], a) and torch.equal(ps[j], p), (route, j)


def test_a_dsmil_model_raises():
    from mhim_mil_amd import _lib as L
    from mhim_mil_amd.mhim import MHIM
    torch.manual_seed(0)
    m = MHIM(baseline="dsmil", n_classes=CC, input_dim=D, merge_enable=False).to(DEV).eval()
    xs = _dev(bags_np(1500, sizes=(20, 30)))
    with pytest.raises(L.MhimxError, match="TransMIL"):
        m.infer_cls_attn(xs)
    with pytest.raises(L.MhimxError, match="TransMIL"):
        m.infer_cls_topk(xs, 2)
    assert len(m.infer_many(xs, return_attn=True)[1]) == 2           # (those models have infer_many(return_attn=True))
