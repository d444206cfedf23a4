"""Ragged multi-bag TransMIL inference (mhimx_infer_transmil_run, csrc/infer_transmil.hip) on the GPU: the eval-mode MHIM(TransMIL)
forward of bags of different row counts in one C call, against the CPU oracle (oracle.mhim_oracle.forward_test per bag), the module's own
forward_test loop, the single-bag kernels stage by stage (through the workspace layout), and MHIM.infer_many / validate(chunk=).

Tolerances: logits 1e-4 abs against the oracle - the bound tests/test_nystrom_gpu.py::test_g8_sattention holds forward_test to; the loss
1e-4 against the oracle's cross entropy of its own logits; call against loop 2e-4 (each side is within 1e-4 of the oracle; the loop's
pseudo-inverse runs through the chain kernel, the call's through launches); chunk-wide products 1e-4 of the scale against an fp64 product
of the call's own inputs (close() of test_nystrom_gpu.py); every bag-batched kernel bit for bit against the single-bag kernel.

Bag sizes: one row; either side of the PPEG 7 x 7 rule (36 / 37 tokens after the cls row counts: N = 36, 37); pad 1, 0 and 255 (N = 254,
255, 256: the last with l = 2); l = 3 (600); more than 32 chunks of 64 tokens and past forward_test's n >= 2048 kernel switch (2100)."""
import functools
import types

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 256
SIZES = (1, 36, 37, 254, 255, 256, 600, 2100)
CLASSES = (2, 4)
SEEDS = {2: (41, 700), 4: (43, 760)}             # class count -> (state seed, first bag seed)
LOGIT_TOL = 1e-4
KW = dict(act="gelu", dropout=0.0, merge_enable=False)


# ------------------------------------------------------------------------------------------------ data (CPU only)
def state(seed, cc, d=D):
    """synth.mhim_state for TransMIL with NON-zero feature / predictor biases (the init law's are zero: those paths would go unchecked)."""
    st = synth.mhim_state(seed, input_dim=d, n_classes=cc, baseline="selfattn", merge_enable=False)
    st["feature.0.bias"] = (0.05 * synth.normal(seed + 900, (512,))).astype(np.float32)
    st["predictor.bias"] = (0.05 * synth.normal(seed + 901, (cc,))).astype(np.float32)
    return st


def bags_np(seed0, sizes=SIZES, d=D):
    return [synth.bag(seed0 + j, n, d) for j, n in enumerate(sizes)]


def labels_of(cc, n=len(SIZES)):
    return [(3 * j + 1) % cc for j in range(n)]


@functools.lru_cache(maxsize=None)
def reference(cc):
    """The oracle's logits [8, C] and losses [8] for the parity call of class count ``cc``: computed once, shared, never modified."""
    sseed, bseed = SEEDS[cc]
    po, cfg = O.as_torch(state(sseed, cc)), O.Cfg(baseline="selfattn", **KW)
    lg, ls = [], []
    with torch.no_grad():
        for x, y in zip(bags_np(bseed), labels_of(cc)):
            l = O.forward_test(torch.from_numpy(x), po, cfg).reshape(-1)
            lg.append(l.float().numpy())
            ls.append(float(O.cross_entropy(l, y)))
    return np.stack(lg), np.array(ls)


# ------------------------------------------------------------------------------------------------ device helpers
def _ops():
    from mhim_mil_amd import ops
    return ops


def build(sd, cc, d=D, **kw):
    from mhim_mil_amd.mhim import MHIM
    args = dict(KW)
    args.update(kw)
    m = MHIM(baseline="selfattn", n_classes=cc, input_dim=d, **args)
    sd = dict(sd)
    if "merge.global_q_mm" in sd:
        sd["merge.global_q"] = sd["merge.global_q_mm"]
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    m.online_encoder.layer1.attn.dropout = 0.0           # (the to_out dropouts of a train-mode model: zeroed, as in the Nystrom parity tests)
    m.online_encoder.layer2.attn.dropout = 0.0
    return m.eval()


def _dev(xs):
    return [torch.from_numpy(x).to(DEV) for x in xs]


@functools.lru_cache(maxsize=None)
def model(cc):
    return build(state(SEEDS[cc][0], cc), cc)


@functools.lru_cache(maxsize=None)
def parity_bags(cc):
    return tuple(_dev(bags_np(SEEDS[cc][1])))


def close(got, ref, rtol, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------------------------------------ 3. stage by stage (runs first)
@torch.no_grad()
def test_stages_match_the_single_bag_kernels_through_the_layout(monkeypatch):
    """Every stage of one call over the eight bags, read through mhimx_infer_transmil_layout and fed with the call's own upstream buffer
    of that bag: the bag-batched kernels and the landmark stage bit for bit against the single-bag launches, the two chunk-wide products
    against fp64."""
    import ctypes as C
    from mhim_mil_amd import _lib as L, nystrom as NY
    monkeypatch.setattr(NY, "_CHAIN", False)
    ops, lib = _ops(), L.lib()
    cc = 2
    m, xs = model(cc), list(parity_bags(cc))
    ws = torch.full((int(ops.infer_transmil_ws_bytes(m._infer_transmil_cfg(), xs)),), 255, dtype=torch.uint8, device=DEV)   # NaN-poisoned
    r = ops.infer_transmil_many(m._infer_transmil_cfg(), xs, want_z=True, ws=ws)
    torch.cuda.synchronize()
    lo, nb, tok = r.layout, len(xs), int(r.layout.tokens)
    assert tok == sum(256 * ((n + 1 + 255) // 256) for n in SIZES)
    enc = m.online_encoder
    scale = enc.layer1.attn.scale
    pe = enc.pos_embedding
    for l, layer in enumerate((enc.layer1, enc.layer2)):
        X, QKV, OUT, Y = (r.view(k, (tok, w), l) for k, w in (("x", 512), ("qkv", 1536), ("out", 512), ("y", 512)))
        LM, A2, Z = r.view("lm", (nb, 256, 1024), l), r.view("a2", (nb, 8, 256, 256), l), r.view("z", (nb, 8, 256, 256), l)
        A3V, LSE3, W2 = r.view("a3v", (nb, 8, 256, 64), l), r.view("lse3", (nb, 8, 256), l), r.view("w2", (nb, 8, 256, 64), l)
        att = layer.attn
        for b, N in enumerate(SIZES):
            t0, T, pad = int(lo.tok0[b]), int(lo.T[b]), int(lo.pad[b])
            assert T == 256 * ((N + 256) // 256) and pad == T - N - 1
            what = f"layer {l} bag {b} (N = {N})"
            x, qkv, out, y = X[t0 + pad:t0 + T], QKV[t0:t0 + T], OUT[t0:t0 + T], Y[t0 + pad:t0 + T]
            # chunk-wide: to_qkv of the LayerNorm rows, exact zeros on the pad rows; to_out + bias + residual
            xn = torch.nn.functional.layer_norm(x.double(), (512,), layer.norm.weight.double(), layer.norm.bias.double())
            close(qkv[pad:], xn @ att.to_qkv.weight.double().t(), 1e-4, what + " qkv")
            assert torch.count_nonzero(qkv[:pad]).item() == 0 and not torch.isnan(qkv[:pad]).any(), what + " qkv pad rows"
            close(y, x.double() + out[pad:].double() @ att.to_out[0].weight.double().t() + att.to_out[0].bias.double(), 1e-4, what + " to_out")
            # bag-batched landmark means
            lm = torch.empty((256, 1024), device=DEV)
            L.check(lib.mhimx_landmark_mean(NY._st(), NY._ptr(qkv), 1536, T, T // 256, 1024, NY._ptr(lm)), "landmark_mean")
            assert torch.equal(LM[b], lm), what + " landmark means"
            # landmark stage: a2 and the pseudo-inverse, launch per product
            a2, z, _, _, _ = NY._landmark_pinv_forward(LM[b].contiguous(), scale)
            assert torch.equal(A2[b], a2), what + " a2"
            assert torch.equal(Z[b], z), what + " z"
            # bag-batched a3v + merge
            no = ops.NysOperands(qkv, LM[b].contiguous(), scale)
            a3v, lse3 = ops.nys_a3v_fwd(no)
            assert torch.equal(A3V[b], a3v) and torch.equal(LSE3[b], lse3), what + " a3v / lse3"
            # bag-batched residual convolution + out launch, on the call's own w2
            wc = att.res_conv.weight.reshape(8, -1).contiguous()
            o = torch.empty((T, 512), device=DEV)
            L.check(lib.mhimx_resconv(NY._st(), NY._ptr(qkv, 1024), 1536, NY._ptr(wc), 33, 64, T, 512, NY._ptr(o), 512, 0, 0), "resconv")
            o, _ = ops.nys_out_fwd(no, W2[b].contiguous(), o, accumulate=True)
            assert torch.equal(out, o), what + " block output"
            if l == 0:                               # bag-batched PPEG: the rows going into layer 2
                x2 = NY.PPEG.apply(y.contiguous(), pe.proj.weight, pe.proj1.weight, pe.proj2.weight, pe.proj.bias, pe.proj1.bias, pe.proj2.bias, 0, 1)
                assert torch.equal(r.view("x", (tok, 512), 1)[t0 + pad:t0 + T], x2), what + " PPEG"
    # tail: the cls rows after the final norm, the predictor
    cls = r.view("cls", (nb, 512))
    assert torch.equal(cls, r.z)
    Y2 = r.view("y", (tok, 512), 1)
    rows = torch.stack([Y2[int(lo.tok0[b]) + int(lo.pad[b])] for b in range(nb)]).double()
    ref = torch.nn.functional.layer_norm(rows, (512,), enc.norm.weight.double(), enc.norm.bias.double())
    close(cls, ref, 1e-5, "final norm")
    close(r.logits, ref @ m.predictor.weight.double().t() + m.predictor.bias.double(), 1e-5, "predictor")


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("cc", CLASSES)
def test_infer_many_matches_the_oracle(cc):
    m, xs = model(cc), list(parity_bags(cc))
    labels = torch.tensor(labels_of(cc), device=DEV)
    logits, loss = m.infer_many(xs, labels=labels)
    assert m.last["infer_native"] is True and m.last["infer_calls"] == 1
    ref_lg, ref_ls = reference(cc)
    got = logits.cpu().numpy()
    print("max |logits - oracle| per bag:", np.abs(got - ref_lg).max(1))
    assert got.shape == (len(SIZES), cc)
    for j, n in enumerate(SIZES):
        np.testing.assert_allclose(got[j], ref_lg[j], atol=LOGIT_TOL, rtol=0, err_msg=f"bag {j} (N = {n})")
    np.testing.assert_allclose(loss.cpu().numpy(), ref_ls, atol=1e-4, rtol=0)
    # a label outside [0, C): NaN for that bag alone
    bad = labels.clone()
    bad[2] = cc
    _, loss2 = m.infer_many(xs, labels=bad)
    assert torch.isnan(loss2[2]) and torch.equal(loss2[[0, 1, 3]], loss[[0, 1, 3]])


# ------------------------------------------------------------------------------------------------ 2. against the loop of the same build
def test_call_matches_the_forward_test_loop_and_its_seed_stream():
    cc = 2
    m, xs = model(cc), list(parity_bags(cc))
    m2 = build(state(SEEDS[cc][0], cc), cc)
    m._step = m2._step = 17
    native = m.infer_many(xs)
    assert m.last["infer_native"] is True
    loop = torch.cat([m2.forward_test(x).reshape(1, -1) for x in xs])
    print("max |native - loop| per bag:", (native - loop).abs().max(1).values.cpu().numpy())
    assert (native - loop).abs().max().item() <= 2e-4
    assert m._step == m2._step == 17 + 3 * len(xs)


# ------------------------------------------------------------------------------------------------ 4. neighbours do not matter
def test_a_bag_s_bits_do_not_depend_on_its_neighbours():
    cc = 4
    m, xs = model(cc), list(parity_bags(cc))
    base = m.infer_many(xs)
    rev = m.infer_many(xs[::-1])
    assert torch.equal(rev.flip(0), base)
    for j in (0, 3, 5, 7):
        assert torch.equal(m.infer_many([xs[j]])[0], base[j]), j
    assert torch.equal(m.infer_many(xs), base)                           # and two runs give the same bytes


# ------------------------------------------------------------------------------------------------ 5. graph capture
def test_a_captured_call_replays_the_eager_bits_on_new_contents():
    cc = 2
    m = model(cc)
    ops = _ops()
    cfg = m._infer_transmil_cfg()
    sizes = (300, 37, 1, 600)
    xs = _dev(bags_np(900, sizes=sizes))
    labels = torch.tensor([1, 0, 1, 1], device=DEV)
    ops.infer_transmil_many(cfg, xs, labels=labels)                      # (the first call on the device: outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # one stream, no parallel branches
        r = ops.infer_transmil_many(cfg, xs, labels=labels)
    for x, new in zip(xs, bags_np(950, sizes=sizes)):                    # new bag contents in the same buffers
        x.copy_(torch.from_numpy(new))
    eager = ops.infer_transmil_many(cfg, xs, labels=labels)
    elog, eloss = eager.logits.clone(), eager.loss.clone()
    for _ in range(2):
        r.logits.zero_(); r.loss.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(r.logits, elog) and torch.equal(r.loss, eloss)


# ------------------------------------------------------------------------------------------------ 6. chunking
def test_chunks_by_bag_count_and_by_rows_give_the_same_logits(monkeypatch):
    cc = 2
    m = model(cc)
    xs = _dev([synth.bag(1200 + j, 20 + 7 * (j % 5), D) for j in range(33)])
    one = torch.cat([m.infer_many(xs[:32]), m.infer_many(xs[32:])])
    got = m.infer_many(xs)
    assert m.last == {"infer_native": True, "infer_calls": 2} and torch.equal(got, one)
    monkeypatch.setattr(type(m), "infer_rows_per_call", lambda self: 100)
    small = m.infer_many(xs[:12])
    assert m.last["infer_native"] is True and m.last["infer_calls"] >= 3
    assert torch.equal(small, got[:12])


# ------------------------------------------------------------------------------------------------ 7. half-precision bags
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_bags_give_the_bits_of_the_widened_call(dtype):
    cc = 2
    m = model(cc)
    xs = [x.to(dtype) for x in _dev(bags_np(1300, sizes=(1, 37, 255, 300)))]
    half = m.infer_many(xs)
    assert m.last["infer_native"] is True
    assert torch.equal(half, m.infer_many([x.float() for x in xs]))


# ------------------------------------------------------------------------------------------------ 8. routes that stay on the loop
def test_routes_outside_the_call_keep_the_loop():
    from mhim_mil_amd import _lib as L
    cc = 2
    xs = _dev(bags_np(1400, sizes=(40, 300)))
    m = build(state(SEEDS[cc][0], cc), cc)
    lg, attn = m.infer_many(xs, return_attn=True)
    assert m.last["infer_native"] is False
    for j, x in enumerate(xs):
        o = m.forward_test(x, return_attn=True)
        assert torch.equal(lg[j], o[0].reshape(-1)) and all(torch.equal(a, b) for a, b in zip(attn[j], o[1]))
    for kind in ("merge_test", "train", "f32"):
        if kind == "merge_test":
            sd = synth.mhim_state(SEEDS[cc][0], input_dim=D, n_classes=cc, baseline="selfattn", merge_k=5)
            mm = build(sd, cc, merge_enable=True, merge_k=5, merge_test=True)
            mm.merge.dropout = 0.0
        elif kind == "train":
            mm = build(state(SEEDS[cc][0], cc), cc).train()
        else:
            mm = build(state(SEEDS[cc][0], cc), cc, prec="f32")
        s0 = mm._step
        got = mm.infer_many(xs)
        assert mm.last["infer_native"] is False, kind
        mm._step = s0
        ref = torch.cat([mm.forward_test(x).reshape(1, -1) for x in xs])
        assert torch.equal(got, ref), kind
    with pytest.raises(L.MhimxError, match="one attention map per layer"):
        m.infer_topk(xs, 2)


# ------------------------------------------------------------------------------------------------ 9. validation
VAL_ARGS = types.SimpleNamespace(model="mhim", baseline="selfattn", n_classes=2, bin_metric=False, bootstrap_mode=(), best_metric_index=0)


def test_validate_in_chunks_returns_what_the_loop_returns():
    from mhim_mil_amd import validate as V
    from mhim_mil_amd.engine import CommonMIL
    m = model(2)
    rng = np.random.default_rng(0)
    loader = [{"input": torch.from_numpy(synth.bag(1500 + b, int(rng.integers(20, 120)), D)).unsqueeze(0), "target": torch.tensor([b % 2])}
              for b in range(12)]
    m.last = None
    out = V.validate(CommonMIL(VAL_ARGS), VAL_ARGS, m, loader, status="val", chunk=5)
    assert m.last["infer_native"] is True and m.last["infer_calls"] == 1        # (validate_many hands 5 bags to a call)
    base = V.validate(CommonMIL(VAL_ARGS), VAL_ARGS, m, loader, status="val", chunk=0)
    assert len(out) == len(base)
    np.testing.assert_allclose(out[0], base[0], atol=1e-6)              # the metrics
    # the mean loss: the two routes' logits differ by at most 2e-4 (test 2's bound) and the cross entropy moves by at most twice that
    np.testing.assert_allclose(out[2], base[2], atol=4e-4)
