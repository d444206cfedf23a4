"""Ragged multi-bag DSMIL inference (mhimx_infer_dsmil_run, csrc/infer_dsmil.hip) on the GPU: the eval-mode MHIM(DSMIL) forward of bags of
different row counts in one C call, against the CPU oracle (oracle.mhim_oracle.forward_test per bag), the module's own forward_test loop,
and MHIM.infer_many / validate(chunk=).

Tolerances are the ones tests/test_dsmil_gpu.py::test_g13_dsmil_module_vs_reference_fixture holds the DSMIL encoder to against reference
fixtures: bag and max-instance logits 1e-4 abs, B atol 2e-5 / rtol 1e-3, attention atol 2e-5 / rtol 1e-4; the loss 2e-5 relative to the
fp64 cross entropy of the oracle's mix.  The critical rows must equal the oracle's arg-max exactly; the committed seeds keep the two
largest classes[:, c] of every bag at least 1e-3 of max |classes| apart (far above the 3-term bf16 form's ~2^-16), which
tests/test_infer_dsmil_cpu.py checks without a GPU and the parity test asserts again on the data it uses.

The data helpers at the top touch no device: the CPU test file imports them."""
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
SIZES = (1, 31, 32, 33, 160, 161, 255, 256, 257, 513, 700)
CLASSES = (2, 3, 16)
# class count -> (state seed, first bag seed): chosen on the CPU so that the oracle's data meets assert_gap_and_coverage
SEEDS = {2: (151, 1600), 3: (52, 620), 16: (113, 1240)}
LOGIT_TOL = 1e-4
B_TOL = dict(atol=2e-5, rtol=1e-3)
ATTN_TOL = dict(atol=2e-5, rtol=1e-4)
GAP = 1e-3
KW = dict(act="gelu", dropout=0.0, merge_enable=False)


# ------------------------------------------------------------------------------------------------ data (CPU only)
def state(seed, cc, d=D, **kw):
    """synth.mhim_state for DSMIL with a NON-zero feature bias (the init law's is zero: that bias path would go unchecked)."""
    kw.setdefault("merge_enable", False)
    st = synth.mhim_state(seed, input_dim=d, n_classes=cc, baseline="dsmil", **kw)
    st["feature.0.bias"] = (0.05 * synth.normal(seed + 900, (512,))).astype(np.float32)
    return st


def bags_np(seed0, sizes=SIZES, d=D):
    return [synth.bag(seed0 + j, n, d) for j, n in enumerate(sizes)]


def oracle_bag(x, po, cfg):
    """What the oracle computes for one bag [N, D] (numpy): both logit rows, B, the instance score, classes and its arg-max rows."""
    xt = torch.from_numpy(x)
    with torch.no_grad():
        (lb, li), B = O.forward_test(xt, po, cfg)
        _, attn = O.forward_test(xt, po, cfg, return_attn=True)
        h = O.feature(xt, po, cfg.act)
        classes = O._linear(h, po["online_encoder.i_classifier.0.weight"], po["online_encoder.i_classifier.0.bias"])
    f = lambda t: t.detach().float().numpy()
    return dict(N=x.shape[0], lb=f(lb).reshape(-1), li=f(li).reshape(-1), B=f(B), attn=f(attn).reshape(-1), classes=f(classes),
                crit=classes.argmax(0).numpy())


@functools.lru_cache(maxsize=None)
def reference(cc):
    """The oracle's outputs for the parity call of class count ``cc`` (11 bags, one per size): computed once, shared, never modified."""
    sseed, bseed = SEEDS[cc]
    po, cfg = O.as_torch(state(sseed, cc)), O.Cfg(baseline="dsmil", attn2score=True, **KW)
    return tuple(oracle_bag(x, po, cfg) for x in bags_np(bseed))


def assert_gap_and_coverage(ref):
    """The parity test's condition on the oracle's own data: a clear arg-max everywhere, one critical row in a chunk >= 1, one in a last
    partial 32-row tile that is not the bag's first tile."""
    late_chunk = part_tile = False
    for r in ref:
        cl, n = r["classes"], r["N"]
        scale = float(np.abs(cl).max())
        for c in range(cl.shape[1]):
            if n > 1:
                top = np.sort(cl[:, c])[-2:]
                assert top[1] - top[0] >= GAP * scale, (n, c, float(top[1] - top[0]), scale)
            row = int(r["crit"][c])
            late_chunk |= row >= 256
            part_tile |= n % 32 != 0 and n > 32 and row >= (n // 32) * 32
    assert late_chunk and part_tile, (late_chunk, part_tile)


# ------------------------------------------------------------------------------------------------ device helpers
def _ops():
    from mhim_mil_amd import ops
    return ops


def build(sd, cc, d=D, **kw):
    from mhim_mil_amd.mhim import MHIM
    args = dict(KW)
    args.update(kw)
    m = MHIM(baseline="dsmil", n_classes=cc, input_dim=d, **args)
    sd = dict(sd)
    if "merge.global_q_mm" in sd:
        sd["merge.global_q"] = sd["merge.global_q_mm"]
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    m = m.to(DEV)
    if args.get("merge_enable", True):
        m.merge.dropout = 0.0
    return m.eval()


def _dev(xs):
    return [torch.from_numpy(x).to(DEV) for x in xs]


def _call(m, xs, labels=None, ws=None, no_norm=False):
    """One mhimx_infer_dsmil_run through the thin wrapper: everything the boundary can return."""
    return _ops().infer_dsmil_many(m._infer_dsmil_cfg(no_norm), xs, labels=labels, want_attn=True, want_B=True, want_crit=True, ws=ws)


FIELDS = ("logits_bag", "logits_ins", "logits", "B", "crit", "loss")


def _bag_outputs(r, j):
    out = [getattr(r, f)[j].clone() for f in FIELDS if getattr(r, f) is not None]
    return out + [r.attn[r.offsets[j]:r.offsets[j + 1]].clone()]


def _loop_mix(m, xs, **kw):
    """validate_func's mix over the forward_test loop: the parent's only route."""
    rows = []
    for x in xs:
        lg = m.forward_test(x, **kw)[0]
        rows.append((0.5 * lg[0] + 0.5 * lg[1]).reshape(1, -1))
    return torch.cat(rows)


# ------------------------------------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("cc", CLASSES)
def test_oracle_parity(cc):
    ref = reference(cc)
    assert_gap_and_coverage(ref)                                         # the test cannot hide a wrong arg-max
    sseed, bseed = SEEDS[cc]
    m = build(state(sseed, cc), cc, attn2score=True)
    xs = _dev(bags_np(bseed))
    labels = torch.tensor([j % cc for j in range(len(xs))], device=DEV)
    r = _call(m, xs, labels=labels)
    torch.cuda.synchronize()
    assert r.offsets[-1] == sum(SIZES) and r.crit.shape == (len(SIZES), cc) and r.crit.dtype == torch.int64
    got = {f: getattr(r, f).cpu().numpy() for f in FIELDS}
    attn = r.attn.cpu().numpy()
    worst = dict(lb=0.0, li=0.0, B=0.0, attn=0.0)
    for j, o in enumerate(ref):
        worst["lb"] = max(worst["lb"], float(np.abs(got["logits_bag"][j] - o["lb"]).max()))
        worst["li"] = max(worst["li"], float(np.abs(got["logits_ins"][j] - o["li"]).max()))
        worst["B"] = max(worst["B"], float(np.abs(got["B"][j] - o["B"]).max()))
        worst["attn"] = max(worst["attn"], float(np.abs(attn[r.offsets[j]:r.offsets[j + 1]] - o["attn"]).max()))
    print(f"[infer dsmil C={cc}] worst abs errors {worst}")
    mix = np.stack([0.5 * o["lb"].astype(np.float64) + 0.5 * o["li"].astype(np.float64) for o in ref])
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(mix), labels.cpu(), reduction="none").numpy()
    print(f"[infer dsmil C={cc}] worst relative loss error {float(np.abs(got['loss'] / ce - 1.0).max()):.3e}")
    for j, o in enumerate(ref):
        msg = f"bag {j} (N = {o['N']})"
        np.testing.assert_array_equal(got["crit"][j], o["crit"], err_msg=msg)          # ALL bags and classes, none left out
        np.testing.assert_allclose(got["logits_bag"][j], o["lb"], atol=LOGIT_TOL, rtol=0, err_msg=msg)
        np.testing.assert_allclose(got["logits_ins"][j], o["li"], atol=LOGIT_TOL, rtol=0, err_msg=msg)
        np.testing.assert_allclose(got["logits"][j], mix[j], atol=LOGIT_TOL, rtol=0, err_msg=msg)
        np.testing.assert_allclose(got["B"][j], o["B"], err_msg=msg, **B_TOL)
        np.testing.assert_allclose(attn[r.offsets[j]:r.offsets[j + 1]], o["attn"], err_msg=msg, **ATTN_TOL)
    assert (got["crit"][0] == 0).all()                                   # N = 1: one row critical for every class
    np.testing.assert_allclose(got["loss"], ce, rtol=2e-5, atol=0)


# ------------------------------------------------------------------------------------------------ 2. the attention rules and no_norm
@pytest.mark.parametrize("cc", [2, 3])
@pytest.mark.parametrize("no_norm", [False, True])
def test_attention_without_cls_attn_matches_the_module(cc, no_norm):
    """attn2score=False: max_c A[m, c], or max_c of the scaled raw scores with no_norm - against the model's own forward_test (the oracle's
    dsmil() returns the softmax maximum even under no_norm).  attn2score=True is test_oracle_parity's attention."""
    sseed, bseed = SEEDS[cc]
    m = build(state(sseed, cc), cc, attn2score=False)
    xs = _dev(bags_np(bseed, sizes=(1, 33, 257, 700)))
    logits, attn = m.infer_many(xs, return_attn=True, no_norm=no_norm)
    assert m.last["infer_native"] is True
    for j, x in enumerate(xs):
        lg, a = m.forward_test(x, return_attn=True, no_norm=no_norm)
        assert attn[j].shape == (x.shape[0],)
        np.testing.assert_allclose(attn[j].cpu().numpy(), a.reshape(-1).cpu().numpy(), err_msg=f"bag {j}", **ATTN_TOL)
        np.testing.assert_allclose(logits[j].cpu().numpy(), (0.5 * lg[0] + 0.5 * lg[1]).reshape(-1).cpu().numpy(), atol=LOGIT_TOL, rtol=0)
        if not no_norm:
            assert float(attn[j].max()) <= 1.0 + 1e-6 and float(attn[j].min()) >= 0.0


def test_no_norm_leaves_the_cls_attn_score_alone():
    cc = 2
    sseed, bseed = SEEDS[cc]
    m = build(state(sseed, cc), cc, attn2score=True)
    xs = _dev([bags_np(bseed)[k] for k in (3, 8)])                      # the parity call's bags of 33 and 257 rows
    a0, a1 = _call(m, xs), _call(m, xs, no_norm=True)
    assert torch.equal(a0.attn, a1.attn) and torch.equal(a0.logits, a1.logits)
    for j, o in enumerate(reference(cc)[k] for k in (3, 8)):
        np.testing.assert_allclose(a1.attn[a1.offsets[j]:a1.offsets[j + 1]].cpu().numpy(), o["attn"], **ATTN_TOL)


# ------------------------------------------------------------------------------------------------ 3. route equivalence
def test_infer_many_native_against_the_forward_test_loop():
    cc = 3
    sseed, bseed = SEEDS[cc]
    st = state(sseed, cc)
    m = build(st, cc)
    xs = _dev(bags_np(bseed))
    labels = torch.tensor([j % cc for j in range(len(xs))], device=DEV)
    step0 = m._step
    logits, attn, loss = m.infer_many(xs, labels=labels, return_attn=True)
    assert m.last["infer_native"] is True and m.last["infer_calls"] == 1 and m._step == step0 + len(xs)
    lb, li, B = m.last["infer_parts"]
    assert logits.shape == (len(xs), cc) and lb.shape == li.shape == (len(xs), cc) and B.shape == (len(xs), cc, 512)
    assert torch.equal(logits, 0.5 * lb + 0.5 * li)
    for j, x in enumerate(xs):
        (flb, fli), fB = m.forward_test(x)
        _, fa = m.forward_test(x, return_attn=True)
        msg = f"bag {j} (N = {x.shape[0]})"
        np.testing.assert_allclose(lb[j].cpu().numpy(), flb.reshape(-1).cpu().numpy(), atol=LOGIT_TOL, rtol=0, err_msg=msg)
        np.testing.assert_allclose(li[j].cpu().numpy(), fli.reshape(-1).cpu().numpy(), atol=LOGIT_TOL, rtol=0, err_msg=msg)
        np.testing.assert_allclose(B[j].cpu().numpy(), fB[0].cpu().numpy(), err_msg=msg, **B_TOL)
        np.testing.assert_allclose(attn[j].cpu().numpy(), fa.reshape(-1).cpu().numpy(), err_msg=msg, **ATTN_TOL)
    mix = _loop_mix(m, xs)
    np.testing.assert_allclose(logits.cpu().numpy(), mix.cpu().numpy(), atol=LOGIT_TOL, rtol=0)
    ce = torch.nn.functional.cross_entropy(mix.double(), labels, reduction="none")
    np.testing.assert_allclose(loss.cpu().numpy(), ce.cpu().numpy(), rtol=2e-4)
    # [1, N, D] entries, as a loader yields them
    assert torch.equal(m.infer_many([x[None] for x in xs]), logits)


@pytest.mark.parametrize("kind", ["merge_test", "train", "f32"])
def test_models_outside_the_call_take_the_loop_and_return_the_mix(kind):
    cc = 2
    sseed, bseed = SEEDS[cc]
    if kind == "merge_test":
        m = build(state(sseed, cc, merge_enable=True, merge_k=5), cc, merge_enable=True, merge_k=5, merge_test=True)
    elif kind == "f32":
        m = build(state(sseed, cc), cc, prec="f32")
    else:
        m = build(state(sseed, cc), cc).train()
    xs = _dev(bags_np(bseed, sizes=(33, 160, 257)))
    labels = torch.tensor([0, 1, 1], device=DEV)
    logits, loss = m.infer_many(xs, labels=labels)                      # (the parent raised here)
    assert m.last["infer_native"] is False and m.last["infer_calls"] == 0
    mix = _loop_mix(m, xs)
    assert torch.equal(logits, mix)
    assert torch.equal(loss, torch.nn.functional.cross_entropy(mix, labels, reduction="none"))
    lb, li, B = m.last["infer_parts"]
    assert torch.equal(0.5 * lb + 0.5 * li, logits) and B.shape == (3, cc, 512)
    _, attn = m.infer_many(xs, return_attn=True)
    for j, x in enumerate(xs):
        assert torch.equal(attn[j], m.forward_test(x, return_attn=True)[1].reshape(-1))


# ------------------------------------------------------------------------------------------------ 4. position independence (bits)
def test_a_bag_has_the_same_bits_alone_first_of_32_and_last_of_32():
    from mhim_mil_amd import _lib as L
    cc = 3
    sseed, bseed = SEEDS[cc]
    m = build(state(sseed, cc), cc, attn2score=False)                   # (attention through the finalize launch's blocks)
    a = _dev([synth.bag(77, 513, D)])[0]
    sizes = [1, 700, 1, 33, 256, 1, 31, 257] + [1 + 19 * j for j in range(23)]
    others = _dev(bags_np(500, sizes=sizes))
    assert len(others) == L.INFER_MAX - 1 and sizes.count(1) >= 3
    lists = ([a], [a] + others, others + [a])
    need = max(_ops().infer_dsmil_ws_bytes(m._infer_dsmil_cfg(), xs) for xs in lists)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    outs = []
    for xs, pos in zip(lists, (0, 0, L.INFER_MAX - 1)):
        ws.fill_(255)                                                    # NaN in every float the call does not write itself
        labels = torch.zeros(len(xs), dtype=torch.int64, device=DEV)
        labels[pos] = 2
        r = _call(m, xs, labels=labels, ws=ws)
        torch.cuda.synchronize()
        outs.append(_bag_outputs(r, pos))
        if len(xs) > 1:
            assert not torch.isnan(r.logits).any() and not torch.isnan(r.attn).any() and not torch.isnan(r.B).any()
    assert not any(torch.isnan(t).any() for t in outs[0])
    for o in outs[1:]:
        for t0, t1 in zip(outs[0], o):
            assert torch.equal(t0, t1)
    # two runs of a call give equal bits
    r1, r2 = _call(m, lists[1]), _call(m, lists[1])
    torch.cuda.synchronize()
    for f in FIELDS[:5] + ("attn",):
        assert torch.equal(getattr(r1, f), getattr(r2, f)), f


# ------------------------------------------------------------------------------------------------ 5. chunking
def test_long_lists_are_chunked_in_loader_order_under_the_dsmil_row_cap():
    cc = 2
    sseed, _ = SEEDS[cc]
    m = build(state(sseed, cc), cc)
    sizes = [20 + 7 * j for j in range(40)]
    xs = _dev(bags_np(600, sizes=sizes))
    labels = torch.arange(40, device=DEV) % 2
    logits, loss = m.infer_many(xs, labels=labels)
    assert m.last["infer_native"] is True and m.last["infer_calls"] == 2 and logits.shape == (40, cc) and loss.shape == (40,)
    one = torch.cat([_call(m, [x]).logits for x in xs])
    assert torch.equal(logits, one)                                      # loader order; a bag's bits do not depend on its chunk
    m.infer_row_cap = 1200                                               # the DSMIL cap derived from it is honoured
    cap = m.infer_rows_per_call()
    assert 0 < cap < 600
    chunks = m.infer_chunks(xs)
    assert all(hi - lo == 1 or sum(sizes[lo:hi]) <= cap for lo, hi in chunks) and len(chunks) > 2
    logits2 = m.infer_many(xs)
    assert m.last["infer_calls"] == len(chunks) and torch.equal(logits2, logits)


# ------------------------------------------------------------------------------------------------ 6. half precision, pitched bags
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_bags_give_the_bits_of_the_fp32_call_on_the_widened_rows(dtype):
    cc = 2
    sseed, bseed = SEEDS[cc]
    m = build(state(sseed, cc), cc, attn2score=False)
    half = [x.to(dtype) for x in _dev(bags_np(bseed, sizes=(1, 33, 257, 700)))]
    pitched = torch.zeros((161, D + 8), dtype=dtype, device=DEV)
    pitched[:, :D] = torch.from_numpy(synth.bag(88, 161, D)).to(DEV).to(dtype)
    pitched[:, D:] = float("nan")                                        # the padding is never read
    half.append(pitched[:, :D])
    assert half[-1].stride(0) == D + 8 and not half[-1].is_contiguous()
    rh = _call(m, half)
    rf = _call(m, [x.float().contiguous() for x in half])
    torch.cuda.synchronize()
    for f in FIELDS[:5] + ("attn",):
        assert torch.equal(getattr(rh, f), getattr(rf, f)), f
    logits = m.infer_many(half)
    assert m.last["infer_native"] is True and torch.equal(logits, rh.logits)
    # a pitched fp32 bag is read where it lies too
    p32 = torch.full((161, D + 4), float("nan"), device=DEV)
    p32[:, :D] = half[-1].float()
    assert torch.equal(_call(m, [p32[:, :D]]).logits[0], rf.logits[-1])


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_a_captured_call_replays_the_eager_bits():
    cc = 3
    sseed, bseed = SEEDS[cc]
    m = build(state(sseed, cc), cc, attn2score=False)
    xs = _dev(bags_np(bseed, sizes=(700, 33, 1, 257)))
    labels = torch.tensor([1, 0, 2, 1], device=DEV)
    eager = _call(m, xs, labels=labels)                                  # (also the first call on the device: outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # one stream, no parallel branches
        r = _call(m, xs, labels=labels)
    for _ in range(2):
        for f in FIELDS + ("attn",):
            getattr(r, f).zero_()
        g.replay()
        torch.cuda.synchronize()
        for f in FIELDS + ("attn",):
            assert torch.equal(getattr(r, f), getattr(eager, f)), f


# ------------------------------------------------------------------------------------------------ 8. validation
VAL_ARGS = types.SimpleNamespace(model="mhim", baseline="dsmil", n_classes=2, bin_metric=False, bootstrap_mode=(), best_metric_index=0)
VAL_SEED, VAL_BAGS = 31, 10


def val_state():
    """The validation model: class 1's instance bias is raised so that the toy set's predictions fall on both sides (a constant added to
    a column of classes moves neither the critical rows nor the bag logits)."""
    st = state(VAL_SEED, 2)
    st["online_encoder.i_classifier.0.bias"] = st["online_encoder.i_classifier.0.bias"] + np.array([0.0, 2.6], np.float32)
    return st


def val_set():
    """A toy validation set whose bags differ in scale, so that their logits are well separated (checked by the test on the loop's
    logits: no two bags closer than 1e-3 in the class-1 margin, no margin within 1e-3 of zero)."""
    rng = np.random.default_rng(3)
    bags, labels = [], []
    for b in range(VAL_BAGS):
        n = int(rng.integers(20, 300))
        bags.append((synth.bag(700 + b, n, D) * np.float32(0.25 + 0.35 * b)).astype(np.float32))
        labels.append(b % 2)
    return bags, labels


def test_validate_in_chunks_matches_the_bag_after_bag_loop():
    from mhim_mil_amd import validate as V
    from mhim_mil_amd.engine import CommonMIL
    m = build(val_state(), 2)
    bags, labels = val_set()
    loader = [{"input": torch.from_numpy(x).unsqueeze(0), "target": torch.tensor([y])} for x, y in zip(bags, labels)]
    eng = CommonMIL(VAL_ARGS)
    m.last = None
    base = V.validate(eng, VAL_ARGS, m, loader, status="val")
    assert m.last is None                                               # chunk = 0: validate_func, bag after bag
    out = V.validate(eng, VAL_ARGS, m, loader, status="val", chunk=4)
    assert m.last["infer_native"] is True and m.last["infer_calls"] == 1
    xs = _dev(bags)
    loop = torch.cat([eng.validate_func(VAL_ARGS, model=m, bag=x, label=None, criterion=None, batch_size=1, i=0, pos=None)[0].reshape(1, -1)
                      for x in xs])
    margin = np.sort((loop[:, 1] - loop[:, 0]).cpu().numpy())
    assert np.diff(margin).min() > 1e-3 and np.abs(margin).min() > 1e-3, margin        # well separated: the metrics cannot flip
    native, _ = eng.validate_many(VAL_ARGS, m, xs, torch.tensor(labels, device=DEV), torch.nn.CrossEntropyLoss())
    np.testing.assert_allclose(native.cpu().numpy(), loop.cpu().numpy(), atol=LOGIT_TOL, rtol=0)
    assert len(out) == len(base) and type(out[0]) is type(base[0])
    assert list(out[0]) == list(base[0])                                 # metric tuples identical
    np.testing.assert_allclose(out[2], base[2], rtol=2e-4)               # mean loss
