"""Half-precision feature bags (fp16 / bf16) in the ragged native calls - mhimx_infer_run_x, mhimx_pure_window_run_x,
mhimx_ragged_window_run_x - on the GPU.  Every fp16 and bf16 value is an fp32 value, and the two kernels that read X widen in registers
in front of the fp32 kernels' unchanged split and k loop: a call on half bags must give THE BITS of the same library's fp32 entry point
on ``x.float()`` of those very tensors.  That reference is computed here, in the same test, never stored; every comparison below is
torch.equal - there is no tolerance to choose.  (One case is also held against the CPU oracle, at tests/test_infer_gpu.py's bounds.)
Inputs: synth.bag values cast to the dtype under test, a handful of elements per bag overwritten with zeros, negative values and
subnormals of that dtype (fp16: 6e-8, 3e-6); no inf, no NaN."""
import numpy as np
import pytest
import torch

from mhim_mil_amd import _lib as L
from mhim_mil_amd import synth
from oracle import mhim_oracle as O
from tests.test_infer_gpu import ATTN_TOL, LOGIT_TOL, RAW_TOL, _call, _oracle, _state
from tests.test_mhim_gpu import V2, build

pytestmark = pytest.mark.gpu
DEV = "cuda"
HALVES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
# every tile, chunk and clamped-row edge of the two launches that read X or its rows: 32-row k-steps, 160-row projection tiles, 256-row
# scorer chunks, more than one tile
INFER_SIZES = (1, 31, 32, 33, 159, 160, 161, 257, 700)
SPECIALS = {torch.float16: (0.0, -0.0, -1.75, -3.0e-3, 6e-8, -6e-8, 3e-6, 6.0e-5), torch.bfloat16: (0.0, -0.0, -1.75, -3.0e-3, 1e-39, -4e-40, 2.5)}


def _half_bag(seed, n, d, dtype, pitch=None):
    """synth.bag cast to ``dtype`` with the special values written over a few elements of the first, a middle and the last row;
    ``pitch``: the bag as a view of the first d columns of a wider tensor."""
    x = torch.from_numpy(synth.bag(seed, n, d)).to(dtype)
    sp = torch.tensor(SPECIALS[dtype], dtype=torch.float32).to(dtype)
    for r in sorted({0, n // 2, n - 1}):
        cols = torch.from_numpy(np.random.default_rng(seed + r).permutation(d)[:sp.numel()].copy())
        x[r, cols] = sp
    if dtype == torch.float16:
        assert (x[0].float().abs() < 6.2e-5).logical_and(x[0] != 0).any()           # the subnormals survived the cast
    assert torch.isfinite(x.float()).all()
    x = x.to(DEV)
    if pitch is not None:
        wide = torch.full((n, pitch), 7.0, dtype=dtype, device=DEV)
        wide[:, :d] = x
        x = wide[:, :d]
        assert x.stride(0) == pitch
    return x


def _infer_bags(d, dtype, seed=40):
    order = np.random.default_rng(seed).permutation(len(INFER_SIZES))
    sizes = [INFER_SIZES[i] for i in order]
    return [_half_bag(seed + j, n, d, dtype, pitch=d + 8 if n == 161 else None) for j, n in enumerate(sizes)], sizes


def _same(a, b, names=("logits", "z", "stats", "score", "attn", "loss")):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert x is not None and torch.equal(x, y), (name, float((x.double() - y.double()).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("d", [256, 1024])
@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_inference_on_half_bags_gives_the_bits_of_the_widened_call(dtype, d):
    m = build(_state(11, d, merge_k=5), "auto", input_dim=d, **V2).eval()
    xs, sizes = _infer_bags(d, dtype)
    wide = [x.float() for x in xs]
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, 2, size=len(xs))).to(DEV)
    half, ref = _call(m, xs, labels=labels), _call(m, wide, labels=labels)
    torch.cuda.synchronize()
    assert half.offsets == ref.offsets and not torch.isnan(ref.logits).any()
    _same(half, ref)
    # the same through the model: half bags go in as they are
    lg_h, at_h, ls_h = m.infer_many(xs, labels=labels, return_attn=True)
    assert m.last["infer_native"] is True
    lg_w, at_w, ls_w = m.infer_many(wide, labels=labels, return_attn=True)
    assert m.last["infer_native"] is True
    assert torch.equal(lg_h, lg_w) and torch.equal(ls_h, ls_w) and torch.equal(lg_h, ref.logits) and torch.equal(ls_h, ref.loss)
    assert all(torch.equal(a, b) for a, b in zip(at_h, at_w))
    _, raw_h = m.infer_many(xs, return_attn=True, no_norm=True)
    _, raw_w = m.infer_many(wide, return_attn=True, no_norm=True)
    assert all(torch.equal(a, b) for a, b in zip(raw_h, raw_w))


def test_half_inference_against_the_oracle_on_the_widened_rows():
    """fp16, D = 256: oracle.forward_test on x.float() at the bounds of tests/test_infer_gpu.py (logits 1e-4 abs, ATTN_TOL, RAW_TOL)."""
    d = 256
    st = _state(11, d, merge_k=5)
    m = build(st, "auto", input_dim=d, **V2).eval()
    po, cfg = O.as_torch(st), O.Cfg(**V2)
    xs, sizes = _infer_bags(d, torch.float16)
    r = _call(m, xs)
    torch.set_num_threads(16)
    for j, x in enumerate(xs):
        o_lg, o_a, o_raw = _oracle(x.float(), po, cfg)
        sl = slice(r.offsets[j], r.offsets[j + 1])
        msg = f"bag {j} (N = {sizes[j]})"
        np.testing.assert_allclose(r.logits[j].cpu().numpy(), o_lg, atol=LOGIT_TOL, rtol=0, err_msg=msg)
        np.testing.assert_allclose(r.attn[sl].cpu().numpy(), o_a, err_msg=msg, **ATTN_TOL)
        np.testing.assert_allclose(r.score[sl].cpu().numpy(), o_raw, err_msg=msg, **RAW_TOL)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_a_half_bag_does_not_depend_on_its_neighbours(dtype):
    from mhim_mil_amd import ops
    d = 256
    m = build(_state(3, d, merge_k=5), "auto", input_dim=d, **V2).eval()
    mine = _half_bag(1, 333, d, dtype)
    others = [_half_bag(2 + j, n, d, dtype) for j, n in enumerate((700, 45, 161, 1))]
    five = others[:2] + [mine] + others[2:]
    need = max(ops.infer_ws_bytes(m._infer_cfg(), xs) for xs in (five, [mine]))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    outs = []
    for xs, pos in ((five, 2), ([mine], 0)):
        ws.fill_(255)                                                    # NaN in every float the call does not write itself
        r = _call(m, xs, ws=ws)
        torch.cuda.synchronize()
        sl = slice(r.offsets[pos], r.offsets[pos + 1])
        outs.append((r.logits[pos].clone(), r.stats[pos].clone(), r.score[sl].clone(), r.attn[sl].clone(), r.z[pos].clone()))
    assert not any(torch.isnan(t).any() for t in outs[0])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------------------------------ 3
def _two_windows(make, bags_of, state, extra=lambda tr: []):
    """Two trainers from one state dict: one gets the half bags, the other ``x.float()`` of them.  Window 1 with update=False (the flat
    gradient, every bag's logits and losses), tr.update(), window 2 with update=True (parameters, both Adam moments, the counters)."""
    tr_h, tr_w = make(), make()
    for w, upd in enumerate((False, True)):
        xs, ls = bags_of(w)
        lg_h, lo_h = tr_h.window_step(xs, ls, update=upd)
        last_h = tr_h.last
        wide = [x.float() for x in xs]
        lg_w, lo_w = tr_w.window_step(wide, ls, update=upd)
        torch.cuda.synchronize()
        assert tr_w.last["exec"] == last_h["exec"] and tr_w.last["x_dtype"] == torch.float32
        assert last_h["x_dtype"] == xs[0].dtype
        assert len(lg_h) == len(xs)
        for j in range(len(xs)):
            assert torch.equal(lg_h[j], lg_w[j]) and torch.equal(lo_h[j], lo_w[j]), (w, j)
            assert not torch.isnan(lg_h[j]).any()
        if not upd:
            assert torch.equal(tr_h.flat.grad, tr_w.flat.grad) and float(tr_h.flat.grad.abs().max()) > 0
            tr_h.update()
            tr_w.update()
            torch.cuda.synchronize()
        for name, a, b in zip(("student", "teacher", "m", "v", "opt_step", "tick", "extra"), state(tr_h), state(tr_w)):
            assert torch.equal(a, b), (w, name, float((a.double() - b.double()).abs().max()))
        for a, b in zip(extra(tr_h), extra(tr_w)):
            assert torch.equal(a, b)
    assert tr_h.flat.step == tr_w.flat.step and tr_h.s._step == tr_w.s._step
    return last_h


@pytest.mark.parametrize("dtype, d", [(torch.float16, 256), (torch.bfloat16, 256), (torch.float16, 1024)], ids=["fp16-256", "bf16-256", "fp16-1024"])
def test_pure_window_on_half_bags_gives_the_bits_of_the_widened_window(dtype, d):
    """FusedTrainer(model="mhim_pure", accumulation_steps=5), dropout 0.25, N = 64, 97, 160, 161, 700 (D = 1024 too: the split-K slabs of
    d W1 differ with D).  The pure window's route is named by last["exec"] is True with a layout of the window's bags (the string routes
    are the full model's: tests/test_pure_window_gpu.py)."""
    from tests.test_pure_window_gpu import _trainer
    sizes = (64, 97, 160, 161, 700)

    def bags_of(w):
        return ([_half_bag(300 + 10 * w + j, n, d, dtype) for j, n in enumerate(sizes)],
                [torch.tensor([(j + w) % 2], device=DEV) for j in range(len(sizes))])

    def state(tr):
        fl = tr.flat
        return [fl.student, fl.student, fl.m, fl.v, tr.opt_step, tr.tick]

    last = _two_windows(lambda: _trainer(d, dropout=0.25, accum=5), bags_of, state)
    assert last["exec"] is True and len(last["bags"]) == len(sizes) and last["layout"].rows == sum((n + 31) // 32 * 32 for n in sizes)
    assert last["x_dtype"] == dtype
    kept = torch.cat([(b["H_student"] != 0).reshape(-1) for b in last["bags"]]).float().mean().item()
    assert abs(kept - 0.75) < 2e-2, kept                               # the dropout was on


# ------------------------------------------------------------------------------------------------------------------ 4
def test_full_mhim_window_on_half_bags_gives_the_bits_of_the_widened_window():
    """FusedTrainer(model="mhim", accumulation_steps=4) over N = 64, 97, 333, 700, fp16, D = 256: student parameters, Adam moments, the EMA
    teacher and the global queries."""
    from tests.test_ragged_window_gpu import D, ROUTE, _pair
    sizes = (64, 97, 333, 700)

    def bags_of(w):
        return ([_half_bag(500 + 10 * w + j, n, D, torch.float16)[None] for j, n in enumerate(sizes)],
                [torch.tensor([(j + w) % 2], device=DEV) for j in range(len(sizes))])

    def state(tr):
        fl = tr.flat
        return [fl.student, fl.teacher, fl.m, fl.v, tr.opt_step, tr.tick]

    def extra(tr):
        return [tr.s.merge.global_q_mm.detach(), tr.t.merge.global_q_mm.detach()] + [p.detach() for p in tr.t.parameters()]

    last = _two_windows(lambda: _pair(dropout=0.25, accum=4)[0], bags_of, state, extra)
    assert last["exec"] == ROUTE and last["x_dtype"] == torch.float16 and len(last["bags"]) == len(sizes)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_a_captured_half_call_replays_the_bits_of_the_eager_call():
    d = 256
    m = build(_state(4, d, merge_k=5), "auto", input_dim=d, **V2).eval()
    xs = [_half_bag(10, 700, d, torch.float16), _half_bag(11, 33, d, torch.float16), _half_bag(12, 161, d, torch.float16, pitch=d + 8)]
    labels = torch.tensor([1, 0, 1], device=DEV)
    eager = _call(m, xs, labels=labels)                                  # (also the first call on the device: outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = _call(m, xs, labels=labels)
    for _ in range(2):
        for t in (r.logits, r.stats, r.score, r.attn, r.z, r.loss):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        _same(r, eager)


# ------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("kind", ["merge_test", "gated"])
def test_models_outside_the_call_widen_half_bags_as_before(kind):
    if kind == "merge_test":
        model = build(synth.mhim_state(3, input_dim=256, merge_k=5), "auto", input_dim=256, merge_test=True, **V2)
    else:
        model = build(synth.mhim_state(3, input_dim=256, merge_k=5, gated=True), "auto", input_dim=256, gated=True, **V2)
    model.eval()
    xs = [_half_bag(60 + j, n, 256, torch.float16) for j, n in enumerate((45, 161, 333))]
    lg_h, at_h = model.infer_many(xs, return_attn=True)
    assert model.last["infer_native"] is False
    lg_w, at_w = model.infer_many([x.float() for x in xs], return_attn=True)
    assert model.last["infer_native"] is False
    assert torch.equal(lg_h, lg_w) and all(torch.equal(a, b) for a, b in zip(at_h, at_w))


def test_a_mixed_list_is_an_error_at_the_boundary_and_a_widening_in_the_model():
    from mhim_mil_amd import ops
    d = 256
    m = build(_state(5, d, merge_k=5), "auto", input_dim=d, **V2).eval()
    xs = [_half_bag(70, 45, d, torch.float16), _half_bag(71, 161, d, torch.bfloat16), _half_bag(72, 33, d, torch.float16).float()]
    with pytest.raises(L.MhimxError, match="mixed dtypes"):
        ops.infer_many(m._infer_cfg(), xs)
    with pytest.raises(L.MhimxError, match="row pitch"):                # 8 elements of 2 bytes: a pitch of d + 4 is refused, not read
        ops.infer_many(m._infer_cfg(), [torch.zeros((40, d + 4), dtype=torch.float16, device=DEV)[:, :d]])
    lg = m.infer_many(xs)
    assert m.last["infer_native"] is True                              # (widened: the fp32 call)
    assert torch.equal(lg, m.infer_many([x.float() for x in xs]))
    pitched = _half_bag(73, 40, d, torch.float16, pitch=d + 4)         # a half pitch the call does not take: widened, never refused
    assert torch.equal(m.infer_many([pitched]), m.infer_many([pitched.float()])) and m.last["infer_native"] is True


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "streaming"])
def test_the_feeder_delivers_half_bags_as_they_are_when_asked(resident):
    from mhim_mil_amd.feeder import BagFeeder, BagLoader
    src = [torch.from_numpy(synth.bag(80 + j, n, 256)).half() for j, n in enumerate((45, 161, 97))]
    got = [(b.clone(), int(l), i) for b, l, i in BagFeeder(src, [0, 1, 0], device=DEV, resident=resident, dtype=None)]
    torch.cuda.synchronize()
    assert [i for _, _, i in got] == [0, 1, 2] and [l for _, l, _ in got] == [0, 1, 0]
    for (b, _, i) in got:
        assert b.dtype == torch.float16 and b.shape == src[i].shape and b.stride(1) == 1
        assert torch.equal(b.cpu().view(torch.int16), src[i].view(torch.int16))          # byte for byte
    # the default is today's behaviour: fp32 bags
    for b, _, i in BagFeeder(src, [0, 1, 0], device=DEV, resident=resident):
        assert b.dtype == torch.float32 and torch.equal(b.cpu(), src[i].float())
    batch = next(iter(BagLoader(src, [0, 1, 0], device=DEV, resident=resident, dtype=None)))
    assert batch["input"].dtype == torch.float16 and batch["input"].shape == (1, 45, 256)
    torch.cuda.synchronize()
