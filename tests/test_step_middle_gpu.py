"""The student's middle of the three native train calls of the full MHIM(ABMIL) model - mhimx_step_run, mhimx_window_run (csrc/step.hip) and
mhimx_ragged_window_run (csrc/ragged_window.hip) - at the settings the other executor tests leave out: they all run attn2score=True with
aux_alpha=0.5, so the teacher's pseudo-score branch, the plain attention score, the head with and without the teacher's row are each seen
from one side only.  GPU box only.  D = 256, merge_k = 5, the V2 recipe of tests/test_window_gpu.py with dropout 0.25 on both models,
tie-free synth.bag data; N = 600 (three scorer chunks, 19 row tiles, no multiple of 32), the ragged window {64, 600, 333}.

Every expected relation was taken on the commit before the middle became one copy (csrc/step_mid.hpp); the file passes there unchanged.
What the parent does NOT satisfy bit for bit, and is therefore asserted at tests/test_ragged_window_gpu.py's bounds instead (the figures
are in profiles/step_middle_shared.md): a ragged window projects both models with pure_window_project_kernel and scores the teacher
with infer_score_kernel / rw_finalize_kernel where the single-bag step runs mhimx_bag_project and mhimx_abmil_pool_fwd, so its feature
rows, and with them score, tokens and logits, agree with the step's to rounding only (observed on the parent: score <= 7.2e-6, tokens
<= 4.6e-6, logits <= 1.8e-7 apart); its row lists ARE the step's, bit for bit.

A bag above 16 384 rows (the multi-workgroup select inside mhimx_step_run) has no case here: tests/test_round6_gpu.py::
test_step_executor_takes_whole_slide_bags[16385-512] already asserts the executor's row list equal to MHIM.student_rows' for the same
score, seed and tick, one row above the threshold."""
import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from tests.test_ragged_window_gpu import _grads_close
from tests.test_window_gpu import V2, _mk

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, KM, N1 = 256, 5, 600
RAGGED = (64, 600, 333)
SETTINGS = pytest.mark.parametrize("attn2score, aux_alpha", [(False, 0.0), (False, 0.5), (True, 0.0), (True, 0.5)])


def _trainer(attn2score, aux_alpha, accum=1):
    from mhim_mil_amd.engine import FusedTrainer
    torch.manual_seed(5)
    base = synth.mhim_state(7, input_dim=D, merge_k=KM)
    cfg = dict(V2, attn2score=attn2score, dropout=0.25)
    return FusedTrainer(_mk(base, D, **cfg), _mk(synth.spread_teacher(base), D, **cfg), aux_alpha=aux_alpha, mm=0.9997, accumulation_steps=accum)


def _bags(sizes, seed):
    return ([torch.from_numpy(synth.bag(seed + j, n, D)).to(DEV)[None] for j, n in enumerate(sizes)],
            [torch.tensor([j % 2], device=DEV) for j in range(len(sizes))])


def _equal(a, b, what):
    """Bit equality, with the figures in the message (and on stdout, for a run that only measures)."""
    a, b = a.detach().reshape(-1), b.detach().reshape(-1)
    bad = int((a != b).sum())
    worst = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
    print(f"[step_middle] {what}: {bad} of {a.numel()} elements differ, max |a - b| = {worst:.3e}")
    assert bad == 0, f"{what}: {bad} of {a.numel()} elements differ, max |a - b| = {worst:.3e}"


def _outside_projection(tr, g):
    """Every gradient view of the flat buffer but feature.0.weight / feature.0.bias (the fused dPRE image sums that pair in another
    order), as one vector.  (The views, not the buffer: it pads every tensor to 16 bytes and nobody writes the padding.)"""
    fl = tr.flat
    names = [name for name in fl.grad_views if name not in ("feature.0.weight", "feature.0.bias")]
    assert len(names) == len(fl.grad_views) - 2 and len(names) >= 10
    return torch.cat([g[fl.offsets[name]:fl.offsets[name] + fl.grad_views[name].numel()] for name in names])


def _alone(tr1, x, label, cnt, seeds, q0, tick0):
    """mhimx_step_run(update = 0) on one bag with a window's seeds, its first queries and its tick value: the bag's views, cloned."""
    from mhim_mil_amd import ops
    ex = tr1._exec_cfg()
    x2, N = x[0], x.shape[1]
    lay = ops.step_layout(ex["cfg"], N, cnt)
    ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)
    tr1.s.merge.global_q_mm.data.copy_(q0)
    tr1.tick.copy_(tick0)
    tr1.flat.grad.zero_()
    ops.step_run(ex["cfg"], x2, label, cnt, seeds, 1, ws, False)
    torch.cuda.synchronize()
    p = tr1._last_full(ws, lay, N, cnt, ops.ws_view(ws, lay.logits, 2), ops.ws_view(ws, lay.losses, 3))
    return {k: p[k].clone() for k in ("rows", "score", "tokens", "logits")}, tr1.flat.grad.clone()


def _record_seeds(tr):
    """Every seed the trainer draws from now on, in call order."""
    seen = []
    for m in (tr.s, tr.t):
        def draw(teacher=False, _orig=m._next_seed):
            seen.append(_orig(teacher=teacher))
            return seen[-1]
        m._next_seed = draw
    return seen


# ------------------------------------------------------------------------------------------------------------------ (a) the single bag
@SETTINGS
def test_step_executor_vs_python_orchestration(attn2score, aux_alpha):
    """First step of one bag, forward_backward (update = 0): logits, losses, rows, score, tokens and every gradient element behind the
    projection pair are bit-equal between mhimx_step_run and the Python orchestration (FusedTrainer._nat_prep / _nat_bag)."""
    (x,), (y,) = _bags([N1], 400)
    tr_c, tr_p = _trainer(attn2score, aux_alpha), _trainer(attn2score, aux_alpha)
    tr_p.use_executor = False
    for tr in (tr_c, tr_p):
        tr.forward_backward(x, y)
    torch.cuda.synchronize()
    assert tr_c.last["exec"] is True and tr_p.last["exec"] is False
    assert int(tr_c._exec["cfg"].attn2score) == int(attn2score) and float(tr_c._exec["cfg"].aux_alpha) == aux_alpha
    for key in ("logits", "losses", "rows", "score", "tokens"):
        _equal(tr_c.last[key], tr_p.last[key], key)
    gc, gp = tr_c.flat.grad, tr_p.flat.grad
    assert float(gc.abs().max()) > 0
    _equal(_outside_projection(tr_c, gc), _outside_projection(tr_p, gp), "gradient behind the projection pair")


# ------------------------------------------------------------------------------------------------------------------ (b) the same-shape window
@SETTINGS
def test_same_shape_window_vs_single_bag_steps(attn2score, aux_alpha):
    """A window of 2 bags of 600 rows through mhimx_window_run, update=False: each bag's rows, score, tokens and logits are bit-equal to
    mhimx_step_run(update = 0) on that bag alone with the window's seeds, first queries and tick value."""
    from mhim_mil_amd import _lib as L
    xs, ys = _bags([N1, N1], 410)
    tr, tr1 = _trainer(attn2score, aux_alpha, accum=2), _trainer(attn2score, aux_alpha)
    q0, tick0 = tr.s.merge.global_q_mm.data.clone(), tr.tick.clone()
    drawn = _record_seeds(tr)
    tr.window_step(xs, ys, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == "mhimx_window_run" and len(drawn) == 8
    (cnt, _), = tr._exec["layouts"].values()
    per = [{k: p[k].clone() for k in ("rows", "score", "tokens", "logits")} for p in tr.last["bags"]]
    for j in range(2):
        # (every bag's two dropout seeds first, then bag after bag the select's and Merge's: FusedTrainer._exec_window)
        seeds = L.StepSeeds(drop_teacher=drawn[2 * j], drop_student=drawn[2 * j + 1], select=drawn[4 + 2 * j], mca=drawn[5 + 2 * j])
        one, _ = _alone(tr1, xs[j], ys[j], cnt, seeds, q0, tick0)
        for key in ("rows", "score", "tokens", "logits"):
            _equal(per[j][key], one[key], f"bag {j} {key}")


# ------------------------------------------------------------------------------------------------------------------ (c) the ragged window
@SETTINGS
def test_ragged_window_vs_single_bag_steps(attn2score, aux_alpha):
    """A window of bags {64, 600, 333} through mhimx_ragged_window_run, update=False, against mhimx_step_run(update = 0) on each bag alone
    with the window's seeds, first queries and tick value, by the method of tests/test_ragged_window_gpu.py's per-bag comparison: the row
    lists are bit-equal; score at that file's bound for a score (atol 1e-4, rtol 2e-3), logits at its 1e-4 absolute, the tokens - like the
    logits a function of the bag's feature rows - at the same 1e-4 absolute; the window's gradient against the
    single-bag gradients summed and scaled by 1 / n at atol = rtol = 2e-3 of scale (_grads_close).
    Bag 0 overwrites, later bags add: a window of bag 0 alone leaves the same gradient bits whatever the gradient buffer held before (NaN
    here) - a one-bag window's loss scale is 1, a three-bag window's 1 / 3, so bag 0's share of the larger window has no bit-equal twin -
    and the three-bag sum above is missed by a factor if a later bag overwrote."""
    from mhim_mil_amd import ops
    xs, ys = _bags(RAGGED, 420)
    tr, tr1 = _trainer(attn2score, aux_alpha, accum=3), _trainer(attn2score, aux_alpha)
    q0, tick0 = tr.s.merge.global_q_mm.data.clone(), tr.tick.clone()
    tr.window_step(xs, ys, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == "mhimx_ragged_window_run"
    table, n = tr.last["table"], len(RAGGED)
    per = [{k: p[k].clone() for k in ("rows", "score", "tokens", "logits")} for p in tr.last["bags"]]
    g_win = tr.flat.grad.clone()
    ones = [_alone(tr1, xs[j], ys[j], table[j].cnt, table[j].seeds, q0, tick0) for j in range(n)]
    for j in range(n):
        one = ones[j][0]
        for key in ("score", "tokens", "logits"):
            d = (per[j][key].double() - one[key].double()).abs()
            print(f"[step_middle] ragged bag {j} {key}: {int((per[j][key] != one[key]).sum())} of {d.numel()} differ, max |a - b| = {float(d.max()):.3e}")
        _equal(per[j]["rows"], one["rows"], f"ragged bag {j} rows")
        np.testing.assert_allclose(per[j]["score"].cpu().numpy(), one["score"].cpu().numpy(), atol=1e-4, rtol=2e-3, err_msg=f"score of bag {j}")
        np.testing.assert_allclose(per[j]["tokens"].cpu().numpy(), one["tokens"].cpu().numpy(), atol=1e-4, rtol=0, err_msg=f"tokens of bag {j}")
        np.testing.assert_allclose(per[j]["logits"].cpu().numpy(), one["logits"].cpu().numpy(), atol=1e-4, rtol=0, err_msg=f"logits of bag {j}")
    fl = tr.flat
    g_sum = sum(o[1].double() for o in ones) / n
    cut = lambda g: {name: g[fl.offsets[name]:fl.offsets[name] + v.numel()] for name, v in fl.grad_views.items()}
    _grads_close(cut(g_win), {name: v.float().cpu() for name, v in cut(g_sum).items()})
    # bag 0 alone, as a window of one: over a zeroed gradient buffer and over one full of NaN
    ex = tr._exec_cfg()
    lay = ops.ragged_window(ex["cfg"], table, 1, layout_only=True)
    got = []
    for fill in (0.0, float("nan")):
        tr.s.merge.global_q_mm.data.copy_(q0)
        tr.tick.copy_(tick0)
        fl.grad.fill_(fill)
        ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)
        ops.ragged_window(ex["cfg"], table, 1, 1, ws, update=False)
        torch.cuda.synchronize()
        got.append(fl.grad.clone())
    assert bool(torch.isfinite(_outside_projection(tr, got[1])).all()), "bag 0 added to what the gradient buffer held"
    _equal(_outside_projection(tr, got[0]), _outside_projection(tr, got[1]), "gradient of bag 0 alone, zeroed buffer against NaN buffer")
    fl.grad.zero_()
