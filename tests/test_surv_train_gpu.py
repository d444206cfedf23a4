"""Survival training in the native train calls - GPU box only: mhimx_head_surv_fwd_bwd, mhimx_pure_window_run_surv,
mhimx_ragged_window_run_surv, FusedTrainer(loss="nll_surv") and CommonMIL.forward_func's survival branch.

Shapes: E = 512, C = 4 time bins (the reference's n_bins), D = 256; teacher-free bags of N in {1, 31, 33, 65} (one row, one short of a
32-row tile, one past it, a third tile), full-model bags of N in {64, 97, 130} (the minimum, no multiple of 32, a fifth tile), merge_k = 5.
Tolerances are the ones the classification windows are held to (tests/test_pure_window_gpu.py, tests/test_ragged_window_gpu.py): logits
1e-4 absolute, every gradient atol = 2e-3 max|ref|, rtol = 2e-3, parameters after Adam mean <= 3e-6 and max <= 4.1e-4; everything the
issue states as bit-equal is compared with torch.equal."""
import types

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O
from tests import surv_oracle as SO
from tests import test_pure_window_gpu as PWG
from tests.test_single_pass_gpu import _draws_from_device
from tests.test_window_gpu import V2, _check_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, K, E = 256, 4, 512
PURE_SIZES = (1, 31, 33, 65)
FULL_SIZES = (64, 97, 130)
EPS = 1e-7


def _ops():
    from mhim_mil_amd import ops
    return ops


def _f32(*vals):
    """the fp32 product of python floats, as the kernels take main_alpha * inv_accum"""
    p = np.float32(1.0)
    for v in vals:
        p = np.float32(p * np.float32(v))
    return float(p)


def _bits(a, b):
    """bit-equal, NaN patterns included"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _pairs(Ys, cs):
    return [(torch.tensor([y], device=DEV), torch.tensor([float(c)], device=DEV)) for y, c in zip(Ys, cs)]


# ------------------------------------------------------------------------------------------------ models and trainers
def _pure_model(dropout=0.25, **kw):
    from mhim_mil_amd.mhim import MHIM
    m = MHIM(input_dim=D, n_classes=K, baseline="attn", dropout=dropout, act="gelu", da_act="relu", merge_enable=False, **kw)
    sd = synth.mhim_state(7, input_dim=D, n_classes=K, merge_enable=False)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(DEV).train()


def _pure_trainer(accum=4, dropout=0.25, loss="nll_surv", surv_alpha=0.4, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    extra = {} if loss is None else dict(loss=loss, surv_alpha=surv_alpha)
    return FusedTrainer(_pure_model(dropout), None, lr=2e-4, model="mhim_pure", accumulation_steps=accum, **extra, **kw)


def _full_pair(accum=3, dropout=0.0, loss="nll_surv", surv_alpha=0.4, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    torch.manual_seed(5)
    base = synth.mhim_state(7, input_dim=D, n_classes=K, merge_k=5)
    tsd = synth.spread_teacher(base)
    cfg = dict(V2, dropout=dropout)
    models = []
    for sd in (base, tsd):
        m = MHIM(input_dim=D, n_classes=K, baseline="attn", **cfg)
        sd = dict(sd)
        sd["merge.global_q"] = sd["merge.global_q_mm"]
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        m = m.to(DEV).train()
        m.merge.dropout = 0.0
        models.append(m)
    extra = {} if loss is None else dict(loss=loss, surv_alpha=surv_alpha)
    return FusedTrainer(models[0], models[1], aux_alpha=0.5, mm=0.9997, accumulation_steps=accum, **extra, **kw), models[0], models[1], base, tsd


def _pure_bags(sizes=PURE_SIZES, seed=300):
    return [torch.from_numpy(synth.bag(seed + j, n, D)) for j, n in enumerate(sizes)]


def _grads_close(tr, ref, what=""):
    for name, r in ref.items():
        g = tr.flat.grad_views[name].cpu().numpy()
        r = (r.detach() if torch.is_tensor(r) else torch.as_tensor(r)).double().numpy().reshape(g.shape)
        print(f"  {what} grad {name}: max err {np.abs(g - r).max():.3e} of scale {np.abs(r).max():.3e}")
        np.testing.assert_allclose(g, r, atol=2e-3 * (np.abs(r).max() + 1e-30), rtol=2e-3, err_msg=name)


# ------------------------------------------------------------------------------------------------ 1. the head building block
def _head_inputs(C, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    z = torch.randn(E, generator=g).to(DEV)
    t = torch.randn(E, generator=g).to(DEV)
    wp = (0.05 * torch.randn(C, E, generator=g)).to(DEV)
    bp = (0.3 * torch.randn(C, generator=g)).to(DEV)
    return z, t, wp, bp


@pytest.mark.parametrize("teacher", [False, True])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_head_is_the_two_launch_composition_bit_for_bit(C, teacher):
    """logits = mhimx_head_fwd_bwd's; nll and risk = mhimx_surv_nll's on them; g_z, d_wp, d_bp = those of mhimx_surv_nll(g_scale =
    main_alpha / accum) followed by mhimx_head_fwd_bwd's autograd form - all bit for bit: the survival form is the same kernel text around
    the same device function."""
    ops = _ops()
    z, t, wp, bp = _head_inputs(C)
    t_in = t if teacher else None
    kw = dict(temp_t=0.1, main_alpha=0.7, aux_alpha=0.5, inv_accum=1.0 / 3.0)
    lg_ce = ops.head_fwd_bwd(z, t_in, wp, bp, torch.tensor([0], device=DEV), **kw)[0]
    for cens in (0.0, 1.0):
        for y in sorted({0, C - 1}):
            for alpha in (0.0, 0.4):
                Y, c = torch.tensor([y], device=DEV), torch.tensor([cens], device=DEV)
                logits, losses, risk, g_z, d_wp, d_bp = ops.head_surv_fwd_bwd(z, t_in, wp, bp, Y, c, surv_alpha=alpha, surv_eps=EPS, **kw)
                assert _bits(logits, lg_ce)
                r_ref, l_ref, g = ops.surv_nll(logits.view(1, C), Y, c, alpha=alpha, eps=EPS, g_scale=_f32(0.7, 1.0 / 3.0))
                assert _bits(losses[1:2], l_ref) and _bits(risk, r_ref), (C, teacher, cens, y, alpha)
                lg2, ls2, g_z2, d_wp2, d_bp2 = ops.head_fwd_bwd(z, t_in, wp, bp, None, g_logits_in=g.view(-1), **kw)
                assert _bits(lg2, logits) and _bits(ls2[2:3], losses[2:3])
                for a, b, what in ((g_z, g_z2, "g_z"), (d_wp, d_wp2, "d_wp"), (d_bp, d_bp2, "d_bp")):
                    assert _bits(a, b), (what, C, teacher, cens, y, alpha, float((a - b).abs().max()))
                assert float(d_bp.abs().max()) > 0 and torch.isfinite(g_z).all()
                want = 0.7 * float(losses[1]) + 0.5 * float(losses[2])
                assert abs(float(losses[0]) - want) <= 1e-6 * max(1.0, abs(want))
                assert (float(losses[2]) != 0.0) == teacher


def test_head_clamps_accumulate_and_a_bin_out_of_range():
    ops = _ops()
    C = 4
    z, t, wp, bp = _head_inputs(C, seed=1)
    zero_w = torch.zeros_like(wp)
    # a censored row whose survival value underflows eps; an uncensored row in bin 0 whose hazard underflows eps: zero gradient rows
    for fill, y, cens, want in ((40.0, C - 1, 1.0, -(1 - 0.4) * np.log(EPS)), (-40.0, 0, 0.0, -np.log(EPS))):
        b40 = torch.full((C,), fill, device=DEV)
        Y, c = torch.tensor([y], device=DEV), torch.tensor([cens], device=DEV)
        logits, losses, risk, g_z, d_wp, d_bp = ops.head_surv_fwd_bwd(z, None, zero_w, b40, Y, c, surv_alpha=0.4, surv_eps=EPS)
        assert (logits == fill).all() and abs(float(losses[1]) - want) < 1e-5
        assert (d_bp == 0).all() and (d_wp == 0).all() and (g_z == 0).all()
        _, l_ref, g = ops.surv_nll(logits.view(1, C), Y, c, alpha=0.4, eps=EPS, g_scale=1.0)
        assert (g == 0).all() and _bits(losses[1:2], l_ref)
    # accumulate = 1 adds to d_wp / d_bp (one fp32 addition per element)
    Y, c = torch.tensor([2], device=DEV), torch.tensor([0.0], device=DEV)
    _, _, _, g_z0, d_wp0, d_bp0 = ops.head_surv_fwd_bwd(z, t, wp, bp, Y, c, surv_alpha=0.4, aux_alpha=0.5, temp_t=0.1)
    pre_w, pre_b = torch.randn_like(wp), torch.randn_like(bp)
    acc_w, acc_b = pre_w.clone(), pre_b.clone()
    _, _, _, g_z1, _, _ = ops.head_surv_fwd_bwd(z, t, wp, bp, Y, c, surv_alpha=0.4, aux_alpha=0.5, temp_t=0.1, d_wp=acc_w, d_bp=acc_b, accumulate=True)
    assert _bits(acc_w, pre_w + d_wp0) and _bits(acc_b, pre_b + d_bp0) and _bits(g_z0, g_z1)
    # a bin outside [0, C): NaN loss, zero survival gradient, the risk still written
    for y in (-1, C):
        out = ops.head_surv_fwd_bwd(z, None, wp, bp, torch.tensor([y], device=DEV), c, surv_alpha=0.4)
        assert torch.isnan(out[1][1]) and torch.isnan(out[1][0]) and (out[5] == 0).all() and (out[4] == 0).all() and torch.isfinite(out[2]).all()
    # the generic head (C > 4) runs the same row: against mhimx_surv_nll on its logits
    z, t, wp, bp = _head_inputs(16, seed=2)
    Y, c = torch.tensor([9], device=DEV), torch.tensor([1.0], device=DEV)
    logits, losses, risk, g_z, d_wp, d_bp = ops.head_surv_fwd_bwd(z, t, wp, bp, Y, c, surv_alpha=0.4, aux_alpha=0.5, temp_t=0.1, inv_accum=0.5)
    r_ref, l_ref, g = ops.surv_nll(logits.view(1, 16), Y, c, alpha=0.4, eps=EPS, g_scale=0.5)
    assert _bits(losses[1:2], l_ref) and _bits(risk, r_ref) and _bits(d_bp, g.view(-1))
    _, _, g_z2, d_wp2, _ = ops.head_fwd_bwd(z, t, wp, bp, None, g_logits_in=g.view(-1), aux_alpha=0.5, temp_t=0.1, inv_accum=0.5)
    assert _bits(g_z, g_z2) and _bits(d_wp, d_wp2)
    # E = 1000 (no multiple of 256), C = 3: the four-elements-per-thread form of the short-chain head
    gen = torch.Generator().manual_seed(9)
    z, t = torch.randn(1000, generator=gen).to(DEV), torch.randn(1000, generator=gen).to(DEV)
    wp, bp = (0.05 * torch.randn(3, 1000, generator=gen)).to(DEV), (0.3 * torch.randn(3, generator=gen)).to(DEV)
    Y, c = torch.tensor([1], device=DEV), torch.tensor([0.0], device=DEV)
    logits, losses, risk, g_z, d_wp, d_bp = ops.head_surv_fwd_bwd(z, t, wp, bp, Y, c, surv_alpha=0.4, aux_alpha=0.5, temp_t=0.1)
    r_ref, l_ref, g = ops.surv_nll(logits.view(1, 3), Y, c, alpha=0.4, eps=EPS, g_scale=1.0)
    lg2, _, g_z2, d_wp2, d_bp2 = ops.head_fwd_bwd(z, t, wp, bp, None, g_logits_in=g.view(-1), aux_alpha=0.5, temp_t=0.1)
    assert _bits(losses[1:2], l_ref) and _bits(risk, r_ref) and _bits(logits, lg2) and _bits(g_z, g_z2) and _bits(d_wp, d_wp2) and _bits(d_bp, d_bp2)


# ------------------------------------------------------------------------------------------------ direct calls
def _run_pure(tr, xs, pairs, seeds, tick, update=False, surv=True, host_step=1):
    """mhimx_pure_window_run_surv (surv False: mhimx_pure_window_run_x) on a NaN-filled workspace at the given tick value."""
    ops = _ops()
    n = len(xs)
    ex = tr._exec_cfg()
    table = ops.pure_window_bags(xs, [p[0] for p in pairs], seeds)
    lay = ops.pure_window_layout(ex["cfg"], table, n)
    ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)
    risk = torch.full((n,), float("nan"), device=DEV)
    spec = ops.surv_spec([p[1] for p in pairs], tr.surv_alpha, tr.surv_eps, risk) if surv else None
    tr.tick.fill_(tick)
    ops.pure_window_run(ex["cfg"], table, n, host_step, ws, update, surv=spec)
    torch.cuda.synchronize()
    v = ops.ws_view
    out = dict(lay=lay, ws=ws, risk=risk, logits=v(ws, lay.logits, n * K).view(n, K), losses=v(ws, lay.losses, n * 3).view(n, 3),
               H=v(ws, lay.H, lay.rows * E).view(lay.rows, E), s=v(ws, lay.s, lay.rows), stats=v(ws, lay.stats, 2 * n), z=v(ws, lay.z, n * E).view(n, E),
               dact=v(ws, lay.dact, lay.rows * E, torch.float16).view(lay.rows, E), row0=[int(lay.row0[j]) for j in range(n)])
    return out


def _run_full(tr, s, xs, pairs, seeds, tick, update=False, surv=True, host_step=1, q0=None):
    """mhimx_ragged_window_run_surv (surv False: mhimx_ragged_window_run_x) on a NaN-filled workspace at the given tick value."""
    from mhim_mil_amd import _lib as L
    ops = _ops()
    n = len(xs)
    ex = tr._exec_cfg()
    table = (L.RaggedWindowBag * n)()
    for j, x in enumerate(xs):
        table[j].X, table[j].ldx, table[j].N, table[j].label_dev = x.data_ptr(), x.stride(0), x.shape[0], pairs[j][0].data_ptr()
        table[j].cnt = L.StepCounts(*s.v2_counts(x.shape[0], None))
        table[j].seeds = seeds[j]
    lay = ops.ragged_window(ex["cfg"], table, n, layout_only=True)
    ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)
    risk = torch.full((n,), float("nan"), device=DEV)
    spec = ops.surv_spec([p[1] for p in pairs], tr.surv_alpha, tr.surv_eps, risk) if surv else None
    tr.tick.fill_(tick)
    if q0 is not None:
        s.merge.global_q_mm.data.copy_(q0)
    ops.ragged_window(ex["cfg"], table, n, host_step, ws, update=update, surv=spec)
    torch.cuda.synchronize()
    v = ops.ws_view
    per = []
    for j, x in enumerate(xs):
        r0, N, cnt = int(lay.row0[j]), x.shape[0], table[j].cnt
        per.append(dict(score=v(ws, lay.score, lay.rows)[r0:r0 + N], rows_all=v(ws, lay.rows_all, lay.rows, torch.int64)[r0:r0 + cnt.len_keep + 5],
                        H_teacher=v(ws, lay.H_teacher, lay.rows * E).view(-1, E)[r0:r0 + N],
                        H_student=v(ws, lay.H_student, lay.rows * E).view(-1, E)[r0:r0 + N + 5],
                        z_teacher=v(ws, lay.z_teacher, n * E).view(n, E)[j], z_student=v(ws, lay.z_student, n * E).view(n, E)[j],
                        logits=v(ws, lay.logits, n * 16).view(n, 16)[j, :K], losses=v(ws, lay.losses, n * 4).view(n, 4)[j, :3]))
    return dict(lay=lay, ws=ws, risk=risk, bags=per, table=table)


def _full_seeds(n, base=11):
    from mhim_mil_amd import _lib as L
    return [L.StepSeeds(base + 10 * j, base + 1 + 10 * j, base + 2 + 10 * j, base + 3 + 10 * j) for j in range(n)]


# ------------------------------------------------------------------------------------------------ 2. the forward is the classification call's
def test_pure_forward_is_the_classification_calls_and_the_head_is_surv_nlls():
    tr = _pure_trainer()
    xs = [b.to(DEV) for b in _pure_bags()]
    pairs = _pairs([0, 3, 1, 2], [0, 1, 1, 0])
    seeds = [21, 22, 23, 24]
    a = _run_pure(tr, xs, pairs, seeds, tick=3, surv=True)
    b = _run_pure(tr, xs, pairs, seeds, tick=3, surv=False)
    for name in ("H", "s", "stats", "z", "logits"):
        assert _bits(a[name], b[name]), name
    assert torch.isfinite(a["logits"]).all() and 0.7 < float((a["H"][a["row0"][3]:a["row0"][3] + 65] != 0).float().mean()) < 0.8
    Y, c = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    risk, nll = _ops().surv_nll(a["logits"], Y, c, alpha=tr.surv_alpha, eps=EPS)
    assert _bits(a["losses"][:, 1], nll) and _bits(a["risk"], risk)
    assert _bits(a["losses"][:, 0], nll * float(tr.main_alpha)) and (a["losses"][:, 2] == 0).all()
    assert not _bits(a["losses"][:, 1], b["losses"][:, 1])


def test_full_forward_is_the_classification_calls_and_the_head_is_surv_nlls():
    tr, s, t, _, _ = _full_pair(dropout=0.25)
    xs = [torch.from_numpy(synth.bag(400 + j, n, D)).to(DEV) for j, n in enumerate(FULL_SIZES)]
    pairs = _pairs([3, 0, 2], [1, 0, 0])
    seeds = _full_seeds(3)
    q0 = s.merge.global_q_mm.data.clone()
    a = _run_full(tr, s, xs, pairs, seeds, tick=3, surv=True, q0=q0)
    b = _run_full(tr, s, xs, pairs, seeds, tick=3, surv=False, q0=q0)
    for j in range(3):
        for name in ("score", "rows_all", "H_teacher", "H_student", "z_teacher", "z_student", "logits"):
            assert _bits(a["bags"][j][name], b["bags"][j][name]), (j, name)
        assert _bits(a["bags"][j]["losses"][2:3], b["bags"][j]["losses"][2:3])              # the distillation term is untouched
    logits = torch.stack([p["logits"] for p in a["bags"]])
    losses = torch.stack([p["losses"] for p in a["bags"]])
    Y, c = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    risk, nll = _ops().surv_nll(logits, Y, c, alpha=tr.surv_alpha, eps=EPS)
    assert _bits(losses[:, 1].contiguous(), nll) and _bits(a["risk"], risk) and torch.isfinite(losses).all()
    want = float(tr.main_alpha) * nll.double() + float(tr.aux_alpha) * losses[:, 2].double()
    assert float((losses[:, 0].double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert float(losses[:, 2].abs().min()) > 0


# ------------------------------------------------------------------------------------------------ 3. gradients against the fp64 restatement
def _pure_restatement(bags, Ys, cs, params, dropout, masks, main_alpha, alpha):
    """The oracle's model math (O.pure) in fp64 with surv_oracle's loss: per bag (main_alpha NLLSurv / n).backward() into shared leaves."""
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    cfg = O.Cfg(dropout=dropout, **PWG.CFG)
    n = len(bags)
    logits, nlls, risks = [], [], []
    for j, x in enumerate(bags):
        lo = O.pure(x.double(), po, cfg, drop_mask=None if masks is None else masks[j])
        risk, nll = SO.nll_surv(lo.view(1, -1), torch.tensor([Ys[j]]), torch.tensor([float(cs[j])], dtype=torch.float64), alpha=alpha, eps=EPS)
        (main_alpha * nll[0] / n).backward()
        logits.append(lo.detach()); nlls.append(float(nll[0].detach())); risks.append(float(risk[0].detach()))
    return po, logits, nlls, risks


def test_pure_window_gradients_and_the_update_against_the_fp64_restatement():
    bags = _pure_bags()
    Ys, cs = [0, 3, 1, 2], [0, 1, 1, 0]                            # censored and uncensored bags in one window
    xs, pairs = [b.to(DEV) for b in bags], _pairs(Ys, cs)
    base = O.as_torch(synth.mhim_state(7, input_dim=D, n_classes=K, merge_enable=False))
    res = {}
    for update in (False, True):
        tr = _pure_trainer(accum=4, dropout=0.25)
        logits, losses = tr.window_step(xs, pairs, update=update)
        torch.cuda.synchronize()
        assert tr.last["exec"] == "mhimx_pure_window_run_surv" and tr.last["risk"].shape == (4,)
        assert int(tr.tick) == 1 and int(tr.opt_step) == 1 and tr.flat.step == int(update)
        masks = [(b["H_student"] != 0).cpu() for b in tr.last["bags"]]
        res[update] = (tr, [l.clone() for l in logits], [l.clone() for l in losses], masks, tr.last["risk"].clone())
    for m0, m1 in zip(res[False][3], res[True][3]):
        assert torch.equal(m0, m1)                                  # same seeds, same tick: the same keep-masks
    tr, logits, losses, masks, risk = res[False]
    po, ref_logits, ref_nll, ref_risk = _pure_restatement(bags, Ys, cs, base, 0.25, masks, tr.main_alpha, tr.surv_alpha)
    for j in range(4):
        np.testing.assert_allclose(logits[j].cpu().numpy(), ref_logits[j].numpy(), atol=1e-4, rtol=0)
        assert abs(float(losses[j][1]) - ref_nll[j]) < 3e-4 and abs(float(risk[j]) - ref_risk[j]) < 3e-4
    _grads_close(tr, {k: p.grad for k, p in po.items()}, "pure")
    stu, opt = PWG._adam({k: _with_grad(p) for k, p in po.items()}, {}, 1)
    PWG._check_after_adam(res[True][0], stu, opt, 0)


def _with_grad(p):
    """an fp32 leaf carrying the fp64 leaf's gradient (O.adam_step runs in the dtype it is given: fp32, as the existing files do)"""
    q = p.detach().float()
    q.grad = p.grad.float()
    return q


def _surv_ce(pairs_cpu, alpha):
    """O.cross_entropy's place inside O.train_window: label j is bag j's (Y, c) pair, the criterion surv_oracle's"""
    def loss(logits, j):
        Y, c = pairs_cpu[j]
        return SO.nll_surv(logits.view(1, -1), torch.tensor([Y]), torch.tensor([float(c)], dtype=logits.dtype), alpha=alpha, eps=EPS)[1][0]
    return loss


def test_full_window_gradients_and_the_update_against_the_restatement(monkeypatch):
    """The oracle's window step (O.train_window, q_ema="window", the draws derived from the call's own rows and teacher score - the
    method of tests/test_ragged_window_gpu.py::test_two_ragged_windows_vs_oracle) with surv_oracle's loss where it takes the cross
    entropy; aux_alpha = 0.5; a censored and two uncensored bags."""
    Ys, cs = [3, 0, 2], [1, 0, 0]
    bags = [torch.from_numpy(synth.bag(500 + j, n, D)) for j, n in enumerate(FULL_SIZES)]
    xs, pairs = [b.to(DEV)[None] for b in bags], _pairs(Ys, cs)
    out = {}
    for update in (False, True):
        tr, s, t, base, tsd = _full_pair(accum=3)
        tr.window_step(xs, pairs, update=update)
        torch.cuda.synchronize()
        assert tr.last["exec"] == "mhimx_ragged_window_run_surv" and tr.last["risk"].shape == (3,)
        assert int(tr.tick) == 1 and int(tr.opt_step) == 1 and tr.flat.step == int(update)
        out[update] = (tr, s, t, base, tsd)
    tr, s, t, base, tsd = out[False]
    per = tr.last["bags"]
    perms, shufs, scores = [], [], []
    for j, n in enumerate(FULL_SIZES):
        k, n_sel, _ = O.mask_count(n, 0.03, 0.5)
        rows, score = per[j]["rows"].cpu().numpy(), per[j]["score"].cpu().numpy()
        p, sh = _draws_from_device(score, rows, per[j]["R"], n, k, n_sel)
        perms.append(p); shufs.append(sh); scores.append(torch.from_numpy(score))
    for j in range(3):                                             # both runs drew the same rows
        assert torch.equal(per[j]["rows"], out[True][0].last["bags"][j]["rows"])
    monkeypatch.setattr(O, "cross_entropy", _surv_ce(list(zip(Ys, cs)), tr.surv_alpha))
    stu, tea, opt, info = O.train_window([x.double() for x in bags], [0, 1, 2], O.as_torch(base, torch.float64), O.as_torch(tsd, torch.float64), {},
                                         O.Cfg(**V2), 1, perms=perms, shuffles=shufs, q_ema="window", score_overrides=scores, mm=tr.mm)    # fp64
    for j in range(3):
        np.testing.assert_allclose(per[j]["logits"].cpu().numpy().ravel(), info["logits"][j].numpy().ravel(), atol=1e-4, rtol=0)
        assert abs(float(per[j]["losses"][0]) - info["loss"][j]) < 3e-4
    _grads_close(tr, info["grads"], "full")
    _, s1, t1, _, _ = out[True]
    _check_params(s1, stu, 3e-6, 4.1e-4, "student after the update inside the call")
    _check_params(t1, tea, 1e-6, 2e-6, "teacher after the update inside the call")
    np.testing.assert_allclose(s1.merge.global_q_mm.detach().cpu().numpy(), stu["merge.global_q_mm"].numpy(), atol=2e-6, rtol=0)


# ------------------------------------------------------------------------------------------------ 4. windows and single bags agree
def _sum_of_singles(run_one, n, tr):
    ref = torch.zeros_like(tr.flat.grad, dtype=torch.float64)
    for j in range(n):
        tr.flat.grad.zero_()
        run_one(j)
        ref += tr.flat.grad.double()
    return (ref / n).float()


def _flat_close(tr, got, ref):
    for name, v in tr.flat.grad_views.items():
        o, cnt = tr.flat.offsets[name], v.numel()
        a, r = got[o:o + cnt].cpu().numpy(), ref[o:o + cnt].cpu().numpy()
        np.testing.assert_allclose(a, r, atol=2e-3 * (np.abs(r).max() + 1e-30), rtol=2e-3, err_msg=name)


def test_a_window_is_the_sum_of_its_windows_of_one_and_neighbours_do_not_matter():
    # ---- teacher-free
    tr = _pure_trainer(accum=3)
    xs = [b.to(DEV) for b in _pure_bags((33, 65, 31), seed=600)]
    pairs, seeds = _pairs([1, 3, 0], [0, 1, 0]), [31, 32, 33]
    w = _run_pure(tr, xs, pairs, seeds, tick=5)
    g3 = tr.flat.grad.clone()
    assert float(g3.abs().max()) > 0
    ref = _sum_of_singles(lambda j: _run_pure(tr, xs[j:j + 1], pairs[j:j + 1], seeds[j:j + 1], tick=5), 3, tr)
    _flat_close(tr, g3, ref)
    order = [2, 0, 1]
    w2 = _run_pure(tr, [xs[j] for j in order], [pairs[j] for j in order], [seeds[j] for j in order], tick=5)
    one = _run_pure(tr, xs[1:2], pairs[1:2], seeds[1:2], tick=5)
    r0, r2, N = w["row0"][1], w2["row0"][2], 65
    for a, b, c_, what in ((w["H"][r0:r0 + N], w2["H"][r2:r2 + N], one["H"][:N], "H"), (w["dact"][r0:r0 + N], w2["dact"][r2:r2 + N], one["dact"][:N], "dact"),
                           (w["logits"][1], w2["logits"][2], one["logits"][0], "logits"), (w["losses"][1], w2["losses"][2], one["losses"][0], "losses"),
                           (w["risk"][1:2], w2["risk"][2:3], one["risk"][:1], "risk"), (w["z"][1], w2["z"][2], one["z"][0], "z")):
        assert _bits(a, b) and _bits(a, c_), what
    # ---- the full model
    tr, s, t, _, _ = _full_pair(accum=3, dropout=0.25)
    xs = [torch.from_numpy(synth.bag(700 + j, n, D)).to(DEV) for j, n in enumerate(FULL_SIZES)]
    pairs, seeds = _pairs([2, 0, 3], [0, 0, 1]), _full_seeds(3)
    q0 = s.merge.global_q_mm.data.clone()
    w = _run_full(tr, s, xs, pairs, seeds, tick=5, q0=q0)
    g3 = tr.flat.grad.clone()
    ref = _sum_of_singles(lambda j: _run_full(tr, s, xs[j:j + 1], pairs[j:j + 1], seeds[j:j + 1], tick=5, q0=q0), 3, tr)
    _flat_close(tr, g3, ref)
    w2 = _run_full(tr, s, [xs[j] for j in order], [pairs[j] for j in order], [seeds[j] for j in order], tick=5, q0=q0)
    one = _run_full(tr, s, xs[1:2], pairs[1:2], seeds[1:2], tick=5, q0=q0)
    for name in ("score", "rows_all", "H_student", "z_student", "logits", "losses"):
        assert _bits(w["bags"][1][name], w2["bags"][2][name]) and _bits(w["bags"][1][name], one["bags"][0][name]), name
    assert _bits(w["risk"][1:2], w2["risk"][2:3]) and _bits(w["risk"][1:2], one["risk"][:1])


# ------------------------------------------------------------------------------------------------ 5. determinism and capture
def test_two_runs_give_the_same_bytes_and_a_captured_window_replays_the_eager_call():
    xs = [b.to(DEV) for b in _pure_bags(seed=800)]
    pairs = _pairs([2, 0, 3, 1], [1, 0, 0, 1])
    grads = []
    for _ in range(2):
        tr = _pure_trainer()
        tr.window_step(xs, pairs, update=False)
        torch.cuda.synchronize()
        grads.append((tr.flat.grad.clone(), tr.last["risk"].clone(), tr.last["ws"][:tr.last["layout"].total].clone()))
    assert all(_bits(a, b) for a, b in zip(grads[0][:2], grads[1][:2])) and float(grads[0][0].abs().max()) > 0
    tr_g, tr_e = _pure_trainer(), _pure_trainer()
    snap = PWG._state(tr_g)
    graph = tr_g.capture_window(xs, pairs, warmup=1)
    seed_step = tr_g.s._step
    assert tr_g.last["exec"] == "mhimx_pure_window_run_surv"
    fl = tr_g.flat
    fl.student.copy_(snap[0]); fl.m.copy_(snap[1]); fl.v.copy_(snap[2]); tr_g.opt_step.copy_(snap[3]); tr_g.tick.copy_(snap[4])
    fl.grad.zero_()
    tr_g.last["ws"].fill_(255)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for _ in range(3):
        tr_e.s._step = seed_step - len(xs)                          # (the seeds the capture baked; the tick moves on by itself)
        le, se = tr_e.window_step(xs, pairs)
        assert tr_e.last["exec"] == "mhimx_pure_window_run_surv"
    torch.cuda.synchronize()
    for j in range(len(xs)):
        assert _bits(tr_g.last["logits"][j], le[j]) and _bits(tr_g.last["losses"][j], se[j])
    assert _bits(tr_g.last["risk"], tr_e.last["risk"])
    for name, a, b in zip(("student", "m", "v", "opt_step", "tick"), PWG._state(tr_g), PWG._state(tr_e)):
        assert torch.equal(a, b), name
    assert int(tr_e.tick) == 3 and int(tr_e.opt_step) == 3 and torch.isfinite(tr_g.flat.student).all()


def test_the_full_models_captured_window_replays_the_eager_windows():
    from tests.test_ragged_window_gpu import _restore, _same_bits, _state
    ops = _ops()
    xs = [torch.from_numpy(synth.bag(900 + j, n, D)).to(DEV)[None] for j, n in enumerate(FULL_SIZES)]
    pairs = _pairs([1, 3, 0], [0, 1, 1])
    tr_g, *_ = _full_pair(dropout=0.25)
    snap = _state(tr_g)
    g = tr_g.capture_window(xs, pairs, warmup=1)
    assert tr_g.last["exec"] == "mhimx_ragged_window_run_surv"
    table, n = tr_g.last["table"], 3
    _restore(tr_g, snap)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    replayed, risk_g = _state(tr_g), tr_g.last["risk"].clone()
    runs = []
    for _ in range(2):
        tr_e, *_ = _full_pair(dropout=0.25)
        assert _same_bits(_state(tr_e), snap)
        ex = tr_e._exec_cfg()
        lay = ops.ragged_window(ex["cfg"], table, n, layout_only=True)
        ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)
        risk = torch.empty(n, device=DEV)
        spec = ops.surv_spec([p[1] for p in pairs], tr_e.surv_alpha, tr_e.surv_eps, risk)
        for w in range(3):
            ops.ragged_window(ex["cfg"], table, n, w + 1, ws, update=True, surv=spec)
        torch.cuda.synchronize()
        runs.append((_state(tr_e), risk.clone()))
        assert int(tr_e.tick) == 3 and int(tr_e.opt_step) == 3 and torch.isfinite(tr_e.flat.student).all()
    assert _same_bits(runs[0][0], runs[1][0]) and _bits(runs[0][1], runs[1][1]), "two eager runs differ"
    assert not torch.equal(runs[0][0][0], snap[0])
    assert _same_bits(runs[0][0], replayed) and _bits(runs[0][1], risk_g), "three replays differ from three eager windows"


# ------------------------------------------------------------------------------------------------ 6. trainer and loop
def test_trainer_routes_report_the_new_calls():
    xs = [b.to(DEV) for b in _pure_bags(seed=1000)]
    pairs = _pairs([2, 0, 3, 1], [1, 0, 0, 1])
    tr = _pure_trainer(accum=4)
    tr.window_step(xs, pairs)
    assert tr.last["exec"] == "mhimx_pure_window_run_surv" and tr.flat.step == 1 and tr.last["risk"].shape == (4,)
    tr.window_step(xs[:2], pairs[:2])                               # a shorter last window
    assert tr.last["exec"] == "mhimx_pure_window_run_surv" and tr.flat.step == 2 and tr.last["risk"].shape == (2,)
    one = _pure_trainer(accum=1)
    one.train_step(xs[3], pairs[3])
    assert one.last["exec"] == "mhimx_pure_window_run_surv" and one.flat.step == 1 and int(one.opt_step) == 1 and one._micro == 0
    one.forward_backward(xs[2], pairs[2])
    assert one.last["exec"] == "mhimx_pure_window_run_surv" and one.flat.step == 1 and one._micro == 1
    one.update()
    assert one.flat.step == 2 and int(one.opt_step) == 2 and int(one.tick) == 2
    fx = [torch.from_numpy(synth.bag(1100 + j, n, D)).to(DEV)[None] for j, n in enumerate(FULL_SIZES)]
    fp = _pairs([1, 3, 0], [0, 1, 1])
    tr, *_ = _full_pair(accum=3)
    tr.window_step(fx, fp)
    assert tr.last["exec"] == "mhimx_ragged_window_run_surv" and tr.flat.step == 1 and tr.last["risk"].shape == (3,)
    same = [torch.from_numpy(synth.bag(1200 + j, 97, D)).to(DEV)[None] for j in range(3)]
    tr.window_step(same, fp)                                        # same-shaped bags: the ragged call too (mhimx_window_run has no survival form)
    assert tr.last["exec"] == "mhimx_ragged_window_run_surv" and tr.flat.step == 2
    one, *_ = _full_pair(accum=1)
    one.train_step(fx[1], fp[1])
    assert one.last["exec"] == "mhimx_ragged_window_run_surv" and one.flat.step == 1 and one.last["risk"].shape == (1,)
    with pytest.raises(Exception, match="pair"):
        one.train_step(fx[1], fp[1][0])                             # a bare bin is not a survival label
    torch.cuda.synchronize()
    assert torch.isfinite(one.flat.student).all() and torch.isfinite(tr.flat.student).all()


@pytest.mark.parametrize("kind", ["pure", "full"])
def test_a_refused_window_takes_the_bag_after_bag_route(kind):
    """use_executor off (what MHIMX_STEP_EXEC=0 sets), with clip_grad set: today's route (the teacher-free model bag after bag, the full
    model's stream form; the head is ops.surv_nll + mhimx_head_fwd_bwd's autograd form) does not raise, draws the same seeds and agrees
    with the native route within test 3's tolerances, after the clipped update too.  Dropout 0: the bag-after-bag route moves the
    dropout tick once per bag, the native call once per window, as for the classification windows."""
    if kind == "pure":
        mk = lambda **kw: _pure_trainer(accum=4, dropout=0.0, **kw)
        xs, pairs = [b.to(DEV) for b in _pure_bags((64, 97, 33, 130), seed=1300)], _pairs([2, 0, 3, 1], [1, 0, 0, 1])
        route = "mhimx_pure_window_run_surv"
    else:
        mk = lambda **kw: _full_pair(accum=3, **kw)[0]
        xs = [torch.from_numpy(synth.bag(1400 + j, n, D)).to(DEV)[None] for j, n in enumerate(FULL_SIZES)]
        pairs, route = _pairs([1, 3, 0], [0, 1, 1]), "mhimx_ragged_window_run_surv"
    nat, fb = mk(), mk()
    fb.use_executor = False
    ln, sn = nat.window_step(xs, pairs, update=False)
    lf, sf = fb.window_step(xs, pairs, update=False)
    torch.cuda.synchronize()
    assert nat.last["exec"] == route and fb.last["exec"] is False
    assert nat.s._step == fb.s._step and int(nat.tick) == 1 and nat._micro == fb._micro == len(xs)
    if kind == "full":
        assert all(torch.equal(a["rows"], b["rows"]) for a, b in zip(nat.last["bags"], fb.last["bags"])), "the two routes drew different rows"
    for j in range(len(xs)):
        np.testing.assert_allclose(ln[j].cpu().numpy().ravel(), lf[j].cpu().numpy().ravel(), atol=1e-4, rtol=0)
        np.testing.assert_allclose(sn[j].cpu().numpy()[:3], sf[j].cpu().numpy()[:3], atol=3e-4, rtol=0)
    np.testing.assert_allclose(nat.last["risk"].cpu().numpy(), fb.last["risk"].cpu().numpy(), atol=3e-4, rtol=0)
    _flat_close(nat, nat.flat.grad, fb.flat.grad)
    gn = float(nat.flat.grad[:nat.flat.n_train].double().norm())
    # the clipped update: outside the call on the native route, bag after bag on the other
    clip = 0.25 * gn
    nat, fb = mk(clip_grad=clip), mk(clip_grad=clip)
    fb.use_executor = False
    nat.window_step(xs, pairs)
    fb.window_step(xs, pairs)
    torch.cuda.synchronize()
    assert nat.last["exec"] == route and fb.last["exec"] is False and nat.flat.step == fb.flat.step == 1
    assert int(nat.opt_step) == int(fb.opt_step) == 1 and nat.s._step == fb.s._step
    err = (nat.flat.student.double() - fb.flat.student.double()).abs()
    assert float(err.mean()) <= 3e-6 and float(err.max()) <= 4.1e-4, (float(err.mean()), float(err.max()))


def test_a_row_pitch_the_call_refuses_is_never_handed_to_it():
    tr_v, tr_c = _pure_trainer(accum=2), _pure_trainer(accum=2)
    views = [torch.rand(n, D + 2, device=DEV)[:, :D] for n in (97, 33)]
    pairs = _pairs([1, 2], [0, 1])
    assert views[0].stride(0) == D + 2 and not tr_v._pure_window_ok(views, [p[0] for p in pairs])
    lv, _ = tr_v.window_step(views, pairs)
    lc, _ = tr_c.window_step([v.contiguous() for v in views], pairs)
    assert tr_v.last["exec"] == "mhimx_pure_window_run_surv" and all(_bits(a, b) for a, b in zip(lv, lc))
    PWG._bits_equal(tr_v, tr_c)


def test_forward_func_runs_the_native_survival_step_and_returns_leaves():
    from mhim_mil_amd.engine import CommonMIL, FusedTrainer
    from mhim_mil_amd.optim import FusedAdamEMA
    from mhim_mil_amd.survival import NLLSurvLoss
    m = _pure_model(dropout=0.25)
    opt = FusedAdamEMA(m, None, lr=2e-4, main_alpha=1.0, aux_alpha=0.0, loss="nll_surv")
    args = types.SimpleNamespace(model="mhim_pure", baseline="attn", aux_alpha=0.0)
    bag = torch.from_numpy(synth.bag(12, 97, D)).to(DEV).unsqueeze(0)
    label = [torch.tensor([2], device=DEV), torch.tensor([1.0], device=DEV)]
    crit = NLLSurvLoss(alpha=0.4)
    out = CommonMIL(args, fused=opt).forward_func(args, m, None, bag, label, crit, 1, 0, 0, 0, None)
    tr = opt.trainer
    lg, aux = out[0], out[2]
    assert out[1] is label and lg.shape == (1, K) and lg.is_leaf and lg.requires_grad and aux.is_leaf and out[3] == out[4] == 97
    assert tr.last["exec"] == "mhimx_pure_window_run_surv" and tr.surv_alpha == 0.4 and _bits(lg.detach().view(-1), tr.last["logits"])
    g_native = tr.flat.grad.clone()
    assert float(g_native.abs().max()) > 0
    loss = crit(logits=lg, Y=label[0], c=label[1]) + args.aux_alpha * aux
    loss.backward()                                                 # the loop's criterion / backward touch no parameter
    assert _bits(tr.flat.grad, g_native) and lg.grad is not None
    assert abs(float(loss.detach()) - float(tr.last["losses"][1])) < 1e-6
    # the same step straight from the trainer: the same bits
    ref = FusedTrainer(_pure_model(dropout=0.25), None, lr=2e-4, model="mhim_pure", main_alpha=1.0, aux_alpha=0.0, loss="nll_surv", surv_alpha=0.4)
    l2, _ = ref.forward_backward(bag, (label[0], label[1]), i=0)
    assert _bits(l2, tr.last["logits"]) and _bits(ref.flat.grad, g_native)
    # any other criterion, or no fused trainer: the autograd form as before (parameters receive gradients through autograd)
    out = CommonMIL(args, fused=opt).forward_func(args, m, None, bag, label, lambda **kw: None, 1, 0, 0, 0, None)
    assert out[0].grad_fn is not None


def test_loss_ce_is_the_trainer_of_before_bit_for_bit():
    xs = [b.to(DEV) for b in _pure_bags(seed=1500)]
    ls = [torch.tensor([y], device=DEV) for y in (0, 3, 1, 2)]
    a, b = _pure_trainer(loss="ce", surv_alpha=0.0), _pure_trainer(loss=None)
    for _ in range(2):
        for tr in (a, b):
            tr.window_step(xs, ls)
            assert tr.last["exec"] is True and "risk" not in tr.last
    torch.cuda.synchronize()
    PWG._bits_equal(a, b, "pure")
    assert a.loss == b.loss == "ce" and a.flat.step == 2
    fx = [torch.from_numpy(synth.bag(1600 + j, n, D)).to(DEV)[None] for j, n in enumerate(FULL_SIZES)]
    fa, fb_ = _full_pair(loss="ce", surv_alpha=0.0)[0], _full_pair(loss=None)[0]
    for tr in (fa, fb_):
        tr.window_step(fx, ls[:3])
        assert tr.last["exec"] == "mhimx_ragged_window_run"
    torch.cuda.synchronize()
    from tests.test_ragged_window_gpu import _same_bits, _state
    assert _same_bits(_state(fa), _state(fb_)) and fa.flat.step == 1
