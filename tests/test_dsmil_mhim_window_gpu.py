"""The ragged train call of the full MHIM(DSMIL) model (mhimx_dsmil_mhim_window_run, csrc/dsmil_mhim.hip) under
FusedTrainer(model="mhim") with a DSMIL student and its EMA teacher - GPU box only.  D = 256, merge_k = 5, the V2 recipe of
tests/test_window_gpu.py, tie-free synth.bag data; bag sizes 64 (the minimum), 97 (no multiple of 32), 257 (a second chunk), 2100, and
16 385 (the multi-workgroup select) in one test.

Bounds (tests/test_ragged_window_gpu.py / tests/test_dsmil_window_gpu.py): logits 1e-4 absolute, loss 3e-4, every gradient
atol = rtol = 2e-3 of its scale; after Adam the student by the DSMIL rule (tol = 0.1 * 2 * lr: mean error <= 0.1 tol, share of elements
above tol < 2e-3), the teacher mean 1e-6 / max 2e-6, the global queries 2e-6.

The dropout and draw seeds mix torch.initial_seed() in: it is pinned for every test."""
import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O
from tests.test_single_pass_gpu import _draws_from_device
from tests.test_window_gpu import V2

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 256
SIZES = (64, 257, 2100, 97)
ROUTE = "mhimx_dsmil_mhim_window_run"
LR = 2e-4
SEED = 20260319
EIGHTEEN = 18


@pytest.fixture(autouse=True)
def _pinned_seed():
    torch.manual_seed(SEED)


def _bag(seed, n):
    return torch.from_numpy(synth.bag(seed, n, D))


def _states(Cc=2):
    base = synth.mhim_state(7, input_dim=D, merge_k=5, baseline="dsmil", n_classes=Cc)
    tsd = synth.mhim_state(11, input_dim=D, merge_k=5, baseline="dsmil", n_classes=Cc)       # a teacher of its own: B_teacher != B
    return base, tsd


def _mk(sd, Cc=2, **cfg):
    from mhim_mil_amd.mhim import MHIM
    m = MHIM(input_dim=D, n_classes=Cc, baseline="dsmil", **cfg)
    sd = dict(sd)
    sd["merge.global_q"] = sd["merge.global_q_mm"]
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    m = m.to(DEV).train()
    m.merge.dropout = 0.0
    return m


def _pair(dropout=0.0, accum=4, Cc=2, executor=True, model_kw=None, aux_alpha=0.5, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    torch.manual_seed(SEED)
    base, tsd = _states(Cc)
    cfg = dict(V2, dropout=dropout, **(model_kw or {}))
    s, t = _mk(base, Cc, **cfg), _mk(tsd, Cc, **cfg)
    tr = FusedTrainer(s, t, lr=LR, aux_alpha=aux_alpha, mm=0.9997, accumulation_steps=accum, **kw)
    if not executor:
        tr.use_executor = False
    return tr, s, t, base, tsd


def _dev(bags, labels):
    return [b.to(DEV)[None] for b in bags], [torch.tensor([l], device=DEV) for l in labels]


def _grads_close(gv, ref, what=""):
    seen = 0
    for name, r in ref.items():
        g, r = gv[name].cpu().numpy(), r.numpy() if torch.is_tensor(r) else r
        err, scale = np.abs(g - r.reshape(g.shape)).max(), np.abs(r).max()
        print(f"  {what}grad {name}: max err {err:.3e} of scale {scale:.3e}")
        np.testing.assert_allclose(g, r.reshape(g.shape), atol=2e-3 * (scale + 1e-30), rtol=2e-3, err_msg=name)
        seen += 1
    return seen


def _state(tr):
    fl = tr.flat
    return [fl.student.clone(), fl.teacher.clone(), fl.m.clone(), fl.v.clone(), tr.opt_step.clone(), tr.tick.clone(), fl.step]


def _restore(tr, snap):
    fl = tr.flat
    fl.student.copy_(snap[0]); fl.teacher.copy_(snap[1]); fl.m.copy_(snap[2]); fl.v.copy_(snap[3])
    tr.opt_step.copy_(snap[4]); tr.tick.copy_(snap[5]); fl.step = snap[6]
    fl.grad.zero_()


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:6], b[:6]))


def _read_draws(per, sizes):
    """Every bag's row list [stay | merge] checked, and the (perm, ids_shuffle, score) that make the oracle pick the same rows."""
    perms, shufs, scores = [], [], []
    for j, n in enumerate(sizes):
        k, n_sel, _ = O.mask_count(n, 0.03, 0.5)
        rows, score = per[j]["rows"].cpu().numpy(), per[j]["score"].cpu().numpy()
        assert rows.shape[0] == n - n_sel and np.unique(rows).shape[0] == rows.shape[0] and rows.min() >= 0 and rows.max() < n
        Lk, R = per[j]["Lk"], per[j]["R"]
        assert Lk + R == rows.shape[0]
        p, sh = _draws_from_device(score, np.concatenate([rows[Lk:], rows[:Lk]]), R, n, k, n_sel)      # (the helper reads [merge | stay])
        perms.append(p); shufs.append(sh); scores.append(torch.from_numpy(score))
    return perms, shufs, scores


def _oracle_window(bags, labels, stu, tea, opt, ocfg, step, perms, shufs, scores, mm, aux_alpha=0.5, tfeats=None, masks=None):
    """One optimiser update over the window, written out from the oracle's pieces (O.train_window does not mix DSMIL's two logit
    vectors): per bag O.forward_teacher, O.forward_student with the injected draws and the device's score, loss_b = (CE(0.5 lb + 0.5 li)
    + aux_alpha cl) / n backward into shared leaves; O.adam_step; the "window" chain of the global queries; O.ema_update."""
    n = len(bags)
    stu_g = {k: v.clone().requires_grad_(k not in O.TRAINABLE_EXCLUDE) for k, v in stu.items()}
    q0 = stu["merge.global_q_mm"].clone()
    info = {"logits": [], "loss": [], "ce": [], "cl": [], "lb": [], "li": [], "B": []}
    q_news = []
    for j, x in enumerate(bags):
        if tfeats is None:
            with torch.no_grad():
                t_feat, _ = O.forward_teacher(x, tea, ocfg)
        else:
            t_feat = tfeats[j]
        lg, cl, _, _, ex = O.forward_student(x, stu_g, ocfg, scores[j], t_feat if aux_alpha != 0.0 else None, perms[j], shufs[j],
                                             drop_mask=None if masks is None else masks[j])
        cl = torch.as_tensor(cl)                           # (0.0 without a teacher feature)
        logits = 0.5 * lg[0] + 0.5 * lg[1]
        ce = O.cross_entropy(logits, int(labels[j]))
        ((ce + aux_alpha * cl) / n).backward()
        info["logits"].append(logits.detach()); info["loss"].append(float(ce.detach() + aux_alpha * cl.detach()))
        info["ce"].append(float(ce.detach())); info["cl"].append(float(cl.detach()))
        info["lb"].append(lg[0].detach()); info["li"].append(lg[1].detach()); info["B"].append(ex["feat"].detach())
        q_news.append(ex["global_q_new"].reshape(q0.shape).detach())
    info["grads"] = {k: p.grad.detach().clone() for k, p in stu_g.items() if p.grad is not None}
    new_stu, new_opt = {}, {}
    for k, p in stu_g.items():
        if p.grad is None:
            new_stu[k] = p.detach()
            continue
        m, v = opt.get(k, (torch.zeros_like(p), torch.zeros_like(p)))
        new_stu[k], m, v = O.adam_step(p.detach(), p.grad, m, v, step, lr=LR, wd=1e-5)
        new_opt[k] = (m, v)
    g_mm, q = float(ocfg.merge_mm), q0.double()
    for qn in q_news:                                      # z_j = (q_new_j - mm q0) / (1 - mm): the tokens of bag j (O.train_window, "window")
        q = g_mm * q + (1.0 - g_mm) * (qn.double() - g_mm * q0.double()) / (1.0 - g_mm)
    new_stu["merge.global_q_mm"] = q.float()
    return new_stu, O.ema_update(tea, new_stu, mm), new_opt, info


def _check_student(mdl, ref, opt, what):
    sd, tol = mdl.state_dict(), 0.1 * 2 * LR
    for name in opt:
        err = (sd[name].detach().cpu().double() - ref[name].double()).abs()
        print(f"  {what} after Adam {name}: mean err {err.mean().item():.3e}, above tol {(err > tol + 1e-7).double().mean().item():.3e}")
        assert err.mean().item() <= 0.1 * tol + 1e-7, (what, name, err.mean().item())
        assert (err > tol + 1e-7).double().mean().item() < 2e-3, (what, name, err.max().item())


def _check_teacher(mdl, ref, what):
    sd = mdl.state_dict()
    for name, r in ref.items():
        err = (sd[name].detach().cpu().double() - r.double().view_as(sd[name])).abs()
        assert err.mean().item() <= 1e-6 and err.max().item() <= 2e-6, (what, name, err.mean().item(), err.max().item())


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("Cc", [2, 5])
def test_two_windows_vs_oracle(Cc):
    """Two consecutive windows of bags {64, 257, 2100, 97}, dropout 0, update=False then tr.update(): every bag's rows and teacher score
    are read back, the draws derived from them, the oracle's window run on them.  Logits, both losses, the summed gradient of all
    eighteen tensors, student / teacher parameters and merge.global_q_mm after the update."""
    tr, s, t, base, tsd = _pair(Cc=Cc)
    ocfg = O.Cfg(**{**V2, "baseline": "dsmil"})
    stu, tea, opt = O.as_torch(base), O.as_torch(tsd), {}
    for u in range(2):
        bags = [_bag(500 + 10 * u + j, n) for j, n in enumerate(SIZES)]
        labels = [(u + j) % Cc for j in range(len(SIZES))]
        xs, ls = _dev(bags, labels)
        tr.window_step(xs, ls, update=False)
        torch.cuda.synchronize()
        assert tr.last["exec"] == ROUTE
        per = tr.last["bags"]
        perms, shufs, scores = _read_draws(per, SIZES)
        stu, tea, opt, info = _oracle_window(bags, labels, stu, tea, opt, ocfg, u + 1, perms, shufs, scores, tr.mm)
        for j in range(len(SIZES)):
            d = np.abs(per[j]["logits"].cpu().numpy().ravel() - info["logits"][j].numpy().ravel()).max()
            print(f"  window {u} bag {j}: logits err {d:.3e}, loss err {abs(float(per[j]['losses'][0]) - info['loss'][j]):.3e}")
            np.testing.assert_allclose(per[j]["logits"].cpu().numpy().ravel(), info["logits"][j].numpy().ravel(), atol=1e-4, rtol=0)
            np.testing.assert_allclose(per[j]["logits_bag"].cpu().numpy().ravel(), info["lb"][j].numpy().ravel(), atol=1e-4, rtol=0)
            np.testing.assert_allclose(per[j]["logits_ins"].cpu().numpy().ravel(), info["li"][j].numpy().ravel(), atol=1e-4, rtol=0)
            assert abs(float(per[j]["losses"][0]) - info["loss"][j]) < 3e-4
            assert abs(float(per[j]["losses"][1]) - info["ce"][j]) < 3e-4 and abs(float(per[j]["losses"][2]) - info["cl"][j]) < 3e-4
        assert _grads_close(tr.flat.grad_views, info["grads"], f"window {u} ") == EIGHTEEN == len(tr.flat.grad_views)
        tr.update()
        torch.cuda.synchronize()
        _check_student(s, stu, opt, f"student, window {u}")
        _check_teacher(t, tea, f"teacher, window {u}")
        np.testing.assert_allclose(s.merge.global_q_mm.detach().cpu().numpy(), stu["merge.global_q_mm"].numpy(), atol=2e-6, rtol=0)
        s.load_state_dict({**stu, "merge.global_q": stu["merge.global_q_mm"]})
        t.load_state_dict({**tea, "merge.global_q": tea["merge.global_q_mm"]})
        for name, (m_ref, v_ref) in opt.items():
            o = tr.flat.offsets[name]
            tr.flat.m[o:o + m_ref.numel()].copy_(m_ref.reshape(-1)); tr.flat.v[o:o + v_ref.numel()].copy_(v_ref.reshape(-1))


def test_aux_alpha_zero_window_vs_oracle():
    """aux_alpha = 0 on the full model: the call launches the head's distillation instantiation without the teacher's B (no other test
    reaches that).  Bags of 64 rows (the call's minimum) and 97 (a ragged last tile), C = 2, against the oracle's window at the bounds
    above; the distillation loss is exactly 0 and the loss exactly main_alpha * CE."""
    sizes = (64, 97)
    tr, s, t, base, tsd = _pair(accum=2, aux_alpha=0.0)
    ocfg = O.Cfg(**{**V2, "baseline": "dsmil"})
    bags = [_bag(550 + j, n) for j, n in enumerate(sizes)]
    labels = [1, 0]
    xs, ls = _dev(bags, labels)
    tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == ROUTE and float(tr._dsmil_mhim_cfg()["cfg"].aux_alpha) == 0.0
    per = tr.last["bags"]
    perms, shufs, scores = _read_draws(per, sizes)
    stu, tea, opt, info = _oracle_window(bags, labels, O.as_torch(base), O.as_torch(tsd), {}, ocfg, 1, perms, shufs, scores, tr.mm, aux_alpha=0.0)
    for j in range(len(sizes)):
        losses = per[j]["losses"].float().cpu()
        print(f"  bag {j}: losses {losses.tolist()}, oracle CE {info['ce'][j]:.6f}")
        np.testing.assert_allclose(per[j]["logits"].cpu().numpy().ravel(), info["logits"][j].numpy().ravel(), atol=1e-4, rtol=0)
        np.testing.assert_allclose(per[j]["logits_bag"].cpu().numpy().ravel(), info["lb"][j].numpy().ravel(), atol=1e-4, rtol=0)
        np.testing.assert_allclose(per[j]["logits_ins"].cpu().numpy().ravel(), info["li"][j].numpy().ravel(), atol=1e-4, rtol=0)
        assert abs(float(losses[0]) - info["loss"][j]) < 3e-4 and abs(float(losses[1]) - info["ce"][j]) < 3e-4
        assert float(losses[2]) == 0.0
        assert float(losses[0]) == float(torch.tensor(tr.main_alpha, dtype=torch.float32) * losses[1])
    assert _grads_close(tr.flat.grad_views, info["grads"]) == EIGHTEEN == len(tr.flat.grad_views)
    tr.update()
    torch.cuda.synchronize()
    _check_student(s, stu, opt, "student")
    _check_teacher(t, tea, "teacher")
    np.testing.assert_allclose(s.merge.global_q_mm.detach().cpu().numpy(), stu["merge.global_q_mm"].numpy(), atol=2e-6, rtol=0)


# ------------------------------------------------------------------------------------------------------------------ 2
def test_one_bag_through_train_step_vs_oracle_and_shape_cached_captures_it():
    """accumulation_steps == 1: train_step takes the call with one bag and the update inside; the result against
    O.train_step(model="mhim") on the read-back draws.  shape_cached then captures the call and a replay is the route's step."""
    n = 257
    tr, s, t, base, tsd = _pair(accum=1)
    ocfg = O.Cfg(**{**V2, "baseline": "dsmil"})
    bag = _bag(600, n)
    x, label = bag.to(DEV)[None], torch.tensor([1], device=DEV)
    logits, losses = tr.train_step(x, label)
    torch.cuda.synchronize()
    assert tr.last["exec"] == ROUTE and tr.flat.step == 1 and int(tr.opt_step) == 1 and tr._micro == 0
    assert float(tr.flat.grad.abs().sum()) == 0                    # (the update ran inside the call and cleared the gradient)
    perms, shufs, scores = _read_draws(tr.last["bags"], (n,))
    stu, tea, _, info = O.train_step(bag, 1, O.as_torch(base), O.as_torch(tsd), {}, ocfg, 1, perm=perms[0], ids_shuffle=shufs[0], aux_alpha=0.5,
                                     mm=tr.mm, lr=LR, score_override=scores[0])
    np.testing.assert_allclose(logits.cpu().numpy().ravel(), info["logits"].numpy().ravel(), atol=1e-4, rtol=0)
    assert abs(float(losses[0]) - info["loss"]) < 3e-4 and abs(float(losses[2]) - info["cls_loss"]) < 3e-4
    _check_student(s, stu, {k: None for k in info["grads"]}, "student")
    _check_teacher(t, tea, "teacher")
    np.testing.assert_allclose(s.merge.global_q_mm.detach().cpu().numpy(), stu["merge.global_q_mm"].numpy(), atol=2e-6, rtol=0)
    # forward_backward alone leaves the gradient and _exec_step's bookkeeping
    tr.forward_backward(x, label)
    assert tr.last["exec"] == ROUTE and tr._micro == 1 and tr.flat.step == 1 and float(tr.flat.grad.abs().sum()) > 0
    tr.update()
    # shape_cached: eager on the first visit, captured on the second, replayed on the third
    for visit in range(3):
        out = tr.shape_cached("train_step", x, label)
        assert out is not None and tr.last["exec"] == ROUTE
    torch.cuda.synchronize()
    assert len(tr._shape_graphs["graphs"]) == 1 and not tr._shape_graphs["bad"]
    assert tr.flat.step == 5 and int(tr.opt_step) == 5 and int(tr.tick) == 5 and torch.isfinite(tr.flat.student).all()


# ------------------------------------------------------------------------------------------------------------------ 3
def test_dropout_masks_teacher_and_student_vs_oracle():
    """Dropout 0.25 on both models, the teacher's instance score as max_c A (attn2score off).  The teacher's B_teacher and score
    against O.dsmil on the read-back H_teacher rows; the student against O.forward_student with the keep-mask taken from dact != 0 and
    the teacher's outputs overridden by the read-back ones."""
    kw = {"attn2score": False}
    tr, s, t, base, tsd = _pair(dropout=0.25, model_kw=kw)
    ocfg = O.Cfg(**{**V2, "baseline": "dsmil", "dropout": 0.25, **kw})
    bags = [_bag(700 + j, n) for j, n in enumerate(SIZES)]
    labels = [0, 1, 1, 0]
    xs, ls = _dev(bags, labels)
    tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == ROUTE and float(tr._dsmil_mhim_cfg()["cfg"].drop_p_teacher) == 0.25
    per = tr.last["bags"]
    tea, stu = O.as_torch(tsd), O.as_torch(base)
    masks, tfeats = [], []
    for j, n in enumerate(SIZES):
        Ht = per[j]["H_teacher"].cpu()
        assert 0.2 < float((Ht == 0).float().mean()) < 0.3
        with torch.no_grad():
            _, _, attn, B, _ = O.dsmil(Ht, tea, cls_attn=False)
        np.testing.assert_allclose(per[j]["score"].cpu().numpy(), attn.numpy().ravel(), atol=1e-4, rtol=2e-3, err_msg=f"score of bag {j}")
        np.testing.assert_allclose(per[j]["B_teacher"].cpu().numpy(), B.numpy(), atol=1e-4, rtol=2e-3, err_msg=f"B_teacher of bag {j}")
        mk = (per[j]["dact"] != 0).cpu()
        assert 0.7 < float(mk.float().mean()) < 0.8
        assert not bool((per[j]["dact"][per[j]["H_student"] == 0] != 0).any())     # a dropped element has no gradient path
        masks.append(mk); tfeats.append(per[j]["B_teacher"].cpu().clone())
    perms, shufs, scores = _read_draws(per, SIZES)
    _, _, _, info = _oracle_window(bags, labels, stu, tea, {}, ocfg, 1, perms, shufs, scores, tr.mm, tfeats=tfeats, masks=masks)
    for j in range(len(SIZES)):
        np.testing.assert_allclose(per[j]["logits"].cpu().numpy().ravel(), info["logits"][j].numpy().ravel(), atol=1e-4, rtol=0)
        np.testing.assert_allclose(per[j]["B"].cpu().numpy(), info["B"][j].numpy(), atol=1e-4, rtol=2e-3)
        assert abs(float(per[j]["losses"][0]) - info["loss"][j]) < 3e-4
    assert _grads_close(tr.flat.grad_views, info["grads"]) == EIGHTEEN


# ------------------------------------------------------------------------------------------------------------------ 4
def test_row_lists_are_student_rows_manys():
    """Every bag's row list is bit-equal to MHIM.student_rows_many on the call's own score, its select seed and the tick (a 16 385-row bag
    takes the multi-workgroup select); len(rows) = N - n_sel, unique, in range."""
    sizes = (64, 16385, 97)
    tr, s, t, _, _ = _pair(accum=3)
    bags = [_bag(800 + j, n) for j, n in enumerate(sizes)]
    xs, ls = _dev(bags, [0, 1, 0])
    step0 = s._step
    tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == ROUTE and s._step == step0 + 3 * len(sizes) and t._step == len(sizes)
    per, table = tr.last["bags"], tr.last["table"]
    for j, n in enumerate(sizes):
        k, n_sel, _ = O.mask_count(n, 0.03, 0.5)
        rows = per[j]["rows"]
        r = rows.cpu().numpy()
        assert r.shape[0] == n - n_sel and np.unique(r).shape[0] == r.shape[0] and r.min() >= 0 and r.max() < n
        s._step = step0 + 3 * j + 1                                # the bag's draws: feature dropout, THE SELECT, Merge
        (ref, len_keep, Lk, R), = s.student_rows_many([per[j]["score"].clone()])
        assert s._step == step0 + 3 * j + 2
        torch.cuda.synchronize()
        assert (len_keep, Lk, R) == (n - n_sel, per[j]["Lk"], per[j]["R"]) and int(table[j].seeds.select) != 0
        assert torch.equal(ref, rows), f"rows of bag {j}"
    s._step = step0 + 3 * len(sizes)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_a_bag_does_not_see_its_neighbours():
    """A bag's score, rows, logits, B and Merge tokens have the same bits at position 0 of {a, b, c}, at position 2 of {c, b, a} and in a
    window of one; the workspace is filled with NaN before each call and every call starts from the same state."""
    from mhim_mil_amd import _lib as L, ops
    tr, s, t, _, _ = _pair(dropout=0.25, accum=3)
    sizes = {"a": 257, "b": 2100, "c": 97}
    xs = {key: _bag(900 + j, n).to(DEV) for j, (key, n) in enumerate(sizes.items())}
    lab = {key: torch.tensor([j % 2], device=DEV) for j, key in enumerate(sizes)}
    seeds = {key: L.StepSeeds(11 + 10 * j, 12 + 10 * j, 13 + 10 * j, 14 + 10 * j) for j, key in enumerate(sizes)}
    tr.window_step([xs[key][None] for key in "abc"], [lab[key] for key in "abc"], update=False)
    assert tr.last["exec"] == ROUTE
    ex = tr._dsmil_mhim_cfg()
    snap = _state(tr)
    got = []
    for order in ("abc", "cba", "a"):
        _restore(tr, snap)
        table = (L.RaggedWindowBag * len(order))()
        for j, key in enumerate(order):
            x = xs[key]
            table[j].X, table[j].ldx, table[j].N, table[j].label_dev = x.data_ptr(), x.stride(0), x.shape[0], lab[key].data_ptr()
            table[j].cnt = L.StepCounts(*s.v2_counts(x.shape[0], None))
            table[j].seeds = seeds[key]
        lay = ops.dsmil_mhim_window(ex["cfg"], table, len(order), layout_only=True)
        ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)                 # NaN everywhere
        ops.dsmil_mhim_window(ex["cfg"], table, len(order), 1, ws, update=False)
        torch.cuda.synchronize()
        j = order.index("a")
        r0, t0, N, cnt = int(lay.row0[j]), int(lay.tok0[j]), sizes["a"], table[j].cnt
        f = lambda off, n_, dt=torch.float32: ws[off:off + n_ * dt.itemsize].view(dt)
        n = len(order)
        got.append((f(lay.score, lay.rows)[r0:r0 + N].clone(), f(lay.rows_all, lay.rows, torch.int64)[r0:r0 + cnt.len_keep].clone(),
                    f(lay.logits, 2 * n).view(n, 2)[j].clone(), f(lay.B, n * 1024).view(n, 1024)[j].clone(),
                    f(lay.B_teacher, n * 1024).view(n, 1024)[j].clone(),
                    f(lay.tokens, lay.tok_rows * 512).view(-1, 512)[t0:t0 + cnt.Lk + 5].clone(),
                    f(lay.losses, 3 * n).view(n, 3)[j].clone()))
        assert all(torch.isfinite(v.float()).all() for v in got[-1])
    for other in got[1:]:
        for a, b, what in zip(got[0], other, ("score", "rows", "logits", "B", "B_teacher", "token rows", "losses")):
            assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------------------------ 6
def test_two_runs_give_the_same_bits_and_a_captured_window_replays_the_eager_windows():
    """Two eager runs of three windows from the same state: the same bits in parameters, both moments, teacher and queries.  One captured
    window replayed three times equals three eager windows of the same bag table, bit for bit (the device tick moves the draws)."""
    from mhim_mil_amd import ops
    bags = [_bag(1000 + j, n) for j, n in enumerate(SIZES)]
    xs, ls = _dev(bags, [1, 0, 0, 1])
    tr_g, *_ = _pair(dropout=0.25)
    snap = _state(tr_g)
    g = tr_g.capture_window(xs, ls, warmup=1)
    assert tr_g.last["exec"] == ROUTE
    table, n = tr_g.last["table"], len(SIZES)
    _restore(tr_g, snap)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    replayed = _state(tr_g)
    runs = []
    for _ in range(2):
        tr_e, *_ = _pair(dropout=0.25)
        assert _same_bits(_state(tr_e), snap)
        ex = tr_e._dsmil_mhim_cfg()
        lay = ops.dsmil_mhim_window(ex["cfg"], table, n, layout_only=True)
        ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)
        for w in range(3):
            ops.dsmil_mhim_window(ex["cfg"], table, n, w + 1, ws, update=True)
        torch.cuda.synchronize()
        runs.append(_state(tr_e))
        assert int(tr_e.tick) == 3 and int(tr_e.opt_step) == 3 and torch.isfinite(tr_e.flat.student).all()
    assert _same_bits(runs[0], runs[1]), "two eager runs differ"
    assert not torch.equal(runs[0][0], snap[0]) and not torch.equal(runs[0][1], snap[1])
    assert _same_bits(runs[0], replayed), "three replays of the captured window differ from three eager windows"


# ------------------------------------------------------------------------------------------------------------------ 7
def test_update_inside_equals_update_outside():
    """update = 1 equals update = 0 followed by mhimx_optim_step (the trainer's update()), bit for bit."""
    bags = [_bag(1100 + j, n) for j, n in enumerate(SIZES)]
    xs, ls = _dev(bags, [1, 0, 1, 0])
    res = []
    for inside in (True, False):
        tr, *_ = _pair(dropout=0.25)
        tr.window_step(xs, ls, update=inside)
        assert tr.last["exec"] == ROUTE and tr._micro == (0 if inside else len(SIZES))
        if not inside:
            assert float(tr.flat.grad.abs().sum()) > 0
            tr.update()
        torch.cuda.synchronize()
        assert tr.flat.step == 1 and int(tr.opt_step) == 1 and float(tr.flat.grad.abs().sum()) == 0
        res.append(_state(tr))
    assert _same_bits(res[0], res[1])


# ------------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision_bags_give_the_bits_of_the_fp32_call(dtype):
    """fp16 / bf16 bags go into the call as they are and give the bits of the fp32 call on x.float()."""
    bags = [_bag(1200 + j, n).to(dtype) for j, n in enumerate(SIZES)]
    labels = [1, 0, 1, 0]
    res = []
    for widen in (False, True):
        tr, *_ = _pair(dropout=0.25)
        xs = [(b.float() if widen else b).to(DEV)[None] for b in bags]
        ls = [torch.tensor([l], device=DEV) for l in labels]
        logits, _ = tr.window_step(xs, ls, update=True)
        torch.cuda.synchronize()
        assert tr.last["exec"] == ROUTE and tr.last["x_dtype"] == (torch.float32 if widen else dtype)
        res.append((_state(tr), [l.clone() for l in logits]))
    assert _same_bits(res[0][0], res[1][0]) and all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("dropout", [0.0, 0.25])
def test_against_todays_route_of_the_same_build(dropout):
    """The call and today's per-op autograd route (use_executor = False) on the same bag from the same state make the same draws (same
    seeds, same tick): logits and the gradient of all eighteen tensors at the bounds above, for every size; the update then agrees too.
    clip_grad runs the update outside the call: window_step(update=True) equals update=False + the clipped update, bit for bit."""
    for j, n in enumerate(SIZES):
        x, label = _bag(1300 + j, n).to(DEV)[None], torch.tensor([j % 2], device=DEV)
        tr, s, t, _, _ = _pair(dropout=dropout, accum=1)
        tr0, s0, t0, _, _ = _pair(dropout=dropout, accum=1, executor=False)
        logits, losses = tr.forward_backward(x, label)
        logits0, losses0 = tr0.forward_backward(x, label)
        torch.cuda.synchronize()
        assert tr.last["exec"] == ROUTE and tr0.last["exec"] is False
        assert (s._step, t._step, int(tr.tick), tr._micro) == (s0._step, t0._step, int(tr0.tick), tr0._micro)
        np.testing.assert_allclose(logits.cpu().numpy().ravel(), logits0.cpu().numpy().ravel(), atol=1e-4, rtol=0)
        assert abs(float(losses[0]) - float(losses0[0])) < 3e-4 and abs(float(losses[2]) - float(losses0[2])) < 3e-4
        fl = tr.flat
        assert torch.equal(fl.grad[fl.n_train:], tr0.flat.grad[fl.n_train:])
        ref = {name: tr0.flat.grad_views[name].detach().cpu() for name in fl.grad_views}
        assert _grads_close(fl.grad_views, ref, f"N = {n} ") == EIGHTEEN
        tr.update(); tr0.update()
        torch.cuda.synchronize()
        assert tr.flat.step == tr0.flat.step == 1
        np.testing.assert_allclose(tr.flat.teacher.cpu().numpy(), tr0.flat.teacher.cpu().numpy(), atol=2e-6, rtol=0)
    if dropout:
        return
    bags = [_bag(1350 + j, n) for j, n in enumerate(SIZES)]
    xs, ls = _dev(bags, [1, 0, 1, 0])
    outs = []
    for how in ("window_step", "by hand"):
        trc, *_ = _pair(clip_grad=0.05)
        trc.window_step(xs, ls, update=(how == "window_step"))
        if how == "by hand":
            assert trc._micro == 4
            gn = float(trc.flat.grad[:trc.flat.n_train].double().norm())
            assert gn > 0.05, gn                                                       # the clip bites
            trc.update()
        torch.cuda.synchronize()
        assert trc.last["exec"] == ROUTE and trc.flat.step == 1
        outs.append(_state(trc))
    assert _same_bits(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------ 10
def _fallback_cases():
    def world(tr, s, t):
        tr.world = 2
    def sche(tr, s, t):
        s.mrh_sche = [0.03] * 8
    def f32(tr, s, t):
        s.prec = "f32"
    def merge_test(tr, s, t):
        t.merge_test = True
    return {"world > 1": (world, {}), "mrh_sche": (sche, {}), "injected draws": (None, "draws"), 'prec="f32"': (f32, {}),
            "merge_test": (merge_test, {}), "a kernel-event hook": (None, "hook")}


@pytest.mark.parametrize("case", list(_fallback_cases()))
def test_refused_cases_take_todays_route(case, monkeypatch):
    """Each refused case takes today's route (exec False) without raising and leaves both seed counters, the tick and the step where
    today's route (use_executor = False) leaves them; without the condition the same bag takes the call."""
    from mhim_mil_amd import ops
    n = 257
    prep, how = _fallback_cases()[case]
    x, label = _bag(1400, n).to(DEV)[None], torch.tensor([1], device=DEV)
    k, n_sel, _ = O.mask_count(n, 0.03, 0.5)
    kw = {"i": 0}
    if how == "draws":
        kw.update(perm=torch.randperm(k, device=DEV), ids_shuffle=torch.randperm(n - n_sel, device=DEV))
    left = []
    for executor in (True, False):
        tr, s, t, _, _ = _pair(accum=1, executor=executor)
        if prep is not None:
            prep(tr, s, t)
        if how == "hook":
            monkeypatch.setattr(ops, "KERNEL_EVENT_HOOK", lambda *a: None)
        assert not tr._dsmil_mhim_window_ok([x[0]], [label], 0) or not executor or how == "draws"
        before = (s._step, t._step, int(tr.tick), tr.flat.step)
        tr.forward_backward(x, label, **kw)
        torch.cuda.synchronize()
        assert tr.last["exec"] is False and torch.isfinite(tr.flat.grad).all() and float(tr.flat.grad.abs().sum()) > 0
        left.append((s._step, t._step, int(tr.tick), tr.flat.step, tr._micro))
        assert left[-1][:3] != before[:3]
        if how == "hook":
            monkeypatch.setattr(ops, "KERNEL_EVENT_HOOK", None)
    assert left[0] == left[1], (case, left)
    tr, s, t, _, _ = _pair(accum=1)
    tr.forward_backward(x, label, i=0)
    # (the student's seed counter is not compared: today's route draws no select seed when the draws are injected)
    assert tr.last["exec"] == ROUTE and (t._step, int(tr.tick), tr.flat.step, tr._micro) == left[0][1:]
    # accumulation windows: a refused window takes the bag-after-bag route too
    tr, s, t, _, _ = _pair(accum=2)
    if prep is not None:
        prep(tr, s, t)
    if how == "hook":
        monkeypatch.setattr(ops, "KERNEL_EVENT_HOOK", lambda *a: None)
    xs, ls = _dev([_bag(1410, 97), _bag(1411, 64)], [0, 1])
    if case == "world > 1":
        return                                                     # (today's route of a window ends in a collective: one process here)
    wkw = {"i": 0}
    if how == "draws":
        wkw.update(perms=[torch.randperm(O.mask_count(m, 0.03, 0.5)[0], device=DEV) for m in (97, 64)],
                   shuffles=[torch.randperm(m - O.mask_count(m, 0.03, 0.5)[1], device=DEV) for m in (97, 64)])
    tr.window_step(xs, ls, **wkw)
    torch.cuda.synchronize()
    assert tr.last["exec"] is False and tr.flat.step == 1 and int(tr.opt_step) == 1
