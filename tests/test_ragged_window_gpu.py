"""The ragged accumulation window of the full MHIM(ABMIL) model (mhimx_ragged_window_run, csrc/ragged_window.hip) under
FusedTrainer(model="mhim", accumulation_steps=k).window_step - GPU box only.  D = 256, C = 2, merge_k = 5, the V2 recipe of
tests/test_window_gpu.py, tie-free synth.bag data; bag sizes 64 (the minimum), 97 (no multiple of 32), 257 (a second scorer chunk), 2100,
and 16 385 (the multi-workgroup select)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O
from tests.test_single_pass_gpu import _draws_from_device
from tests.test_window_gpu import V2, _check_params, _mk

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 256
SIZES = (64, 257, 2100, 97)
ROUTE = "mhimx_ragged_window_run"


def _bag(seed, n):
    return torch.from_numpy(synth.bag(seed, n, D))


def _pair(dropout=0.0, seed=5, accum=4, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    torch.manual_seed(seed)
    base = synth.mhim_state(7, input_dim=D, merge_k=5)
    tsd = synth.spread_teacher(base)
    cfg = dict(V2, dropout=dropout)
    s, t = _mk(base, D, **cfg), _mk(tsd, D, **cfg)
    return FusedTrainer(s, t, aux_alpha=0.5, mm=0.9997, accumulation_steps=accum, **kw), s, t, base, tsd


def _dev(bags, labels):
    return [b.to(DEV)[None] for b in bags], [torch.tensor([l], device=DEV) for l in labels]


def _grads_close(gv, ref):
    for name, r in ref.items():
        g, r = gv[name].cpu().numpy(), r.numpy() if torch.is_tensor(r) else r
        np.testing.assert_allclose(g, r.reshape(g.shape), atol=2e-3 * (np.abs(r).max() + 1e-30), rtol=2e-3, err_msg=name)


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


# ------------------------------------------------------------------------------------------------------------------ 1
def test_two_ragged_windows_vs_oracle():
    """Two consecutive windows of bags {64, 257, 2100, 97}, dropout 0, update=False then tr.update(), by the method of
    tests/test_window_gpu.py::_window_vs_oracle with its bounds: every bag's rows and teacher score are read back, the draws derived from
    them, the oracle's window step (q_ema="window") run on them.  logits 1e-4, loss 3e-4, the window's gradient atol = rtol = 2e-3 of scale,
    student parameters mean 3e-6 / max 4.1e-4 per window, teacher 1e-6 / 2e-6, global queries 2e-6."""
    tr, s, t, base, tsd = _pair()
    ocfg = O.Cfg(**V2)
    stu, tea, opt = O.as_torch(base), O.as_torch(tsd), {}
    for u in range(2):
        bags = [_bag(500 + 10 * u + j, n) for j, n in enumerate(SIZES)]
        labels = [(u + j) % 2 for j in range(len(SIZES))]
        xs, ls = _dev(bags, labels)
        tr.window_step(xs, ls, update=False)
        torch.cuda.synchronize()
        assert tr.last["exec"] == ROUTE
        per = tr.last["bags"]
        perms, shufs, scores = [], [], []
        for j, n in enumerate(SIZES):
            k, n_sel, _ = O.mask_count(n, 0.03, 0.5)
            rows, score = per[j]["rows"].cpu().numpy(), per[j]["score"].cpu().numpy()
            assert rows.shape[0] == n - n_sel and np.unique(rows).shape[0] == rows.shape[0] and rows.min() >= 0 and rows.max() < n
            p, sh = _draws_from_device(score, rows, per[j]["R"], n, k, n_sel)
            perms.append(p); shufs.append(sh); scores.append(torch.from_numpy(score))
        stu, tea, opt, info = O.train_window(bags, labels, stu, tea, opt, ocfg, u + 1, perms=perms, shuffles=shufs, q_ema="window",
                                             score_overrides=scores, mm=tr.mm)
        for j in range(len(SIZES)):
            np.testing.assert_allclose(per[j]["logits"].cpu().numpy().ravel(), info["logits"][j].numpy().ravel(), atol=1e-4, rtol=0)
            assert abs(float(per[j]["losses"][0]) - info["loss"][j]) < 3e-4
        _grads_close(tr.flat.grad_views, info["grads"])
        tr.update()
        torch.cuda.synchronize()
        _check_params(s, stu, 3e-6, 4.1e-4 * (u + 1), f"student, window {u}")
        _check_params(t, tea, 1e-6, 2e-6, f"teacher, window {u}")
        np.testing.assert_allclose(s.merge.global_q_mm.detach().cpu().numpy(), stu["merge.global_q_mm"].numpy(), atol=2e-6, rtol=0)
        s.load_state_dict({**stu, "merge.global_q": stu["merge.global_q_mm"]})
        t.load_state_dict({**tea, "merge.global_q": tea["merge.global_q_mm"]})


# ------------------------------------------------------------------------------------------------------------------ 2
def test_teacher_half_and_select_on_its_own():
    """Each bag's instance score and z_teacher against O.forward_teacher, at the bound the existing executor test applies to the step's
    score (tests/test_single_pass_gpu.py::test_production_step_vs_oracle_c2: atol 1e-4, rtol 2e-3); z_teacher - a convex combination of
    feature rows made at the same precision with weights that carry the score's error - at the same bound.  mhimx_select_rows re-run on
    the call's own score with the same seed and tick gives the call's rows_all bit for bit; the select_large sequence does for the
    16 385-row bag."""
    from mhim_mil_amd import ops
    sizes = (64, 16385, 97)
    tr, s, t, base, tsd = _pair(accum=3)
    bags = [_bag(700 + j, n) for j, n in enumerate(sizes)]
    xs, ls = _dev(bags, [0, 1, 0])
    tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == ROUTE
    per, table = tr.last["bags"], tr.last["table"]
    ocfg, tea = O.Cfg(**V2), O.as_torch(tsd)
    for j, n in enumerate(sizes):
        z_ref, sc_ref = O.forward_teacher(bags[j], tea, ocfg)
        np.testing.assert_allclose(per[j]["score"].cpu().numpy(), sc_ref.numpy().ravel(), atol=1e-4, rtol=2e-3, err_msg=f"score of bag {j}")
        np.testing.assert_allclose(per[j]["z_teacher"].cpu().numpy(), z_ref.numpy().ravel(), atol=1e-4, rtol=2e-3, err_msg=f"z_teacher of bag {j}")
        cnt, seed = table[j].cnt, int(table[j].seeds.select)
        score = per[j]["score"].clone()
        if n <= 16384:
            rows = ops.select_rows(score, cnt.k_top, cnt.n_sel, cnt.R, seed, tick=tr.tick, merge_first=True)
        else:
            pm = ops.random_perm(cnt.k_top, seed + 0x51ED270B, tick=tr.tick, device=score.device)
            ids, _, _ = ops.select_mask(score, cnt.k_top, cnt.n_sel, True, perm=pm if cnt.n_sel < cnt.k_top else None)
            r2 = ops.random_perm(cnt.len_keep, seed ^ 0x3C6EF372FE94F82B, tick=tr.tick, src=ids)
            rows = torch.cat([r2[cnt.Lk:], r2[:cnt.Lk]])
        torch.cuda.synchronize()
        assert torch.equal(rows, per[j]["rows"]), f"rows_all of bag {j}"
        off = tr.last["layout"].rows_all + 8 * (per[j]["row0"] + cnt.len_keep)                 # the list's constant tail: the k token rows
        assert torch.equal(tr.last["ws"][off:off + 40].view(torch.int64).cpu(), torch.arange(n, n + 5))


# ------------------------------------------------------------------------------------------------------------------ 3
def _single_bag_runs(tr1, xs, ls, table, q0, tick0):
    """mhimx_step_run(update = 0) on each bag alone with the window's seeds, its first queries and its tick value.  Returns per bag
    (H_student, dact, H_teacher, logits, gradient)."""
    from mhim_mil_amd import _lib as L, ops
    out = []
    ex = tr1._exec_cfg()
    for j, x in enumerate(xs):
        x2, N = x[0], x.shape[1]
        cnt, lay = table[j].cnt, L.StepLayout()
        L.check(L.lib().mhimx_step_layout_of(C.byref(ex["cfg"]), N, C.byref(cnt), C.byref(lay)), "mhimx_step_layout_of")
        ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)
        tr1.s.merge.global_q_mm.data.copy_(q0)
        tr1.tick.copy_(tick0)
        tr1.flat.grad.zero_()
        seeds = table[j].seeds
        L.check(L.lib().mhimx_step_run(ops._stream(), C.byref(ex["cfg"]), x2.data_ptr(), x2.stride(0), N, ls[j].data_ptr(), C.byref(cnt), C.byref(seeds),
                                       1, ws.data_ptr(), ws.numel(), 0), "mhimx_step_run")
        torch.cuda.synchronize()
        f = lambda off, n_, dt=torch.float32: ws[off:off + n_ * dt.itemsize].view(dt)
        out.append((f(lay.H_student, N * 512).view(N, 512).clone(), f(lay.dact, N * 512, torch.float16).view(N, 512).clone(),
                    f(lay.H_teacher, N * 512).view(N, 512).clone(), f(lay.logits, 2).clone(), tr1.flat.grad.clone()))
    return out


def test_mask_contract_against_the_single_bag_step():
    """Dropout 0.25 on both models.  For each bag the zero pattern of the student's feature rows, of d out / d pre and of the teacher's
    rows equals mhimx_step_run(update = 0)'s on that bag alone with the same seeds at the same tick value, exactly; logits (1e-4) and the
    window's gradient (atol = rtol = 2e-3 of scale) agree with those single-bag runs - given the window's first queries - summed and
    scaled by 1 / n."""
    tr, s, t, _, _ = _pair(dropout=0.25)
    tr1, s1, t1, _, _ = _pair(dropout=0.25, accum=1)
    assert float(tr._exec_cfg()["cfg"].drop_p_teacher) == 0.25
    bags = [_bag(800 + j, n) for j, n in enumerate(SIZES)]
    xs, ls = _dev(bags, [0, 1, 1, 0])
    q0, tick0 = s.merge.global_q_mm.data.clone(), tr.tick.clone()
    tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == ROUTE and int(tr.tick) == int(tick0) + 1
    per = tr.last["bags"]
    win = [(p["H_student"].clone(), p["dact"].clone(), p["H_teacher"].clone(), p["logits"].clone()) for p in per]
    g_win = tr.flat.grad.clone()
    one = _single_bag_runs(tr1, xs, ls, tr.last["table"], q0, tick0)
    n = len(SIZES)
    for j in range(n):
        for a, b, what in zip(win[j][:3], one[j][:3], ("student rows", "d out / d pre", "teacher rows")):
            za, zb = a == 0, b == 0
            assert 0.2 < float(za.float().mean()) < 0.3, (j, what, float(za.float().mean()))
            assert torch.equal(za, zb), (j, what, int((za != zb).sum()))
        np.testing.assert_allclose(win[j][3].cpu().numpy(), one[j][3].cpu().numpy(), atol=1e-4, rtol=0)
    g_sum = sum(o[4].double() for o in one) / n
    nt = tr.flat.n_train
    ref = {name: g_sum[tr.flat.offsets[name]:tr.flat.offsets[name] + v.numel()].float().cpu() for name, v in tr.flat.grad_views.items()}
    assert nt > 0
    views = {name: g_win[tr.flat.offsets[name]:tr.flat.offsets[name] + v.numel()] for name, v in tr.flat.grad_views.items()}
    _grads_close(views, ref)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_a_bag_does_not_see_its_neighbours():
    """A bag's score, rows_all, logits and token rows have the same bits at position 0 of {a, b, c}, at position 2 of {c, b, a} and in a
    window of one; the workspace is filled with NaN before each call and every call starts from the same state."""
    from mhim_mil_amd import _lib as L, ops
    tr, s, t, _, _ = _pair(dropout=0.25, accum=3)
    sizes = {"a": 257, "b": 16385, "c": 97}
    xs = {key: _bag(900 + j, n).to(DEV) for j, (key, n) in enumerate(sizes.items())}
    lab = {key: torch.tensor([j % 2], device=DEV) for j, key in enumerate(sizes)}
    seeds = {key: L.StepSeeds(11 + 10 * j, 12 + 10 * j, 13 + 10 * j, 14 + 10 * j) for j, key in enumerate(sizes)}
    ex = tr._exec_cfg()
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
        lay = ops.ragged_window(ex["cfg"], table, len(order), layout_only=True)
        ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)                 # NaN everywhere
        ops.ragged_window(ex["cfg"], table, len(order), 1, ws, update=False)
        torch.cuda.synchronize()
        j = order.index("a")
        r0, N, cnt = int(lay.row0[j]), sizes["a"], table[j].cnt
        f = lambda off, n_, dt=torch.float32: ws[off:off + n_ * dt.itemsize].view(dt)
        got.append((f(lay.score, lay.rows)[r0:r0 + N].clone(), f(lay.rows_all, lay.rows, torch.int64)[r0:r0 + cnt.len_keep + 5].clone(),
                    f(lay.logits, 16 * len(order)).view(-1, 16)[j, :2].clone(), f(lay.H_student, lay.rows * 512).view(-1, 512)[r0 + N:r0 + N + 5].clone()))
        assert all(torch.isfinite(v.float()).all() for v in got[-1])
    for other in got[1:]:
        for a, b, what in zip(got[0], other, ("score", "rows_all", "logits", "tokens")):
            assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------------------------ 5
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
        ex = tr_e._exec_cfg()
        lay = ops.ragged_window(ex["cfg"], table, n, layout_only=True)
        ws = torch.full((lay.total,), 255, dtype=torch.uint8, device=DEV)
        for w in range(3):
            ops.ragged_window(ex["cfg"], table, n, w + 1, ws, update=True)
        torch.cuda.synchronize()
        runs.append(_state(tr_e))
        assert int(tr_e.tick) == 3 and int(tr_e.opt_step) == 3 and torch.isfinite(tr_e.flat.student).all()
    assert _same_bits(runs[0], runs[1]), "two eager runs differ"
    assert not torch.equal(runs[0][0], snap[0])
    assert _same_bits(runs[0], replayed), "three replays of the captured window differ from three eager windows"


# ------------------------------------------------------------------------------------------------------------------ 6
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


# ------------------------------------------------------------------------------------------------------------------ 7
def test_trainer_routes(monkeypatch):
    """A ragged window_step reports the new route, a same-shaped one mhimx_window_run's, injected draws and MHIMX_STEP_EXEC=0 the stream
    form; the new route and the stream form on the same ragged bags (same draws) agree at the bounds of test 1; a shorter last window (2
    of 3 bags) is scaled by 2; clip_grad equals update=False + the clipped update."""
    bags = [_bag(1200 + j, n) for j, n in enumerate(SIZES)]
    xs, ls = _dev(bags, [1, 0, 1, 0])
    tr, s, *_ = _pair()
    logits, losses = tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == ROUTE and len(tr.last["bags"]) == 4
    new = ([l.clone() for l in logits], tr.flat.grad.clone(), [b["rows"].clone() for b in tr.last["bags"]])
    # the stream form on the same bags (MHIMX_STEP_EXEC=0 is read when a trainer is made)
    monkeypatch.setenv("MHIMX_STEP_EXEC", "0")
    tr0, *_ = _pair()
    monkeypatch.delenv("MHIMX_STEP_EXEC")
    assert tr0.use_executor is False
    logits0, _ = tr0.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr0.last["exec"] is False
    assert all(torch.equal(a, b["rows"]) for a, b in zip(new[2], tr0.last["bags"])), "the two routes drew different rows"
    for a, b in zip(new[0], logits0):
        np.testing.assert_allclose(a.cpu().numpy().ravel(), b.cpu().numpy().ravel(), atol=1e-4, rtol=0)
    fl = tr.flat
    ref = {name: tr0.flat.grad[fl.offsets[name]:fl.offsets[name] + v.numel()].cpu() for name, v in fl.grad_views.items()}
    _grads_close({name: new[1][fl.offsets[name]:fl.offsets[name] + v.numel()] for name, v in fl.grad_views.items()}, ref)
    # a same-shaped window keeps mhimx_window_run; injected draws keep the bag-after-bag route
    same = [_bag(1300 + j, 300).to(DEV)[None] for j in range(4)]
    tr2, s2, *_ = _pair()
    tr2.window_step(same, ls, update=False)
    assert tr2.last["exec"] == "mhimx_window_run"
    tr2.update()
    perms, shufs = [], []
    for n in SIZES:
        k, n_sel, _ = O.mask_count(n, 0.03, 0.5)
        perms.append(torch.randperm(k, device=DEV)); shufs.append(torch.randperm(n - n_sel, device=DEV))
    tr2.window_step(xs, ls, perms=perms, shuffles=shufs)
    assert tr2.last["exec"] is False and tr2.flat.step == 2
    # a shorter last window: 2 of 3 bags, every loss scaled by 1 / 2
    tr3, *_ = _pair(accum=3)
    tr3.window_step(xs[:2], ls[:2], update=False)
    torch.cuda.synchronize()
    assert tr3.last["exec"] == ROUTE
    g2 = tr3.flat.grad.clone()
    tr4, *_ = _pair(accum=2)
    tr4.window_step(xs[:2], ls[:2], update=False)
    torch.cuda.synchronize()
    assert tr4.last["exec"] == ROUTE and torch.equal(g2, tr4.flat.grad)
    # clip_grad: the update stays outside the call
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
