"""The one-call teacher-free ABMIL step (mhimx_pure_step_run, csrc/step.hip) under FusedTrainer(model="mhim_pure"): bit for bit against the
Python orchestration it replaces, and against the CPU oracle (oracle/mhim_oracle.py: pure, train_step(model="mhim_pure"), adam_step).
Tolerances are the project's own for train steps (tests/test_single_pass_gpu.py): logits 1e-4 absolute, gradients and Adam moments 2e-3 of
the tensor's scale, parameters after Adam as test_production_step_vs_oracle_c2 bounds them."""
import os
import signal

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(act="gelu", da_act="relu", merge_enable=False)


@pytest.fixture(autouse=True)
def _time_limit(request):
    """Every test here carries its own time limit (seconds; ``time_limit`` attribute of the test function, default 300)."""
    limit = int(getattr(request.function, "time_limit", 300))

    def expired(*_):
        raise TimeoutError(f"{request.node.name}: longer than {limit} s")

    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(limit)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def limit(seconds):
    def deco(fn):
        fn.time_limit = seconds
        return fn
    return deco


def _model(D=512, dropout=0.25, seed=7, **kw):
    from mhim_mil_amd.mhim import MHIM
    m = MHIM(input_dim=D, n_classes=2, baseline="attn", dropout=dropout, **{**CFG, **kw})
    sd = synth.mhim_state(seed, input_dim=D, merge_enable=False)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(DEV).train()


def _trainer(D=512, dropout=0.25, executor=True, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    tr = FusedTrainer(_model(D, dropout), None, lr=kw.pop("lr", 1e-3), model="mhim_pure", **kw)
    if not executor:
        tr.use_executor = False
    return tr


def _state(tr):
    fl = tr.flat
    return [fl.student.clone(), fl.m.clone(), fl.v.clone(), tr.opt_step.clone(), tr.tick.clone()]


def _bits_equal(tr_a, tr_b, what=""):
    for name, a, b in zip(("student", "m", "v", "opt_step", "tick"), _state(tr_a), _state(tr_b)):
        assert torch.equal(a, b), (what, name, float((a.double() - b.double()).abs().max()))
    assert tr_a.s._step == tr_b.s._step and tr_a.flat.step == tr_b.flat.step, what


# ------------------------------------------------------------------------------------------------------------------ 1
@limit(420)
@pytest.mark.parametrize("n,D", [(512, 1024), (10000, 1024), (40000, 1024)])
def test_executor_equals_the_python_orchestration_bit_for_bit(n, D):
    """Three consecutive train steps with dropout 0.25 - c1, 10 000 rows and a bag above the 16 384-row forms: mhimx_pure_step_run issues
    the launches of _nat_prep / _nat_bag / _apply with the same arguments and the same seed, so parameters, both Adam moments, logits,
    losses, the model's seed counter and the device tick / opt_step counters agree BIT FOR BIT."""
    tr_c, tr_p = _trainer(D), _trainer(D, executor=False)
    g = torch.Generator(device=DEV).manual_seed(n)
    for step in range(3):
        x = torch.randn(n, D, device=DEV, generator=g).abs_()
        lab = torch.tensor([step % 2], device=DEV)
        assert tr_c._exec_ok(x) and tr_c._nat_ok(x)
        lc, sc = tr_c.train_step(x, lab)
        lp, sp = tr_p.train_step(x, lab)
        assert tr_c.last["exec"] is True and tr_p.last["exec"] is False
        assert tr_c.last["patch_num"] == tr_c.last["keep_num"] == n and tr_c.last["ws"] is not None
        assert torch.equal(lc, lp) and torch.equal(sc, sp), (step, lc, lp, sc, sp)
        assert torch.equal(tr_c.last["H_student"], tr_p.last["H_student"])
        keep = float((tr_c.last["H_student"] != 0).float().mean())
        assert abs(keep - 0.75) < 0.02, keep                                      # a 0.25 dropout, not a degenerate mask
        _bits_equal(tr_c, tr_p, step)
    assert tr_c.flat.step == 3 and int(tr_c.opt_step) == 3 and int(tr_c.tick) == 3 and tr_c.s._step == 3      # ONE seed per bag


def test_switch_selects_the_python_orchestration(monkeypatch):
    """MHIMX_STEP_EXEC=0 keeps selecting the Python orchestration for the pure kind."""
    monkeypatch.setenv("MHIMX_STEP_EXEC", "0")
    tr = _trainer()
    assert tr.use_executor is False
    x = torch.rand(700, 512, device=DEV)
    assert not tr._exec_ok(x)
    tr.train_step(x, torch.tensor([1], device=DEV))
    assert tr.last["exec"] is False


# ------------------------------------------------------------------------------------------------------------------ 2, 3
def _check_against(tr, info_grads, logits, loss_ce, ref_logits, ref_loss):
    np.testing.assert_allclose(logits.cpu().numpy().ravel(), ref_logits.numpy().ravel(), atol=1e-4, rtol=0)
    assert abs(float(loss_ce) - ref_loss) < 3e-4
    gv = tr.flat.grad_views
    assert set(info_grads) == set(gv)
    for name, ref in info_grads.items():
        g, r = gv[name].cpu().numpy(), ref.numpy()
        np.testing.assert_allclose(g, r.reshape(g.shape), atol=2e-3 * (np.abs(r).max() + 1e-30), rtol=2e-3, err_msg=name)


def _check_after_adam(tr, stu_ref, opt_ref, step):
    sd, fl = tr.s.state_dict(), tr.flat
    for name, ref in stu_ref.items():
        # (Adam's first steps are sign-like: rounding-level gradient differences move the few elements whose gradient is ~0 by up to 2 lr;
        # the bulk must agree tightly - test_production_step_vs_oracle_c2's bound)
        err = (sd[name].detach().cpu().double() - ref.double()).abs()
        assert err.mean().item() <= 3e-6 and err.max().item() <= 4.1e-4 * (step + 1), (step, name, err.mean().item(), err.max().item())
    for name, (m_ref, v_ref) in opt_ref.items():
        o, n = fl.offsets[name], m_ref.numel()
        for what, got, ref in (("m", fl.m[o:o + n], m_ref), ("v", fl.v[o:o + n], v_ref)):
            r = ref.numpy().ravel()
            np.testing.assert_allclose(got.cpu().numpy(), r, atol=2e-3 * (np.abs(r).max() + 1e-30), rtol=2e-3, err_msg=f"{what} {name} step {step}")


@limit(600)
@pytest.mark.parametrize("n,D", [(512, 1024), (10000, 1024)])
def test_two_steps_vs_oracle(n, D):
    """Dropout 0, two steps against O.train_step(model="mhim_pure"): logits, CE, every parameter gradient, the parameters and the Adam
    moments after each update.  Step 1 is forward_backward (update = 0, the gradient inspected) + update(), step 2 one train_step (the
    update inside the call)."""
    tr = _trainer(D, dropout=0.0, lr=2e-4)
    base = synth.mhim_state(7, input_dim=D, merge_enable=False)
    ocfg = O.Cfg(dropout=0.0, **CFG)
    stu, opt = O.as_torch(base), {}
    bags = [torch.from_numpy(synth.bag(300 + i, n, D)) for i in range(2)]
    labels = [1, 0]
    # ---- step 1
    lab = torch.tensor([labels[0]], device=DEV)
    logits, losses = tr.forward_backward(bags[0].to(DEV)[None], lab)
    torch.cuda.synchronize()
    assert tr.last["exec"] is True and tr.flat.step == 0
    stu, _, opt, info = O.train_step(bags[0], labels[0], stu, None, opt, ocfg, 1, model="mhim_pure", aux_alpha=0.0)
    _check_against(tr, info["grads"], logits, losses[1], info["logits"], info["loss"])
    assert float(losses[2]) == 0.0 and float(losses[0]) == float(losses[1])            # no distillation term
    tr.update()
    torch.cuda.synchronize()
    _check_after_adam(tr, stu, opt, 0)
    # ---- step 2: continue from the oracle's state so that exactly one step separates what is compared
    tr.s.load_state_dict(stu)
    for name, (m_ref, v_ref) in opt.items():
        o = tr.flat.offsets[name]
        tr.flat.m[o:o + m_ref.numel()].copy_(m_ref.reshape(-1))
        tr.flat.v[o:o + v_ref.numel()].copy_(v_ref.reshape(-1))
    logits, losses = tr.train_step(bags[1].to(DEV)[None], torch.tensor([labels[1]], device=DEV))
    torch.cuda.synchronize()
    assert tr.last["exec"] is True and tr.flat.step == 2
    stu2, _, opt2, info = O.train_step(bags[1], labels[1], stu, None, opt, ocfg, 2, model="mhim_pure", aux_alpha=0.0)
    np.testing.assert_allclose(logits.cpu().numpy().ravel(), info["logits"].numpy().ravel(), atol=1e-4, rtol=0)
    assert abs(float(losses[0]) - info["loss"]) < 3e-4
    _check_after_adam(tr, stu2, opt2, 1)


@limit(300)
def test_c1_step_with_dropout_vs_oracle():
    """The timed configuration of c1 - 512 x 1024, dropout 0.25: the keep-mask the projection kernel drew from its counter hash is read
    back from the step's feature rows (a GELU output is exactly zero only where it was dropped) and handed to O.pure; autograd and
    O.adam_step give the reference gradients, parameters and moments."""
    n, D = 512, 1024
    tr = _trainer(D, dropout=0.25, lr=2e-4)
    base = synth.mhim_state(7, input_dim=D, merge_enable=False)
    bag = torch.from_numpy(synth.bag(300, n, D))
    logits, losses = tr.forward_backward(bag.to(DEV)[None], torch.tensor([1], device=DEV))
    torch.cuda.synchronize()
    assert tr.last["exec"] is True
    keep = (tr.last["H_student"] != 0).cpu()
    assert abs(float(keep.float().mean()) - 0.75) < 5e-3
    dact = tr.last["ws"][tr._exec["layouts"][("pure", n)][1].dact:][:n * 512 * 2].view(torch.float16).view(n, 512)
    assert not bool((dact[~keep.to(DEV)] != 0).any())                            # a dropped element has no gradient path
    po = {k: v.clone().requires_grad_(True) for k, v in O.as_torch(base).items()}
    lo = O.pure(bag, po, O.Cfg(dropout=0.25, **CFG), drop_mask=keep)
    loss = O.cross_entropy(lo, 1)
    loss.backward()
    grads = {k: p.grad.detach() for k, p in po.items()}
    _check_against(tr, grads, logits, losses[1], lo.detach(), float(loss.detach()))
    tr.update()
    torch.cuda.synchronize()
    stu, opt = {}, {}
    for k, p in po.items():
        pn, m, v = O.adam_step(p.detach(), p.grad, torch.zeros_like(p), torch.zeros_like(p), 1, lr=2e-4, wd=1e-5)
        stu[k], opt[k] = pn, (m, v)
    _check_after_adam(tr, stu, opt, 0)


# ------------------------------------------------------------------------------------------------------------------ 4
@limit(240)
def test_update_0_leaves_the_complete_gradient_and_nothing_else():
    """update = 0 (forward_backward): the flat gradient has the bits of the Python path's; no parameter, no moment and no update count
    changed.  (The DEVICE opt_step counter is advanced by the step's first launch in both routes - the Adam that follows reads it - so it
    is compared between the routes, not against zero.)"""
    tr_c, tr_p = _trainer(), _trainer(executor=False)
    before = _state(tr_c)
    x = torch.rand(3000, 512, device=DEV)
    lab = torch.tensor([1], device=DEV)
    for tr in (tr_c, tr_p):
        tr.forward_backward(x, lab)
    assert tr_c.last["exec"] is True and tr_p.last["exec"] is False
    assert torch.equal(tr_c.flat.grad, tr_p.flat.grad) and float(tr_c.flat.grad.abs().max()) > 0
    for a, b in zip(before[:3], _state(tr_c)[:3]):
        assert torch.equal(a, b)
    assert tr_c.flat.step == 0 and torch.equal(tr_c.opt_step, tr_p.opt_step)
    for tr in (tr_c, tr_p):
        tr.update()
        tr.train_step(x, lab)
    _bits_equal(tr_c, tr_p)


def _dp_bags(D=512):
    g = torch.Generator(device=DEV).manual_seed(77)
    return [torch.randn(n, D, device=DEV, generator=g).abs_() for n in (2048, 1700)]


def _dp_worker(rank, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)                                   # (both ranks share the box's one GPU; gloo stages through the host)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    tr = _trainer(dropout=0.0)
    assert tr.world == 2 and tr._chain is None
    tr.overlap_comm = False                                    # (the mid-backward all-reduce hook lives in the Python orchestration)
    x = _dp_bags()[rank]
    lg, _ = tr.train_step(x, torch.tensor([rank], device=DEV))
    assert tr.last["exec"] is True, "the rank's step did not go through the executor"
    torch.cuda.synchronize()
    torch.save({"logits": lg.cpu().clone(), "state": [v.cpu() for v in _state(tr)]}, os.path.join(out, f"pure_dp{rank}.pt"))
    dist.destroy_process_group()


@limit(600)
def test_data_parallel_rank_step_through_the_executor(tmp_path):
    """Two ranks on one GPU (gloo), one bag each, update = 0 + all-reduce + mhimx_optim_step, against ONE process with accumulation 2 over
    the same two bags (the Python orchestration): the mean of two gradients either way, summed in another order - the replicas are
    bit-identical, and agree with the single process within test_round6_gpu.py's data-parallel bound.  Dropout off: the seed streams of
    two processes and of one differ by construction."""
    import torch.multiprocessing as mp
    port = 43100 + (os.getpid() % 500)
    mp.spawn(_dp_worker, args=(port, str(tmp_path)), nprocs=2, join=True)
    res = [torch.load(os.path.join(tmp_path, f"pure_dp{r}.pt")) for r in range(2)]
    for a, b in zip(res[0]["state"], res[1]["state"]):
        assert torch.equal(a, b)
    tr = _trainer(dropout=0.0, accumulation_steps=2)
    logits = []
    for r, x in enumerate(_dp_bags()):
        lg, _ = tr.train_step(x, torch.tensor([r], device=DEV))
        logits.append(lg.cpu().clone())
        assert tr.last["exec"] is False
    torch.cuda.synchronize()
    assert tr.flat.step == 1
    for r in range(2):
        assert torch.allclose(res[r]["logits"], logits[r], atol=2e-4), (r, res[r]["logits"], logits[r])
    one = [v.cpu() for v in _state(tr)]
    for name, a, b in zip(("student", "m", "v"), res[0]["state"], one):
        d = (a.float() - b.float()).abs()
        assert float(d.mean()) <= 1.2e-5 and float(d.max()) <= 6.6e-3, (name, float(d.mean()), float(d.max()))
    assert torch.equal(res[0]["state"][3], one[3])                             # one update either way


# ------------------------------------------------------------------------------------------------------------------ 5
@limit(420)
def test_run_steps_equals_train_steps():
    """mhimx_pure_step_run_many: 12 bags of 12 different sizes (64 .. 30 000 rows) as ONE C call == 12 train_steps, bit for bit."""
    sizes = [64, 30000, 100, 777, 16384, 2048, 16385, 5000, 1001, 23456, 333, 9999]
    tr_m, tr_1 = _trainer(), _trainer()
    g = torch.Generator(device=DEV).manual_seed(4)
    bags = [torch.randn(n, 512, device=DEV, generator=g).abs_() for n in sizes]
    labels = [torch.tensor([j % 2], device=DEV) for j in range(len(bags))]
    lm, sm = tr_m.run_steps(bags, labels)
    assert tr_m.last["exec"] is True and tr_m.flat.step == 12 and tr_m.last["patch_num"] == sizes[-1]
    for b, l in zip(bags, labels):
        l1, s1 = tr_1.train_step(b, l)
        assert tr_1.last["exec"] is True
    assert torch.equal(lm, l1) and torch.equal(sm, s1)
    _bits_equal(tr_m, tr_1)
    assert int(tr_m.opt_step) == 12 and tr_m.s._step == 12
    with pytest.raises(Exception):
        tr_m.run_steps(bags[:2], labels[:1])


# ------------------------------------------------------------------------------------------------------------------ 6
@limit(300)
def test_captured_step_replays_with_the_bits_of_eager_steps():
    """A hipGraph of one step replayed three times == three eager steps from the same start: the call is enqueue-only, and the dropout
    position and the Adam step live in device counters, so every replay draws a fresh mask.  Both start from a NaN-poisoned (0xFF)
    workspace: the eager one is made that way by _exec_step, the graph's is filled here."""
    n = 2500
    tr_g, tr_e = _trainer(), _trainer()
    x = torch.rand(n, 512, device=DEV)
    lab = torch.tensor([1], device=DEV)
    snap = _state(tr_g)
    graph = tr_g.capture(x, lab, warmup=1)
    seed_step = tr_g.s._step                                    # the capture baked the seed of this position of the model's stream
    assert tr_g.last["exec"] is True
    fl = tr_g.flat
    fl.student.copy_(snap[0]); fl.m.copy_(snap[1]); fl.v.copy_(snap[2]); tr_g.opt_step.copy_(snap[3]); tr_g.tick.copy_(snap[4])
    fl.grad.zero_()
    tr_g.last["ws"].fill_(255)
    masks = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        masks.append((tr_g.last["H_student"] != 0).clone())
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])
    for _ in range(3):
        tr_e.s._step = seed_step - 1                            # (the same seed as the graph's; the tick moves on by itself)
        le, se = tr_e.train_step(x, lab)
        assert tr_e.last["exec"] is True
    torch.cuda.synchronize()
    assert torch.equal(tr_g.last["logits"], le) and torch.equal(tr_g.last["losses"], se)
    for name, a, b in zip(("student", "m", "v", "opt_step", "tick"), _state(tr_g), _state(tr_e)):
        assert torch.equal(a, b), name
    assert torch.isfinite(tr_g.flat.student).all()


@limit(300)
def test_shape_cache_captures_the_pure_step():
    """shape_cached: eager on the first visit, captured on the second, replayed afterwards - through the executor and through the Python
    orchestration (both captures freeze the same host-side seed): bit for bit."""
    tr_c, tr_p = _trainer(), _trainer(executor=False)
    x = torch.rand(1800, 512, device=DEV)
    lab = torch.tensor([0], device=DEV)
    for _ in range(4):
        for tr in (tr_c, tr_p):
            assert tr.shape_cached("train_step", x, lab) is not None
    torch.cuda.synchronize()
    assert tr_c.last["exec"] is True and tr_p.last["exec"] is False
    _bits_equal(tr_c, tr_p)


# ------------------------------------------------------------------------------------------------------------------ 7
def _fallback_pair(make, n=700, D=512, steps=2, exact=True):
    """What the executor refuses runs the Python path (last["exec"] false), never raises, and is what MHIMX_STEP_EXEC=0 computes."""
    trs = [make(), make()]
    trs[1].use_executor = False
    g = torch.Generator(device=DEV).manual_seed(5)
    for step in range(steps):
        x = torch.randn(n, D, device=DEV, generator=g).abs_()
        lab = torch.tensor([step % 2], device=DEV)
        outs = [tr.train_step(x, lab) for tr in trs]
        for tr in trs:
            assert tr.last["exec"] is False
        assert torch.isfinite(outs[0][0]).all()
        if exact:
            assert torch.equal(outs[0][0], outs[1][0])
        else:
            assert torch.allclose(outs[0][0], outs[1][0], atol=1e-4)
    torch.cuda.synchronize()
    if exact:
        assert torch.equal(trs[0].flat.student, trs[1].flat.student)
    assert torch.isfinite(trs[0].flat.student).all()
    return trs


@limit(300)
def test_fallbacks_take_the_python_path_and_do_not_raise():
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM

    def other(**kw):
        def make():
            torch.manual_seed(3)
            m = MHIM(input_dim=512, n_classes=2, dropout=0.25, merge_enable=False, act="gelu", da_act="relu", **kw).to(DEV).train()
            return FusedTrainer(m, None, lr=1e-3, model="mhim_pure")
        return make

    _fallback_pair(other(baseline="attn", gated=True))                              # a gated student
    _fallback_pair(other(baseline="selfattn"), n=600, exact=False)                  # a TransMIL pure model
    _fallback_pair(lambda: _trainer(clip_grad=1.0))                                 # clipping stays outside the call
    trs = _fallback_pair(lambda: _trainer(accumulation_steps=2), steps=4)           # accumulation windows
    assert trs[0].flat.step == 2
    _fallback_pair(lambda: _trainer(), n=63)                                        # below the one-pass kernels' 64 rows


@limit(300)
def test_a_row_pitch_the_call_refuses_is_never_handed_to_it():
    """A bag whose row pitch is not a multiple of 4 floats: _exec_ok says no (mhimx_pure_step_run would return < 0) - and the trainer's own
    _check_x makes every bag contiguous before any route is chosen, so the step of such a view is the step of its contiguous copy."""
    tr_v, tr_c = _trainer(), _trainer()
    buf = torch.rand(900, 514, device=DEV)
    view = buf[:, :512]
    assert view.stride(0) == 514 and not tr_v._exec_ok(view)
    assert not tr_v.pure_exec_shapes_ok(900, 512, 514, 1, view.data_ptr())
    lab = torch.tensor([1], device=DEV)
    lv, _ = tr_v.train_step(view, lab)
    lc, _ = tr_c.train_step(view.contiguous(), lab)
    assert torch.equal(lv, lc)
    _bits_equal(tr_v, tr_c)
