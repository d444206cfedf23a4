"""The ragged accumulation window of the teacher-free ABMIL model (mhimx_pure_window_run, csrc/pure_window.hip) under
FusedTrainer(model="mhim_pure", accumulation_steps=k).window_step: against the CPU oracle (per bag O.pure, main_alpha CE / n backward into
shared leaves, O.adam_step), against the single-bag call (masks, summed gradients) and against itself (neighbours, determinism, capture).
Tolerances are tests/test_pure_step_gpu.py's (_check_against / _check_after_adam): logits 1e-4 absolute, CE 3e-4, every gradient
atol = 2e-3 max|ref|, rtol = 2e-3, parameters after Adam mean <= 3e-6 and max <= 4.1e-4 per step, moments like gradients."""
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


def _trainer(D=512, dropout=0.25, accum=8, executor=True, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    tr = FusedTrainer(_model(D, dropout), None, lr=kw.pop("lr", 2e-4), model="mhim_pure", accumulation_steps=accum, **kw)
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


def _bags(sizes, D, seed=300):
    return [torch.from_numpy(synth.bag(seed + j, n, D)) for j, n in enumerate(sizes)]


def _dev(bags, labels):
    return [b.to(DEV) for b in bags], [torch.tensor([y], device=DEV) for y in labels]


def _oracle_window(bags, labels, params, dropout=0.0, masks=None, main_alpha=1.0):
    """Per bag O.pure, (main_alpha CE / n).backward() into shared leaves.  Returns (leaves with .grad, [logits], [ce])."""
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    cfg = O.Cfg(dropout=dropout, **CFG)
    n = len(bags)
    logits, ces = [], []
    for j, (x, y) in enumerate(zip(bags, labels)):
        lo = O.pure(x, po, cfg, drop_mask=None if masks is None else masks[j])
        ce = O.cross_entropy(lo, y)
        (main_alpha * ce / n).backward()
        logits.append(lo.detach())
        ces.append(float(ce.detach()))
    return po, logits, ces


def _check_window(tr, po, logits, losses, ref_logits, ref_ces):
    for j in range(len(ref_logits)):
        d = np.abs(logits[j].cpu().numpy().ravel() - ref_logits[j].numpy().ravel()).max()
        print(f"  bag {j}: logits max err {d:.3e}, ce err {abs(float(losses[j][1]) - ref_ces[j]):.3e}")
        np.testing.assert_allclose(logits[j].cpu().numpy().ravel(), ref_logits[j].numpy().ravel(), atol=1e-4, rtol=0)
        assert abs(float(losses[j][1]) - ref_ces[j]) < 3e-4
        assert float(losses[j][2]) == 0.0 and float(losses[j][0]) == float(losses[j][1])       # main_alpha = 1, NOT scaled by 1 / n
    gv = tr.flat.grad_views
    assert set(po) == set(gv)
    for name, p in po.items():
        g, r = gv[name].cpu().numpy(), p.grad.numpy()
        print(f"  grad {name}: max err {np.abs(g - r.reshape(g.shape)).max():.3e} of scale {np.abs(r).max():.3e}")
        np.testing.assert_allclose(g, r.reshape(g.shape), atol=2e-3 * (np.abs(r).max() + 1e-30), rtol=2e-3, err_msg=name)


def _adam(po, opt, step, lr=2e-4):
    stu, new = {}, {}
    for k, p in po.items():
        m, v = opt.get(k, (torch.zeros_like(p), torch.zeros_like(p)))
        pn, m, v = O.adam_step(p.detach(), p.grad, m, v, step, lr=lr, wd=1e-5)
        stu[k], new[k] = pn, (m, v)
    return stu, new


def _check_after_adam(tr, stu_ref, opt_ref, step):
    sd, fl = tr.s.state_dict(), tr.flat
    for name, ref in stu_ref.items():
        err = (sd[name].detach().cpu().double() - ref.double()).abs()
        print(f"  after Adam {name}: mean err {err.mean().item():.3e}, max {err.max().item():.3e}")
        assert err.mean().item() <= 3e-6 and err.max().item() <= 4.1e-4 * (step + 1), (step, name, err.mean().item(), err.max().item())
    for name, (m_ref, v_ref) in opt_ref.items():
        o, n = fl.offsets[name], m_ref.numel()
        for what, got, ref in (("m", fl.m[o:o + n], m_ref), ("v", fl.v[o:o + n], v_ref)):
            r = ref.numpy().ravel()
            np.testing.assert_allclose(got.cpu().numpy(), r, atol=2e-3 * (np.abs(r).max() + 1e-30), rtol=2e-3, err_msg=f"{what} {name} step {step}")


def _load(tr, stu, opt):
    tr.s.load_state_dict(stu)
    for name, (m_ref, v_ref) in opt.items():
        o = tr.flat.offsets[name]
        tr.flat.m[o:o + m_ref.numel()].copy_(m_ref.reshape(-1))
        tr.flat.v[o:o + v_ref.numel()].copy_(v_ref.reshape(-1))


def _two_windows_vs_oracle(tr, D, sizes1, sizes2, dropout):
    """Window 1 with update = 0 (gradients inspected) + update(), window 2 with the update inside the call, continuing from the oracle's
    state.  With dropout the keep-masks are read back from the feature rows (a GELU output is exactly zero only where it was dropped)."""
    base = O.as_torch(synth.mhim_state(7, input_dim=D, merge_enable=False))
    stu, opt = base, {}
    for w, sizes in enumerate((sizes1, sizes2)):
        bags = _bags(sizes, D, seed=300 + 50 * w)
        labels = [(j + w) % 2 for j in range(len(sizes))]
        xs, ls = _dev(bags, labels)
        counters = (tr.flat.step, int(tr.tick), int(tr.opt_step), tr.s._step)
        logits, losses = tr.window_step(xs, ls, update=(w == 1))
        torch.cuda.synchronize()
        assert tr.last["exec"] is True and len(logits) == len(losses) == len(sizes)
        assert int(tr.tick) == counters[1] + 1 and int(tr.opt_step) == counters[2] + 1 and tr.s._step == counters[3] + len(sizes)
        assert tr.flat.step == counters[0] + (1 if w == 1 else 0)
        masks = None
        if dropout > 0:
            masks = [(b["H_student"] != 0).cpu() for b in tr.last["bags"]]
            kept = sum(int(m.sum()) for m in masks) / sum(m.numel() for m in masks)
            print(f"  window {w}: kept fraction {kept:.5f} over {sum(m.numel() for m in masks)} elements")
            assert sum(m.shape[0] for m in masks) >= 512 and abs(kept - (1 - dropout)) < 5e-3, kept
            for b, m in zip(tr.last["bags"], masks):
                assert not bool((b["dact"][~m.to(DEV)] != 0).any())                 # a dropped element has no gradient path
        po, ref_logits, ref_ces = _oracle_window(bags, labels, stu, dropout, masks)
        if w == 0:
            _check_window(tr, po, logits, losses, ref_logits, ref_ces)
            tr.update()
            torch.cuda.synchronize()
            assert tr.flat.step == counters[0] + 1
        else:
            for j in range(len(sizes)):
                np.testing.assert_allclose(logits[j].cpu().numpy().ravel(), ref_logits[j].numpy().ravel(), atol=1e-4, rtol=0)
                assert abs(float(losses[j][1]) - ref_ces[j]) < 3e-4
        stu, opt = _adam(po, opt, w + 1)
        _check_after_adam(tr, stu, opt, w)
        _load(tr, stu, opt)


# ------------------------------------------------------------------------------------------------------------------ 1
@limit(900)
def test_ragged_window_vs_oracle_without_dropout():
    sizes = [1, 31, 33, 160, 257, 700, 2999, 16385]
    rng = np.random.RandomState(11)
    s1, s2 = list(rng.permutation(sizes)), list(rng.permutation(sizes))
    _two_windows_vs_oracle(_trainer(512, dropout=0.0), 512, [int(v) for v in s1], [int(v) for v in s2], 0.0)


# ------------------------------------------------------------------------------------------------------------------ 2
@limit(900)
def test_c1_window_and_a_ragged_window_with_dropout_vs_oracle():
    _two_windows_vs_oracle(_trainer(1024, dropout=0.25), 1024, [512] * 8, [70, 1, 513, 33, 200, 31, 900, 64], 0.25)


# ------------------------------------------------------------------------------------------------------------------ 3
@limit(300)
def test_a_bags_mask_is_the_single_bag_calls_mask():
    """Same seed, same tick value: mhimx_pure_step_run draws, element for element, the keep-mask the window drew for that bag."""
    D, sizes = 512, [64, 700, 33, 2999, 257, 1]
    tr = _trainer(D, dropout=0.25, accum=6)
    one = _trainer(D, dropout=0.25, accum=1)
    xs, ls = _dev(_bags(sizes, D), [0, 1] * 3)
    tr.tick.fill_(5)
    step0 = tr.s._step
    tr.window_step(xs, ls)
    torch.cuda.synchronize()
    assert tr.last["exec"] is True and int(tr.tick) == 6
    for j in (0, 1, 3):
        mask_w = (tr.last["bags"][j]["H_student"] != 0).clone()
        one.tick.fill_(5)
        one.s._step = step0 + j
        one.forward_backward(xs[j], ls[j])
        torch.cuda.synchronize()
        assert one.last["exec"] is True and int(one.tick) == 6
        mask_1 = one.last["H_student"] != 0
        assert mask_w.shape == mask_1.shape and torch.equal(mask_w, mask_1), (j, float((mask_w != mask_1).float().mean()))
        assert 0.7 < float(mask_w.float().mean()) < 0.8
        one._micro = 0
        one.flat.grad.zero_()


# ------------------------------------------------------------------------------------------------------------------ 4
@limit(300)
def test_neighbours_do_not_matter():
    """A bag's logits, losses, feature rows and d out / d pre rows: the same bits as first of 2, last of 8 and alone."""
    D = 512
    x = torch.from_numpy(synth.bag(42, 777, D)).to(DEV)
    lab = torch.tensor([1], device=DEV)
    others = _dev(_bags([31, 160, 257, 700, 1, 2999, 64], D), [0, 1, 0, 1, 0, 1, 0])
    got = []
    for where in ("first of 2", "last of 8", "alone"):
        tr = _trainer(D, dropout=0.25)
        if where == "first of 2":
            xs, ls, j = [x, others[0][3]], [lab, others[1][3]], 0
        elif where == "last of 8":
            xs, ls, j = others[0] + [x], others[1] + [lab], 7
        else:
            xs, ls, j = [x], [lab], 0
        tr.tick.fill_(9)
        tr.s._step = 100 - j                                    # bag j draws the seed of position 101 of the model's stream
        tr.window_step(xs, ls, update=False)
        torch.cuda.synchronize()
        assert tr.last["exec"] is True
        b = tr.last["bags"][j]
        got.append([b["logits"].clone(), b["losses"].clone(), b["H_student"].clone(), b["dact"].clone()])
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert torch.equal(a, b)
    assert float((got[0][2] != 0).float().mean()) < 0.8


# ------------------------------------------------------------------------------------------------------------------ 5
@limit(420)
def test_determinism_and_capture():
    D, sizes = 512, [700, 33, 1, 2999, 257, 160, 31, 512]
    xs, ls = _dev(_bags(sizes, D), [0, 1] * 4)
    grads = []
    for _ in range(2):
        tr = _trainer(D, dropout=0.25)
        tr.window_step(xs, ls, update=False)
        torch.cuda.synchronize()
        assert tr.last["exec"] is True
        grads.append(tr.flat.grad.clone())
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0 and torch.isfinite(grads[0]).all()
    tr_g, tr_e = _trainer(D, dropout=0.25), _trainer(D, dropout=0.25)
    snap = _state(tr_g)
    graph = tr_g.capture_window(xs, ls, warmup=1)
    seed_step = tr_g.s._step
    assert tr_g.last["exec"] is True
    fl = tr_g.flat
    fl.student.copy_(snap[0]); fl.m.copy_(snap[1]); fl.v.copy_(snap[2]); tr_g.opt_step.copy_(snap[3]); tr_g.tick.copy_(snap[4])
    fl.grad.zero_()
    tr_g.last["ws"].fill_(255)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for _ in range(3):
        tr_e.s._step = seed_step - len(sizes)                   # (the seeds the capture baked; the tick moves on by itself)
        le, se = tr_e.window_step(xs, ls)
        assert tr_e.last["exec"] is True
    torch.cuda.synchronize()
    for j in range(len(sizes)):
        assert torch.equal(tr_g.last["logits"][j], le[j]) and torch.equal(tr_g.last["losses"][j], se[j])
    for name, a, b in zip(("student", "m", "v", "opt_step", "tick"), _state(tr_g), _state(tr_e)):
        assert torch.equal(a, b), name
    assert int(tr_e.tick) == 3 and int(tr_e.opt_step) == 3 and torch.isfinite(tr_g.flat.student).all()


# ------------------------------------------------------------------------------------------------------------------ 6
@limit(420)
def test_summed_gradient_against_the_single_bag_call():
    """Dropout 0, 4 x 10 000 x 1024: the window's gradient vs the sum of mhimx_pure_step_run(update = 0) gradients / n (other tiles, so
    the gradient tolerance, not bits)."""
    D, n, N = 1024, 4, 10000
    g = torch.Generator(device=DEV).manual_seed(3)
    xs = [torch.randn(N, D, device=DEV, generator=g).abs_() for _ in range(n)]
    ls = [torch.tensor([j % 2], device=DEV) for j in range(n)]
    tr = _trainer(D, dropout=0.0, accum=n)
    tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] is True
    one = _trainer(D, dropout=0.0, accum=1)
    ref = torch.zeros_like(one.flat.grad)
    for x, l in zip(xs, ls):
        one._micro = 0
        one.flat.grad.zero_()
        one.forward_backward(x, l)
        torch.cuda.synchronize()
        assert one.last["exec"] is True
        ref += one.flat.grad
    ref /= n
    for name in tr.flat.grad_views:
        o, cnt = tr.flat.offsets[name], tr.flat.grad_views[name].numel()
        a, r = tr.flat.grad[o:o + cnt].cpu().numpy(), ref[o:o + cnt].cpu().numpy()
        print(f"  grad {name}: max err {np.abs(a - r).max():.3e} of scale {np.abs(r).max():.3e}")
        np.testing.assert_allclose(a, r, atol=2e-3 * (np.abs(r).max() + 1e-30), rtol=2e-3, err_msg=name)


# ------------------------------------------------------------------------------------------------------------------ 7
@limit(600)
@pytest.mark.parametrize("sizes,accum", [([700], 8), ([1], 8), ([3, 5], 2), ([3, 5], 8), ([40, 900, 33], 8)])
def test_one_bag_tiny_and_short_last_windows_vs_oracle(sizes, accum):
    """n = 1, row spaces of 32 and 64 rows, and windows shorter than accumulation_steps (the tail of an epoch): scaled by 1 / len(bags)."""
    D = 512
    tr = _trainer(D, dropout=0.0, accum=accum)
    bags = _bags(sizes, D, seed=900)
    labels = [j % 2 for j in range(len(sizes))]
    xs, ls = _dev(bags, labels)
    logits, losses = tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] is True
    base = O.as_torch(synth.mhim_state(7, input_dim=D, merge_enable=False))
    po, ref_logits, ref_ces = _oracle_window(bags, labels, base)
    _check_window(tr, po, logits, losses, ref_logits, ref_ces)
    tr.update()
    torch.cuda.synchronize()
    stu, opt = _adam(po, {}, 1)
    _check_after_adam(tr, stu, opt, 0)
    assert tr.flat.step == 1 and int(tr.opt_step) == 1 and int(tr.tick) == 1


# ------------------------------------------------------------------------------------------------------------------ 8
@limit(300)
def test_clip_grad_runs_the_update_outside_the_call():
    D, sizes = 512, [700, 33, 257, 1]
    base = O.as_torch(synth.mhim_state(7, input_dim=D, merge_enable=False))
    bags = _bags(sizes, D, seed=500)
    labels = [1, 0, 1, 0]
    po, _, _ = _oracle_window(bags, labels, base)
    _, total = O.clip_grad_norm({k: p.grad for k, p in po.items()}, 1.0)
    clip = 0.25 * total                                         # binds
    tr = _trainer(D, dropout=0.0, accum=4, clip_grad=clip)
    xs, ls = _dev(bags, labels)
    tr.window_step(xs, ls)
    torch.cuda.synchronize()
    assert tr.last["exec"] is True and tr.flat.step == 1 and int(tr.opt_step) == 1
    clipped, _ = O.clip_grad_norm({k: p.grad for k, p in po.items()}, clip)
    stu, opt = {}, {}
    for k, p in po.items():
        pn, m, v = O.adam_step(p.detach(), clipped[k], torch.zeros_like(p), torch.zeros_like(p), 1, lr=2e-4, wd=1e-5)
        stu[k], opt[k] = pn, (m, v)
    _check_after_adam(tr, stu, opt, 0)


# ------------------------------------------------------------------------------------------------------------------ 9
def _fallback_pair(make, sizes, D=512):
    """What the window call does not take runs today's bag-after-bag route (last["exec"] false), never raises and consumes exactly the
    state a trainer with the executor switched off consumes."""
    trs = [make(), make()]
    trs[1].use_executor = False
    xs, ls = _dev(_bags(sizes, D, seed=70), [j % 2 for j in range(len(sizes))])
    for _ in range(2):
        outs = [tr.window_step(xs, ls) for tr in trs]
        for tr in trs:
            assert tr.last["exec"] is False
        for a, b in zip(outs[0][0], outs[1][0]):
            assert torch.equal(a, b) and torch.isfinite(a).all()
    torch.cuda.synchronize()
    _bits_equal(trs[0], trs[1])
    assert trs[0].flat.step == 2
    return trs


@limit(420)
def test_fallbacks_do_not_raise_and_do_not_consume_state(monkeypatch):
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM

    def other(accum=4, **kw):
        def make():
            torch.manual_seed(3)
            m = MHIM(input_dim=512, n_classes=2, dropout=0.25, merge_enable=False, act="gelu", da_act="relu", **kw).to(DEV).train()
            return FusedTrainer(m, None, lr=1e-3, model="mhim_pure", accumulation_steps=accum)
        return make

    sizes = [700, 100, 257, 64]
    _fallback_pair(other(baseline="attn", gated=True), sizes)                       # a gated student
    _fallback_pair(other(baseline="attn", prec="f32"), sizes)                       # exact fp32 products
    _fallback_pair(lambda: _trainer(accum=33), [64 + j for j in range(33)])         # more bags than the table holds
    tr = _trainer(accum=4)
    tr.pure_window_row_cap = 512                                                    # more rows than the trainer's cap
    xs, ls = _dev(_bags(sizes, 512), [0, 1, 0, 1])
    assert not tr._pure_window_ok(xs, ls)
    tr.window_step(xs, ls)
    assert tr.last["exec"] is False and tr.flat.step == 1
    with pytest.raises(AssertionError):                                             # a SHORT window cannot fall back (1 / accumulation_steps)
        tr.window_step(xs[:2], ls[:2])
    monkeypatch.setenv("MHIMX_STEP_EXEC", "0")
    trs = _fallback_pair(lambda: _trainer(accum=4), sizes)
    assert trs[0].use_executor is False


@limit(300)
def test_a_row_pitch_the_call_refuses_is_never_handed_to_it():
    """Bags whose row pitch is not a multiple of 4 floats: the mirrored check says no (mhimx_pure_window_run would return < 0 and name the
    bag) - and _check_x makes every bag contiguous before any route is chosen, so the window of such views is the window of their copies."""
    tr_v, tr_c = _trainer(accum=2), _trainer(accum=2)
    views = [torch.rand(n, 514, device=DEV)[:, :512] for n in (900, 33)]
    ls = [torch.tensor([1], device=DEV), torch.tensor([0], device=DEV)]
    assert views[0].stride(0) == 514 and not tr_v._pure_window_ok(views, ls)
    lv, _ = tr_v.window_step(views, ls)
    lc, _ = tr_c.window_step([v.contiguous() for v in views], ls)
    assert tr_v.last["exec"] is True and all(torch.equal(a, b) for a, b in zip(lv, lc))
    _bits_equal(tr_v, tr_c)
