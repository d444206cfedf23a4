"""The ragged train call of the teacher-free DSMIL model (mhimx_dsmil_window_run, csrc/dsmil_window.hip) under
FusedTrainer(model="mhim_pure") with a DSMIL student: window_step (accumulation_steps > 1) and train_step / forward_backward
(accumulation_steps == 1) against the CPU oracle (per bag O.pure, main_alpha CE(0.5 logits_bag + 0.5 logits_ins) / n backward into shared
leaves, O.adam_step; O.train_step for the single bag), against today's bag-after-bag route of the same build and against itself
(neighbours, ties, determinism, capture, half-precision bags).

Tolerances are tests/test_dsmil_gpu.py's: logits 1e-4 absolute, CE 3e-4, every gradient max error <= 5e-3 max|ref|, after Adam with
tol = 0.1 * 2 * lr: mean error <= 0.1 tol and share of elements above tol < 2e-3.  Moments (the state is the oracle's before every
update, so their error is the current gradient's): m within 5e-3 (1 - beta1) max|g_ref|, v within 1.01e-2 (1 - beta2) max|g_ref|^2
(|g^2 - r^2| <= |g - r| (2 |r| + |g - r|)).

The dropout seeds mix torch.initial_seed() in: it is pinned for every test (_pinned_seed), so a mask is a function of the test alone.
The derivative of the two ReLUs is discontinuous too; what one gate near zero could move is printed (_gate_exposure: why no margin is
asserted).  The arg-max is discontinuous: every oracle comparison first asserts, from the oracle's own instance logits, that in every bag and class
the largest and the second largest differ by more than 1e-3 (the device's instance logits are within ~3e-5 of fp32)."""
import signal

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(act="gelu", da_act="relu", merge_enable=False, baseline="dsmil")
EXEC = "mhimx_dsmil_window_run"
D = 256
SIX, FOUR, THREE = [70, 1, 513, 33, 257, 64], [700, 100, 257, 64], [300, 31, 65]      # bag seeds 300, 320, 340
WI, BI = "online_encoder.i_classifier.0.weight", "online_encoder.i_classifier.0.bias"
LR, B1, B2 = 2e-4, 0.9, 0.999
SEED = 20260319                                                  # torch.manual_seed of every test (the dropout masks hang on it)


@pytest.fixture(autouse=True)
def _pinned_seed():
    """A bag's dropout seed mixes torch.initial_seed() in (MHIM._next_seed): pinned, so that every mask here is a function of the test
    alone and not of what an earlier test of the suite left behind."""
    torch.manual_seed(SEED)


@pytest.fixture(autouse=True)
def _time_limit(request):
    """Every test here carries its own time limit (seconds; ``time_limit`` attribute of the test function, default 120)."""
    limit = int(getattr(request.function, "time_limit", 120))

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


def _base(C=2, d=D):
    return synth.mhim_state(7, input_dim=d, baseline="dsmil", merge_enable=False, n_classes=C)


def _model(C=2, dropout=0.0, d=D, **kw):
    from mhim_mil_amd.mhim import MHIM
    m = MHIM(input_dim=d, n_classes=C, dropout=dropout, **{**CFG, **kw})
    m.load_state_dict({k: torch.as_tensor(v) for k, v in _base(C, d).items()})
    return m.to(DEV).train()


def _trainer(C=2, dropout=0.0, accum=8, executor=True, d=D, model_kw=None, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    tr = FusedTrainer(_model(C, dropout, d, **(model_kw or {})), None, lr=kw.pop("lr", LR), model="mhim_pure", accumulation_steps=accum, **kw)
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


def _bags(sizes, seed, d=D):
    return [torch.from_numpy(synth.bag(seed + j, n, d)) for j, n in enumerate(sizes)]


def _dev(bags, labels):
    return [b.to(DEV) for b in bags], [torch.tensor([y], device=DEV) for y in labels]


def _assert_gap(x, params, mask=None, dropout=0.0):
    """The oracle's own instance logits: largest and second largest of every class more than 1e-3 apart."""
    with torch.no_grad():
        h = O.feature(x, params, "gelu", mask, dropout)
        cl = h @ params[WI].detach().t() + params[BI].detach()
    if cl.shape[0] > 1:
        t = torch.topk(cl, 2, 0).values
        gap = float((t[0] - t[1]).min())
        assert gap > 1e-3, f"arg-max gap {gap:.3e}: change the bag seed"


GATE_DELTA = 1e-5            # a ReLU pre-activation nearer to zero than this may take either side on the device (largest seen: 6e-6)
PB = "online_encoder.b_classifier."


def _gate_exposure(x, y, n, params, mask, dropout, acc):
    """A diagnostic, not a check.  The two ReLUs of the model (V = relu(h Wv^T + bv), U1 = relu(h Wq0^T + bq0)) are discontinuous in
    their derivative like the arg-max, and the device's pre-activations differ from fp32 by a few 1e-6.  Measured over 49 process seeds
    (dropout masks) of test 3 on an MI355X: 38 passed, 1 tripped the arg-max gap assertion, 10 missed the gradient tolerance (0.5 - 2 %
    of scale in v.1.weight or q.0.weight) - and each of those misses was ONE gate with an oracle pre-activation between 1e-6 and 6e-6
    taking the other side: 94 - 100 % of the squared error in one row of the weight gradient, proportional to one bag row's h
    (cosine +-1.00000).  No margin on the gates can be asserted: the issue's own no-dropout sets hold gates within 1e-5 of zero that
    carry up to 2 % of v.1.weight's scale (they do not flip on the device).  So the seed is pinned (_pinned_seed), which makes every
    mask and with it every gate a function of the test alone, and this function prints, per tensor, the most ONE gate with
    |pre-activation| < GATE_DELTA could move a gradient row - |d loss / d out| max|h_row| - so that a miss can be told from a defect.
    A float64 forward of its own, used for this figure only."""
    P = {k: v.detach().double() for k, v in params.items()}
    with torch.no_grad():
        h = O.feature(x.double(), P, "gelu", mask, dropout)
        pv, pu = h @ P[PB + "v.1.weight"].t() + P[PB + "v.1.bias"], h @ P[PB + "q.0.weight"].t() + P[PB + "q.0.bias"]
        cls = h @ P[WI].t() + P[BI]
        crit = cls.argmax(0)
    V, U = torch.relu(pv).requires_grad_(True), torch.relu(pu).requires_grad_(True)
    Q = torch.tanh(U @ P[PB + "q.2.weight"].t() + P[PB + "q.2.bias"])
    A = torch.softmax(Q @ Q[crit].t() / Q.shape[1] ** 0.5, 0)
    lb = torch.einsum("ocv,cv->o", P[PB + "fcc.weight"], A.t() @ V) + P[PB + "fcc.bias"]
    (O.cross_entropy(0.5 * lb + 0.5 * cls.max(0).values, y) / n).backward()
    hmax = h.abs().max(1).values[:, None]
    for key, pre, g in (("v.1", pv, V.grad), ("q.0", pu, U.grad)):
        amb = (pre.abs() < GATE_DELTA).double() * g.abs() * hmax
        acc[key + ".weight"] = max(acc.get(key + ".weight", 0.0), float(amb.max()))


def _report_gates(acc, po):
    for key, worst in acc.items():
        scale = float(po[PB + key].grad.abs().max())
        print(f"  gate exposure {key}: one gate within {GATE_DELTA:g} of zero could move a row by {worst:.3e} ({worst / scale:.2%} of scale)")


def _oracle_window(bags, labels, params, dropout=0.0, masks=None, main_alpha=1.0):
    """Per bag O.pure, (main_alpha CE(mix) / n).backward() into shared leaves.  Returns (leaves with .grad, [mixed logits], [ce])."""
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    cfg = O.Cfg(dropout=dropout, **CFG)
    n = len(bags)
    logits, ces, gates = [], [], {}
    for j, (x, y) in enumerate(zip(bags, labels)):
        mk = None if masks is None else masks[j]
        _assert_gap(x, po, mk, dropout)
        _gate_exposure(x, y, n, po, mk, dropout, gates)
        lb, li = O.pure(x, po, cfg, drop_mask=mk)
        lo = 0.5 * lb + 0.5 * li
        ce = O.cross_entropy(lo, y)
        (main_alpha * ce / n).backward()
        logits.append(lo.detach())
        ces.append(float(ce.detach()))
    _report_gates(gates, po)
    return po, logits, ces


def _check_logits(logits, losses, ref_logits, ref_ces):
    for j in range(len(ref_logits)):
        d = np.abs(logits[j].cpu().numpy().ravel() - ref_logits[j].numpy().ravel()).max()
        print(f"  bag {j}: logits max err {d:.3e}, ce err {abs(float(losses[j][1]) - ref_ces[j]):.3e}")
        np.testing.assert_allclose(logits[j].cpu().numpy().ravel(), ref_logits[j].numpy().ravel(), atol=1e-4, rtol=0)
        assert abs(float(losses[j][1]) - ref_ces[j]) < 3e-4
        assert float(losses[j][2]) == 0.0 and float(losses[j][0]) == float(losses[j][1])       # main_alpha = 1, NOT scaled by 1 / n


def _check_grads(tr, po, what=""):
    gv = tr.flat.grad_views
    seen = 0
    for name, p in po.items():
        if p.grad is None:                                       # (the predictor: no DSMIL route reads it, the flat buffers do not hold it)
            assert name not in gv or float(gv[name].abs().max()) == 0.0, name
            continue
        seen += 1
        g, r = gv[name].cpu().numpy(), p.grad.numpy()
        err, scale = np.abs(g - r.reshape(g.shape)).max(), np.abs(r).max()
        print(f"  {what}grad {name}: max err {err:.3e} of scale {scale:.3e}")
        assert np.isfinite(g).all() and err <= 5e-3 * scale, (name, err, scale)
    assert seen == 12


def _adam(po, opt, step, lr=LR, grads=None):
    stu, new = {}, {}
    for k, p in po.items():
        if p.grad is None:
            stu[k] = p.detach()
            continue
        m, v = opt.get(k, (torch.zeros_like(p), torch.zeros_like(p)))
        pn, m, v = O.adam_step(p.detach(), p.grad if grads is None else grads[k], m, v, step, lr=lr, wd=1e-5)
        stu[k], new[k] = pn, (m, v)
    return stu, new


def _check_after_adam(tr, po, stu_ref, opt_ref, lr=LR, scale_g=1.0, rel=5e-3):
    """Parameters by the project's DSMIL rule; moments by the gradient tolerance ``rel`` carried through (1 - beta) g and (1 - beta2) g^2
    (``scale_g``: what the update multiplied the gradient by)."""
    sd, fl = tr.s.state_dict(), tr.flat
    tol = 0.1 * 2 * lr
    for name, (m_ref, v_ref) in opt_ref.items():
        err = (sd[name].detach().cpu().double() - stu_ref[name].double()).abs()
        print(f"  after Adam {name}: mean err {err.mean().item():.3e}, above tol {(err > tol + 1e-7).double().mean().item():.3e}")
        assert err.mean().item() <= 0.1 * tol + 1e-7, (name, err.mean().item())
        assert (err > tol + 1e-7).double().mean().item() < 2e-3, (name, err.max().item())
        o, n = fl.offsets[name], m_ref.numel()
        gmax = float(po[name].grad.abs().max()) * scale_g
        me = float((fl.m[o:o + n].cpu() - m_ref.reshape(-1)).abs().max())
        ve = float((fl.v[o:o + n].cpu() - v_ref.reshape(-1)).abs().max())
        assert me <= rel * (1 - B1) * gmax + 1e-12, ("m", name, me, gmax)
        assert ve <= (2 * rel + rel * rel) * (1 - B2) * gmax * gmax + 1e-20, ("v", name, ve, gmax)


def _load(tr, stu, opt):
    tr.s.load_state_dict(stu)
    for name, (m_ref, v_ref) in opt.items():
        o = tr.flat.offsets[name]
        tr.flat.m[o:o + m_ref.numel()].copy_(m_ref.reshape(-1))
        tr.flat.v[o:o + v_ref.numel()].copy_(v_ref.reshape(-1))


def _windows_vs_oracle(tr, C, windows, dropout):
    """Every window with update = 0 (the summed gradient inspected in cfg->g) + update(); each one continues from the oracle's state (the
    update inside the call: tests 4, 7, 9).  With dropout the keep-masks are read back from the feature rows (a GELU output is exactly zero
    only where it was dropped)."""
    stu, opt = O.as_torch(_base(C)), {}
    for w, (sizes, seed) in enumerate(windows):
        inside = False
        bags = _bags(sizes, seed)
        labels = [(j + w) % C for j in range(len(sizes))]
        xs, ls = _dev(bags, labels)
        counters = (tr.flat.step, int(tr.tick), int(tr.opt_step), tr.s._step)
        logits, losses = tr.window_step(xs, ls, update=inside)
        torch.cuda.synchronize()
        assert tr.last["exec"] == EXEC and len(logits) == len(losses) == len(sizes)
        assert int(tr.tick) == counters[1] + 1 and int(tr.opt_step) == counters[2] + 1 and tr.s._step == counters[3] + len(sizes)
        assert tr.flat.step == counters[0] + (1 if inside else 0)
        masks = None
        if dropout > 0:
            masks = [(b["H_student"] != 0).cpu() for b in tr.last["bags"]]
            kept = sum(int(m.sum()) for m in masks) / sum(m.numel() for m in masks)
            print(f"  window {w}: kept fraction {kept:.5f} over {sum(m.shape[0] for m in masks)} rows")
            assert sum(m.shape[0] for m in masks) >= 512 and abs(kept - (1 - dropout)) < 5e-3, kept
            for b, m in zip(tr.last["bags"], masks):
                assert not bool((b["dact"][~m.to(DEV)] != 0).any())                 # a dropped element has no gradient path
        po, ref_logits, ref_ces = _oracle_window(bags, labels, stu, dropout, masks)
        _check_logits(logits, losses, ref_logits, ref_ces)
        for j, b in enumerate(tr.last["bags"]):
            assert b["crit"].shape == (C,) and bool(((b["crit"] >= 0) & (b["crit"] < sizes[j])).all())
        if not inside:
            _check_grads(tr, po, f"window {w} ")
            tr.update()
            torch.cuda.synchronize()
            assert tr.flat.step == counters[0] + 1
        stu, opt = _adam(po, opt, w + 1)
        _check_after_adam(tr, po, stu, opt)
        _load(tr, stu, opt)


# ------------------------------------------------------------------------------------------------------------------ 1
def test_two_windows_vs_oracle_without_dropout():
    """Six bags (a shorter window than accumulation_steps = 8, an N = 1 bag), then four."""
    _windows_vs_oracle(_trainer(2, 0.0, accum=8), 2, [(SIX, 300), (FOUR, 320)], 0.0)


# ------------------------------------------------------------------------------------------------------------------ 2
def test_five_classes_vs_oracle():
    _windows_vs_oracle(_trainer(5, 0.0, accum=8), 5, [(THREE, 340)], 0.0)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_dropout_masks_read_back_vs_oracle():
    _windows_vs_oracle(_trainer(2, 0.25, accum=4), 2, [(FOUR, 320)], 0.25)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_single_bag_train_step_vs_oracle_train_step():
    """accumulation_steps = 1, the reference's default: two train_step calls, N = 257 then 700, against O.train_step(model='mhim_pure')."""
    tr = _trainer(2, 0.0, accum=1)
    cfg = O.Cfg(dropout=0.0, **CFG)
    stu, opt = O.as_torch(_base(2)), {}
    for step, (n, seed, y) in enumerate(((257, 322, 1), (700, 320, 0))):
        x = torch.from_numpy(synth.bag(seed, n, D))
        _assert_gap(x, stu)
        prev = {k: v.clone() for k, v in stu.items()}
        stu, _, opt, info = O.train_step(x, y, stu, None, opt, cfg, step + 1, model="mhim_pure", lr=LR)
        logits, losses = tr.train_step(x.to(DEV), torch.tensor([y], device=DEV))
        torch.cuda.synchronize()
        assert tr.last["exec"] == EXEC and logits.shape == (2,) and tr.last["patch_num"] == n
        _check_logits([logits], [losses], [info["logits"]], [info["loss"]])
        po = {k: v.clone().requires_grad_(True) for k, v in prev.items()}            # (the gradients O.train_step used, for the moment bounds)
        lb, li = O.pure(x, po, cfg)
        O.cross_entropy(0.5 * lb + 0.5 * li, y).backward()
        _check_after_adam(tr, po, stu, opt)
        _load(tr, stu, opt)
    assert tr.flat.step == 2 and int(tr.opt_step) == 2 and int(tr.tick) == 2 and tr._micro == 0


def test_forward_backward_leaves_the_gradient_and_shape_cached_captures_the_step():
    tr = _trainer(2, 0.0, accum=1)
    x, y = torch.from_numpy(synth.bag(322, 257, D)), 1
    xs, ls = _dev([x], [y])
    logits, losses = tr.forward_backward(xs[0], ls[0])
    torch.cuda.synchronize()
    assert tr.last["exec"] == EXEC and tr._micro == 1 and tr.flat.step == 0 and int(tr.opt_step) == 1
    po, ref_logits, ref_ces = _oracle_window([x], [y], O.as_torch(_base(2)))
    _check_logits([logits], [losses], ref_logits, ref_ces)
    _check_grads(tr, po)
    tr.update()
    assert tr.flat.step == 1 and tr._micro == 0
    # shape_cached: eager twice, captured on the third visit, replayed after
    tc, te = _trainer(2, 0.25, accum=1), _trainer(2, 0.25, accum=1)
    for visit in range(5):
        out = tc.shape_cached("train_step", xs[0], ls[0])
        assert out is not None and tc.last["exec"] == EXEC, visit
        torch.cuda.synchronize()
        lg = out[0].clone()
        te.s._step = tc.s._step - 1                              # (the seed of the cached step; the tick moves on by itself)
        le, _ = te.train_step(xs[0], ls[0])
        torch.cuda.synchronize()
        assert torch.equal(lg, le), visit
    st = tc._shape_graphs
    assert len(st["graphs"]) == 1 and not st["bad"], st.get("errors")
    assert tc.flat.step == 5 and int(tc.opt_step) == 5
    for name, a, b in zip(("student", "m", "v", "opt_step", "tick"), _state(tc), _state(te)):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------------------------ 5
def test_neighbours_do_not_matter():
    """Bag N = 257 alone, then as the third of four bags, same seed and tick: the same bits.  The call reports every loss unscaled; the
    1 / n scale shows in the gradient: d fcc.bias is the sum of the bags' 0.5 (softmax - onehot) / n, checked for n = 1 and n = 4."""
    x, lab = _dev([torch.from_numpy(synth.bag(322, 257, D))], [1])
    others = _dev(_bags([700, 100, 64], 900), [0, 1, 0])
    got = []
    for where in ("alone", "third of four"):
        tr = _trainer(2, 0.25, accum=4)
        if where == "alone":
            xs, ls, j = x, lab, 0
        else:
            xs, ls, j = others[0][:2] + x + others[0][2:], others[1][:2] + lab + others[1][2:], 2
        tr.tick.fill_(9)
        tr.s._step = 100 - j                                    # bag j draws the seed of position 101 of the model's stream
        tr.window_step(xs, ls, update=False)
        torch.cuda.synchronize()
        assert tr.last["exec"] == EXEC
        b = tr.last["bags"][j]
        got.append({k: b[k].clone() for k in ("logits_bag", "logits_ins", "B", "crit", "H_student", "dact", "logits", "losses")})
        # d fcc.bias = sum_b 0.5 main_alpha (softmax(logits_b) - onehot_b) / n: from the call's own logits, the 1 / n scale of the loss
        n = len(xs)
        want = sum(0.5 * (torch.softmax(bb["logits"].double(), 0) - torch.nn.functional.one_hot(l[0], 2).double()) / n
                   for bb, l in zip(tr.last["bags"], ls))
        g = tr.flat.grad_views["online_encoder.b_classifier.fcc.bias"].double()
        assert float((g - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max())), (where, g, want)
        got[-1]["g_fcc_bias"] = g.clone()
    for k in got[0]:
        if k != "g_fcc_bias":
            assert torch.equal(got[0][k], got[1][k]), k
    assert 0.7 < float((got[0]["H_student"] != 0).float().mean()) < 0.8
    assert float(got[0]["g_fcc_bias"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 6
def test_tie_rule_lowest_row_wins():
    x = torch.from_numpy(synth.bag(77, 200, D))
    tr = _trainer(2, 0.0, accum=2)
    xs, ls = _dev([x], [1])
    tr.window_step(xs, ls, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == EXEC
    crit = tr.last["bags"][0]["crit"].clone()
    c0 = int(crit[0])
    x2 = torch.cat([x, x[c0:c0 + 1]])                             # the class-0 critical row once more, as row 200
    tr2 = _trainer(2, 0.0, accum=2)
    xs2, _ = _dev([x2], [1])
    tr2.window_step(xs2, ls, update=False)
    torch.cuda.synchronize()
    b = tr2.last["bags"][0]
    assert tr2.last["exec"] == EXEC and int(b["crit"][0]) == c0 and int(b["crit"][0]) != 200
    assert torch.isfinite(b["logits"]).all() and torch.isfinite(tr2.flat.grad).all()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_determinism_and_capture():
    sizes = [257, 33, 1, 700]
    xs, ls = _dev(_bags(sizes, 320), [0, 1, 0, 1])
    xs2, ls2 = _dev(_bags(sizes[::-1], 360), [1, 0, 1, 0])
    pair = [_trainer(2, 0.25, accum=4), _trainer(2, 0.25, accum=4)]
    for tr in pair:
        tr.window_step(xs, ls)
        tr.window_step(xs2, ls2)
        assert tr.last["exec"] == EXEC
    torch.cuda.synchronize()
    _bits_equal(pair[0], pair[1], "two trainers")
    assert int(pair[0].tick) == 2 and int(pair[0].opt_step) == 2 and torch.isfinite(pair[0].flat.student).all()
    tr_g, tr_e = _trainer(2, 0.25, accum=4), _trainer(2, 0.25, accum=4)
    snap = _state(tr_g)
    graph = tr_g.capture_window(xs, ls, warmup=1)
    seed_step = tr_g.s._step
    assert tr_g.last["exec"] == EXEC
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
        assert tr_e.last["exec"] == EXEC
    torch.cuda.synchronize()
    for j in range(len(sizes)):
        assert torch.equal(tr_g.last["logits"][j], le[j]) and torch.equal(tr_g.last["losses"][j], se[j])
    for name, a, b in zip(("student", "m", "v", "opt_step", "tick"), _state(tr_g), _state(tr_e)):
        assert torch.equal(a, b), name
    assert int(tr_e.tick) == 3 and int(tr_e.opt_step) == 3 and torch.isfinite(tr_g.flat.student).all()


# ------------------------------------------------------------------------------------------------------------------ 8
def test_dropout_masks_against_todays_route_of_the_same_build():
    """A trainer with use_executor = False, one bag, dropout 0.25, same seed and tick: the keep-masks are bit-equal (the call's projection
    draws the per-element law of ops.gemm_nt's epilogue, which today's route projects through), so the gradients are comparable too."""
    x, lab = _dev([torch.from_numpy(synth.bag(322, 257, D))], [1])
    nat, old = _trainer(2, 0.25, accum=1), _trainer(2, 0.25, accum=1, executor=False)
    seen = {}
    feature = old.s._feature

    def recording(*a, **k):
        r = feature(*a, **k)
        seen["H"] = k["out"]
        return r

    old.s._feature = recording
    nat.forward_backward(x[0], lab[0])
    old.forward_backward(x[0], lab[0])
    torch.cuda.synchronize()
    assert nat.last["exec"] == EXEC and old.last["exec"] is False and nat.s._step == old.s._step and int(nat.tick) == int(old.tick)
    mask_n, mask_o = nat.last["H_student"] != 0, seen["H"] != 0
    print(f"  masks: native keeps {float(mask_n.float().mean()):.4f}, today's route {float(mask_o.float().mean()):.4f}, "
          f"differing share {float((mask_n != mask_o).float().mean()):.4f}")
    assert 0.7 < float(mask_n.float().mean()) < 0.8
    assert mask_n.shape == mask_o.shape and torch.equal(mask_n, mask_o), float((mask_n != mask_o).float().mean())
    _compare_routes(nat, old, "one bag, dropout 0.25")


def test_summed_gradient_against_todays_route_of_the_same_build():
    """A trainer with use_executor = False, no dropout (today's route advances the tick once per bag, the call once per window): one bag, then the four-bag window - the summed gradients within the gradient tolerance; the measured
    differences are printed (profiles/dsmil_window.md records them)."""
    x, lab = _dev([torch.from_numpy(synth.bag(322, 257, D))], [1])
    nat, old = _trainer(2, 0.0, accum=1), _trainer(2, 0.0, accum=1, executor=False)
    nat.forward_backward(x[0], lab[0])
    old.forward_backward(x[0], lab[0])
    torch.cuda.synchronize()
    assert nat.last["exec"] == EXEC and old.last["exec"] is False and nat.s._step == old.s._step and int(nat.tick) == int(old.tick)
    assert torch.allclose(nat.last["logits"], old.last["logits"].view(-1), atol=1e-4, rtol=0)
    _compare_routes(nat, old, "one bag")
    xs, ls = _dev(_bags(FOUR, 320), [0, 1, 0, 1])
    nat, old = _trainer(2, 0.0, accum=4), _trainer(2, 0.0, accum=4, executor=False)
    nat.window_step(xs, ls, update=False)
    for xb, lb in zip(xs, ls):
        old.forward_backward(xb, lb)
    torch.cuda.synchronize()
    assert nat.last["exec"] == EXEC and old.last["exec"] is False
    _compare_routes(nat, old, "four bags")


def _compare_routes(nat, old, what):
    for name in nat._DSMIL_PARAMS:
        a, r = nat.flat.grad_views[name].cpu().numpy(), old.flat.grad_views[name].cpu().numpy()
        err, scale = np.abs(a - r).max(), np.abs(r).max()
        print(f"  [{what}] grad {name}: max difference {err:.3e} of scale {scale:.3e}")
        assert err <= 5e-3 * scale, (name, err, scale)


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_precision_bags_equal_the_fp32_call_on_their_widened_rows(dtype):
    sizes = [100, 33, 257]
    half = [b.to(DEV).to(dtype) for b in _bags(sizes, 320)]
    ls = [torch.tensor([j % 2], device=DEV) for j in range(3)]
    th, tf = _trainer(2, 0.25, accum=3), _trainer(2, 0.25, accum=3)
    lh, sh = th.window_step(half, ls)
    lf, sf = tf.window_step([x.float() for x in half], ls)
    torch.cuda.synchronize()
    assert th.last["exec"] == EXEC and tf.last["exec"] == EXEC and th.last["x_dtype"] == dtype and tf.last["x_dtype"] == torch.float32
    for j in range(3):
        assert torch.equal(lh[j], lf[j]) and torch.equal(sh[j], sf[j])
        for k in ("logits_bag", "logits_ins", "B", "crit", "H_student", "dact"):
            assert torch.equal(th.last["bags"][j][k], tf.last["bags"][j][k]), (j, k)
    _bits_equal(th, tf, str(dtype))
    assert th.flat.step == 1


# ------------------------------------------------------------------------------------------------------------------ 10
def test_clip_grad_runs_the_update_outside_the_call():
    base = O.as_torch(_base(2))
    bags, labels = _bags(FOUR, 320), [1, 0, 1, 0]
    po, _, _ = _oracle_window(bags, labels, base)
    raw = {k: p.grad for k, p in po.items() if p.grad is not None}
    _, total = O.clip_grad_norm(raw, 1.0)
    clip = 0.25 * float(total)                                  # binds
    tr = _trainer(2, 0.0, accum=4, clip_grad=clip)
    xs, ls = _dev(bags, labels)
    tr.window_step(xs, ls)
    torch.cuda.synchronize()
    assert tr.last["exec"] == EXEC and tr.flat.step == 1 and int(tr.opt_step) == 1 and tr._micro == 0
    clipped, _ = O.clip_grad_norm(raw, clip)
    stu, opt = _adam(po, {}, 1, grads=clipped)
    # (the clip factor is clip / ||g||: the device's norm carries the gradient tolerance too, so the clipped gradient carries it twice)
    _check_after_adam(tr, po, stu, opt, scale_g=0.25, rel=1e-2)


# ------------------------------------------------------------------------------------------------------------------ 11
def _fallback_pair(make, sizes, d=D, single=False):
    """What the call does not take runs today's bag-after-bag route (last["exec"] false), never raises and consumes exactly the state a
    trainer with the executor switched off consumes.  ``single``: train_step on the first bag instead of window_step."""
    trs = [make(), make()]
    trs[1].use_executor = False
    xs, ls = _dev(_bags(sizes, 70, d), [j % 2 for j in range(len(sizes))])
    for _ in range(2):
        if single:
            outs = [([o[0]], [o[1]]) for o in (tr.train_step(xs[0], ls[0]) for tr in trs)]
        else:
            outs = [tr.window_step(xs, ls) for tr in trs]
        for tr in trs:
            assert tr.last["exec"] is False
        for a, b in zip(outs[0][0], outs[1][0]):
            assert torch.equal(a, b) and torch.isfinite(a).all()
    torch.cuda.synchronize()
    _bits_equal(trs[0], trs[1])
    assert trs[0].flat.step == 2
    return trs


@limit(300)
def test_fallbacks_do_not_raise_and_do_not_consume_state(monkeypatch):
    sizes = [100, 33, 65, 64]
    _fallback_pair(lambda: _trainer(2, 0.25, accum=4, model_kw={"prec": "f32"}), sizes)      # exact fp32 products
    _fallback_pair(lambda: _trainer(2, 0.25, accum=33), [40 + j for j in range(33)])         # more bags than the table holds
    _fallback_pair(lambda: _trainer(2, 0.25, accum=4, d=320), sizes, d=320)                  # input_dim no multiple of 256

    def capped(**kw):
        tr = _trainer(2, 0.25, **kw)
        tr.dsmil_window_row_cap = 32                                                         # fewer rows than the window / the bag has
        return tr

    tr = _fallback_pair(lambda: capped(accum=4), sizes)[0]                                   # a row cap below the window
    xs, ls = _dev(_bags(sizes, 70), [0, 1, 0, 1])
    assert not tr._dsmil_window_ok(xs, ls)
    with pytest.raises(AssertionError):                                                      # a SHORT window cannot fall back (1 / accumulation_steps)
        tr.window_step(xs[:2], ls[:2])
    _fallback_pair(lambda: _trainer(2, 0.25, accum=1, model_kw={"prec": "f32"}), sizes, single=True)   # the single-bag step falls back alike
    _fallback_pair(lambda: capped(accum=1), sizes, single=True)
    monkeypatch.setenv("MHIMX_STEP_EXEC", "0")
    trs = _fallback_pair(lambda: _trainer(2, 0.25, accum=4), sizes)
    assert trs[0].use_executor is False
