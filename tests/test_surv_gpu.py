"""Survival validation on the GPU (csrc/surv.hip): ops.cindex against the O(n^2) pair definition of tests/surv_oracle.py (all five
outputs bit-equal: the counts are integers and the index is one correctly rounded fp64 division of exact operands), ops.surv_nll against
the fp64 restatement of the reference's formulas, NLLSurvLoss as a criterion, and validate.surv_validate.

The tolerance of the survival head is computed inside the tests: the deviation of the SAME restatement run in torch fp32 on the CPU from
its fp64 run on the test's inputs, times 4 (fp32 sums of <= 16 terms in another order), with an absolute floor of 1e-6.

The data helpers touch no device and every oracle result is computed once and shared."""
import functools
import types

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from tests import surv_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGIT_TOL = 1e-4                      # tests/test_infer_gpu.py, tests/test_infer_dsmil_gpu.py: the inference calls' logit bound
BOOT_SEED = 7784414403328510413       # engines/metrics.py:154


def _ops():
    from mhim_mil_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ 1. the concordance index
CI_SIZES = (2, 255, 256, 257, 1023, 1025, 1500)          # the i-block (256) and j-tile (1024) edges


@functools.lru_cache(maxsize=None)
def ci_data(n, kind):
    """(event, time, risk) of n samples, about half of them events.  'free': distinct times and distinct risks; 'heavy': integer times
    from a small range (events and censored samples share times) and risks on a coarse grid; 'grid': risks on a 4e-9 grid around 0, so
    that tied_tol = 1e-8 decides - differences of 4e-9 and 8e-9 are ties, 1.2e-8 and more are not, nothing lies on the boundary."""
    rng = np.random.default_rng(1000 * n + len(kind))
    event = rng.random(n) < 0.5
    if kind == "free":
        time = (rng.permutation(n) + 0.25).astype(np.float64)
        risk = (rng.permutation(n).astype(np.float32) - n / 2) / np.float32(8.0)
    else:
        time = rng.integers(0, max(2, n // 4), n).astype(np.float64)
        risk = (rng.integers(-3, 4, n) * 0.25).astype(np.float32) if kind == "heavy" else (rng.integers(-3, 4, n) * 4e-9).astype(np.float32)
    if n == 2:
        time = np.array([1.0, 2.0])
    risk = risk.astype(np.float32)
    event[int(np.argmin(time))] = True                   # (the earliest sample is an event: n >= 2 distinct times have a comparable pair)
    assert event.mean() >= 0.3 or n == 2
    for a in (event, time, risk):
        a.setflags(write=False)
    return event, time, risk


def boot_idx(n, B, fold=0):
    from mhim_mil_amd.validate import bootstrap_indices
    return bootstrap_indices(n, B, fold + BOOT_SEED, "cpu")


@functools.lru_cache(maxsize=None)
def ci_reference(n, kind, B):
    """The oracle's [B, 5] for ci_data(n, kind): B = 1 the set itself, B > 1 the resamples the reference draws.  Computed once."""
    event, time, risk = ci_data(n, kind)
    if B == 1:
        rows = [SO.as_row(SO.cindex_pairs(event, time, risk))]
    else:
        idx = boot_idx(n, B).numpy()
        rows = [SO.as_row(SO.cindex_pairs(event[i], time[i], risk[i])) for i in idx]
    out = np.stack(rows)
    out.setflags(write=False)
    return out


def _dev(event, time, risk):
    return (torch.from_numpy(np.ascontiguousarray(event)).to(DEV), torch.from_numpy(np.ascontiguousarray(time)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(risk)).to(DEV))


def _bit_equal(got, ref, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == ref.shape, what
    assert np.array_equal(got, ref, equal_nan=True), (what, got[:3], ref[:3])


@pytest.mark.parametrize("kind", ["free", "heavy"])
@pytest.mark.parametrize("n", CI_SIZES)
def test_cindex_equals_the_pair_definition(n, kind):
    ev, tm, rk = _dev(*ci_data(n, kind))
    ref = ci_reference(n, kind, 1)
    assert not np.isnan(ref).any()
    _bit_equal(_ops().cindex(ev, tm, rk), ref, (n, kind, 1))
    if n >= 30:
        refB = ci_reference(n, kind, 25)
        assert not np.isnan(refB).any()                   # no resample lacks a comparable pair
        _bit_equal(_ops().cindex(ev, tm, rk, sample_idx=boot_idx(n, 25).to(DEV)), refB, (n, kind, 25))


def test_cindex_where_tied_tol_decides():
    n = 257
    event, time, risk = ci_data(n, "grid")
    d = np.abs(risk[:, None] - risk[None, :])
    assert ((d < 9e-9) | (d > 1.1e-8)).all() and (d > 1.1e-8).any() and ((d > 3e-9) & (d < 9e-9)).any()
    ref = ci_reference(n, "grid", 1)
    assert ref[0, 3] > 0 and ref[0, 1] > 0 and ref[0, 2] > 0
    ev, tm, rk = _dev(event, time, risk)
    _bit_equal(_ops().cindex(ev, tm, rk), ref, "grid")
    _bit_equal(_ops().cindex(ev, tm, rk, sample_idx=boot_idx(n, 25).to(DEV)), ci_reference(n, "grid", 25), "grid B=25")
    # a tolerance of 0 counts only equal risks as tied
    ref0 = SO.as_row(SO.cindex_pairs(event, time, risk, tied_tol=0.0))[None]
    assert ref0[0, 3] < ref[0, 3]
    _bit_equal(_ops().cindex(ev, tm, rk, tied_tol=0.0), ref0, "grid tol 0")


def test_cindex_without_a_comparable_pair_is_nan_with_zero_counts():
    nan_row = np.array([[np.nan, 0, 0, 0, 0]])
    one = _dev(np.array([True]), np.array([3.0]), np.array([0.5], np.float32))
    _bit_equal(_ops().cindex(*one), nan_row, "n = 1")
    event, time, risk = ci_data(300, "heavy")
    ev, tm, rk = _dev(np.zeros(300, bool), time, risk)
    assert np.isnan(SO.cindex_pairs(np.zeros(300, bool), time, risk)["cindex"])
    _bit_equal(_ops().cindex(ev, tm, rk), nan_row, "all censored")
    _bit_equal(_ops().cindex(ev, tm, rk, sample_idx=boot_idx(300, 3).to(DEV)), np.repeat(nan_row, 3, 0), "all censored, B = 3")


def test_cindex_is_deterministic_and_capturable():
    n, B = 1025, 25
    ev, tm, rk = _dev(*ci_data(n, "heavy"))
    idx = boot_idx(n, B).to(DEV)
    a = _ops().cindex(ev, tm, rk, sample_idx=idx)
    b = _ops().cindex(ev, tm, rk, sample_idx=idx)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                             # one stream, no parallel branches
        out = _ops().cindex(ev, tm, rk, sample_idx=idx)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), a.view(torch.int64))
    _bit_equal(out, ci_reference(n, "heavy", B), "replay")


# ------------------------------------------------------------------------------------------------ 2. the survival head
NLL_K, NLL_N, G_SCALE = (1, 4, 16), (1, 63, 64, 65, 257), 0.5


@functools.lru_cache(maxsize=None)
def nll_data(n, K):
    """(logits [n, K] fp32, Y, c): random logits of scale 2, every bin and both censorship values; with n >= 63 row 0 is all +40 and
    censored in the last bin (its survival value underflows eps: the S clamp), row 1 all -40 and uncensored in bin 0 (its hazard
    underflows eps: the h clamp; S_pad[0] is the constant 1) - the whole gradient row of either is exactly 0 - and rows 2, 3 carry
    Y = 0 and Y = K - 1."""
    g = torch.Generator().manual_seed(17 * n + K)
    logits = 2.0 * torch.randn(n, K, generator=g)
    Y = torch.randint(0, K, (n,), generator=g)
    c = torch.randint(0, 2, (n,), generator=g).float()
    if n >= 63:
        logits[0], Y[0], c[0] = 40.0, K - 1, 1.0
        logits[1], Y[1], c[1] = -40.0, 0, 0.0
        Y[2], Y[3] = 0, K - 1
        c[2:6] = torch.tensor([0.0, 0.0, 1.0, 1.0])
        Y[4], Y[5] = 0, K - 1
    m = SO.clamp_margins(logits, Y)
    assert ((m - 1).abs() > 1e-3).all(), "a clamped quantity within 1e-3 of eps: fp32 and fp64 could take different sides"
    return logits, Y, c


@functools.lru_cache(maxsize=None)
def nll_reference(n, K, alpha):
    """fp64 (risk, losses, gradient of G_SCALE * sum losses) of the restatement and the bound per quantity: 4 x the deviation of the
    same restatement in torch fp32 on the CPU from the fp64 run, floor 1e-6."""
    logits, Y, c = nll_data(n, K)
    out = {}
    for dt in (torch.float64, torch.float32):
        lg = logits.to(dt).clone().requires_grad_(True)
        risk, losses = SO.nll_surv(lg, Y, c, alpha=alpha)
        (G_SCALE * losses.sum()).backward()
        out[dt] = [t.detach().double().numpy() for t in (risk, losses, lg.grad)]
    bound = [max(4.0 * float(np.abs(a - b).max()), 1e-6) for a, b in zip(out[torch.float32], out[torch.float64])]
    return out[torch.float64], bound


@pytest.mark.parametrize("alpha", [0.0, 0.4])
@pytest.mark.parametrize("K", NLL_K)
@pytest.mark.parametrize("n", NLL_N)
def test_surv_nll_against_the_fp64_restatement(n, K, alpha):
    logits, Y, c = nll_data(n, K)
    (r_risk, r_loss, r_g), bound = nll_reference(n, K, alpha)
    pitched = torch.full((n, K + 3), float("nan"), device=DEV)
    pitched[:, :K] = logits.to(DEV)
    for lg in (logits.to(DEV), pitched[:, :K]):
        risk, losses, g = _ops().surv_nll(lg, Y.to(DEV), c.to(DEV), alpha=alpha, g_scale=G_SCALE)
        assert g.shape == (n, K) and g.is_contiguous()
        dev = [float(np.abs(t.double().cpu().numpy() - r).max()) for t, r in zip((risk, losses, g), (r_risk, r_loss, r_g))]
        print(f"surv_nll n={n} K={K} alpha={alpha} ld={lg.stride(0)}: |risk| {dev[0]:.3e} (bound {bound[0]:.3e})  |loss| {dev[1]:.3e} "
              f"(bound {bound[1]:.3e})  |grad| {dev[2]:.3e} (bound {bound[2]:.3e})")
        for d, b, what in zip(dev, bound, ("risk", "losses", "g_logits")):
            assert d <= b, (what, d, b)
        if n >= 63:
            assert (r_g[:2] == 0).all() and (g[:2] == 0).all()           # both clamps engaged: the gradient is exactly 0
            assert abs(float(losses[0]) + (1 - alpha) * np.log(1e-7)) < 1e-5 and abs(float(losses[1]) + np.log(1e-7)) < 1e-5
        r2, l2 = _ops().surv_nll(lg, Y.to(DEV), c.to(DEV), alpha=alpha)   # without the gradient: the same forward
        assert torch.equal(r2, risk) and torch.equal(l2, losses)


def test_surv_nll_out_of_range_bin():
    logits, Y, c = nll_data(65, 4)
    Y = Y.clone()
    Y[7], Y[9] = -1, 4
    risk, losses, g = _ops().surv_nll(logits.to(DEV), Y.to(DEV), c.to(DEV), g_scale=1.0)
    ok = torch.ones(65, dtype=torch.bool)
    ok[[7, 9]] = False
    assert torch.isnan(losses.cpu()[~ok]).all() and torch.isfinite(losses.cpu()[ok]).all()
    assert (g.cpu()[~ok] == 0).all() and torch.isfinite(risk).all()
    r0, l0, g0 = _ops().surv_nll(logits.to(DEV), nll_data(65, 4)[1].to(DEV), c.to(DEV), g_scale=1.0)
    assert torch.equal(r0, risk) and torch.equal(l0.cpu()[ok], losses.cpu()[ok]) and torch.equal(g0.cpu()[ok], g.cpu()[ok])


# ------------------------------------------------------------------------------------------------ 3. the criterion
def test_nll_surv_loss_backward_is_the_kernels_gradient():
    from mhim_mil_amd.survival import NLLSurvLoss
    n, K = 65, 4
    logits, Y, c = nll_data(n, K)
    for alpha in (0.0, 0.4):
        lg = logits.to(DEV).requires_grad_(True)
        loss = NLLSurvLoss(alpha=alpha)(Y=Y.to(DEV), c=c.to(DEV), logits=lg)
        loss.backward()
        _, losses, g = _ops().surv_nll(logits.to(DEV), Y.to(DEV), c.to(DEV), alpha=alpha, g_scale=1.0 / n)
        assert torch.equal(lg.grad, g) and torch.equal(loss.detach(), losses.mean())
        # the reference's validation form (given hazards and curve): the same loss within the head's bound
        (_, r_loss, _), bound = nll_reference(n, K, alpha)
        h = torch.sigmoid(logits.to(DEV))
        other = NLLSurvLoss(alpha=alpha)(hazards=h, S=torch.cumprod(1 - h, dim=1), Y=Y.to(DEV), c=c.to(DEV))
        assert abs(float(other) - float(loss)) <= bound[1] and abs(float(loss) - r_loss.mean()) <= bound[1]
        assert float(NLLSurvLoss(alpha=0.9)(Y=Y.to(DEV), c=c.to(DEV), logits=logits.to(DEV), alpha=alpha)) == float(loss)   # alpha= overrides


def test_nll_surv_loss_as_the_criterion_of_a_survival_step():
    """One step of the reference's surv_train loop (engines/base_engine.py:395-430): forward_func with label = [Y, c], the criterion on
    the logits, backward."""
    from mhim_mil_amd.engine import CommonMIL
    from mhim_mil_amd.mhim import MHIM
    from mhim_mil_amd.survival import NLLSurvLoss
    K = 4
    st = synth.mhim_state(11, input_dim=256, n_classes=K, merge_enable=False)
    m = MHIM(baseline="attn", n_classes=K, input_dim=256, act="gelu", da_act="relu", merge_enable=False, dropout=0.0)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()}, strict=True)
    m = m.to(DEV).train()
    args = types.SimpleNamespace(model="mhim_pure", baseline="attn", aux_alpha=0.0)
    bag = torch.from_numpy(synth.bag(12, 97, 256)).to(DEV).unsqueeze(0)
    label = [torch.tensor([2], device=DEV), torch.tensor([0.0], device=DEV)]
    out = CommonMIL(args).forward_func(args, m, None, bag, label, NLLSurvLoss(alpha=0.0), 1, 0, 0, 0, None)
    logits, labels_surv = out[0], out[1]
    assert labels_surv is label and logits.shape == (1, K)
    loss = NLLSurvLoss(alpha=0.0)(logits=logits, Y=labels_surv[0], c=labels_surv[1])
    loss.backward()
    _, ref = SO.nll_surv(logits.detach().double().cpu(), torch.tensor([2]), torch.tensor([0.0]))
    assert abs(float(loss) - float(ref)) < 1e-5
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name


# ------------------------------------------------------------------------------------------------ 4. surv_validate
N_BAGS, BINS = 24, 4


@functools.lru_cache(maxsize=None)
def surv_set():
    rng = np.random.default_rng(5)
    batches = []
    for b in range(N_BAGS):
        x = synth.bag(300 + b, int(rng.integers(40, 201)), 256)
        batches.append({"input": torch.from_numpy(x).unsqueeze(0), "target": torch.tensor([int(rng.integers(0, BINS))]),
                        "censorship": torch.tensor([float(rng.integers(0, 2))]), "event": torch.tensor([int(rng.integers(1, 13))])})
    cens = np.array([float(b["censorship"]) for b in batches])
    cens[:2] = (0.0, 1.0)
    batches[0]["censorship"], batches[1]["censorship"] = torch.tensor([0.0]), torch.tensor([1.0])
    return batches, cens, np.array([float(b["event"]) for b in batches])


def _model(baseline):
    from mhim_mil_amd.mhim import MHIM
    if baseline == "attn":
        st = synth.mhim_state(3, input_dim=256, n_classes=BINS, merge_k=5)
        m = MHIM(baseline="attn", n_classes=BINS, input_dim=256, act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5,
                 attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999, merge_ratio=0.9, temp_t=0.1, dropout=0.0)
        st["merge.global_q"] = st["merge.global_q_mm"]
    else:
        st = synth.mhim_state(4, input_dim=256, n_classes=BINS, baseline="dsmil", merge_enable=False)
        m = MHIM(baseline="dsmil", n_classes=BINS, input_dim=256, act="gelu", dropout=0.0, merge_enable=False)
    st["feature.0.bias"] = (0.05 * synth.normal(903, (512,))).astype(np.float32)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()}, strict=True)
    return m.to(DEV).eval()


def _args(baseline, **kw):
    return types.SimpleNamespace(**dict(dict(model="mhim", baseline=baseline, n_classes=BINS, bootstrap_mode=(), best_metric_index=0), **kw))


class _Spy:
    """ops.surv_nll with its inputs and outputs kept: the device's own logits, risk and losses of a pass."""

    def __init__(self, monkeypatch):
        self.calls, self.real = [], _ops().surv_nll
        monkeypatch.setattr(_ops(), "surv_nll", self)

    def __call__(self, logits, Y, c, **kw):
        out = self.real(logits, Y, c, **kw)
        self.calls.append((logits.clone(), out[0].clone(), out[1].clone(), kw))
        return out

    def take(self):
        calls, self.calls = self.calls, []
        return [torch.cat([k[j] for k in calls]) for j in range(3)] + [len(calls)]


class _Stop:
    early_stop = False

    def __call__(self, args, epoch, score, model):
        self.score = score


def _run(baseline, chunk, monkeypatch, status="val", **kw):
    from mhim_mil_amd import validate as V
    from mhim_mil_amd.engine import CommonMIL
    from mhim_mil_amd.survival import NLLSurvLoss
    args, spy, stop = _args(baseline, **kw), _Spy(monkeypatch), _Stop()
    out = V.surv_validate(CommonMIL(args), args, _model(baseline), surv_set()[0], criterion=NLLSurvLoss(alpha=0.0), early_stopping=stop,
                          epoch=3, status=status, chunk=chunk)
    return out, spy.take(), stop


@pytest.mark.parametrize("baseline,chunk", [("attn", 0), ("attn", 5), ("dsmil", 5)])
def test_surv_validate_metric_and_loss_come_from_the_devices_own_risk(baseline, chunk, monkeypatch):
    _, cens, times = surv_set()
    out, (logits, risk, losses, calls), stop = _run(baseline, chunk, monkeypatch)
    assert calls == (5 if chunk else 1) and logits.shape == (N_BAGS, BINS)
    ref = SO.cindex_pairs(1 - cens, times, risk.cpu().numpy())
    assert not np.isnan(ref["cindex"])
    assert len(out) == 5 and out[0] == [ref["cindex"], ref["cindex"]] and out[1] is False and out[3] is None
    assert out[2] == float(losses.mean()) and list(out[4].keys()) == ["cindex", "loss"]
    assert out[4]["cindex"] == ref["cindex"] and out[4]["loss"] == out[2]
    assert stop.score == -ref["cindex"]                                   # early stopping runs on -cindex
    # the head is the restatement's on these logits, and the pass agrees with the bag-after-bag forward
    r64, l64 = SO.nll_surv(logits.double().cpu(), torch.cat([b["target"] for b in surv_set()[0]]), torch.from_numpy(cens))
    np.testing.assert_allclose(risk.cpu().numpy(), r64.numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(losses.cpu().numpy(), l64.numpy(), atol=1e-5, rtol=0)
    if chunk:
        _, (logits0, _, _, _), _ = _run(baseline, 0, monkeypatch)
        np.testing.assert_allclose(logits.cpu().numpy(), logits0.cpu().numpy(), atol=LOGIT_TOL, rtol=0)


def test_surv_validate_test_status_and_bootstrap(monkeypatch):
    _, cens, times = surv_set()
    out, (_, risk, losses, _), _ = _run("attn", 5, monkeypatch, status="test")
    ref = SO.cindex_pairs(1 - cens, times, risk.cpu().numpy())["cindex"]
    assert len(out) == 3 and out[0] == [ref, 0] and out[1] == float(losses.mean())
    assert list(out[2].items()) == [("cindex", ref), ("cindex_std", 0), ("loss", out[1])]
    B, fold = 25, 2
    out, (_, risk, losses, _), _ = _run("attn", 5, monkeypatch, status="test", bootstrap_mode=("test",), num_bootstrap=B, fold_curr=fold)
    rk = risk.cpu().numpy()
    per = np.array([SO.cindex_pairs((1 - cens)[i], times[i], rk[i])["cindex"] for i in boot_idx(N_BAGS, B, fold).numpy()])
    assert not np.isnan(per).any()
    np.testing.assert_allclose(out[0], [per.mean(), per.std(ddof=1)], rtol=1e-12)
    assert list(out[2].keys()) == ["cindex", "cindex_std", "loss"] and [out[2]["cindex"], out[2]["cindex_std"]] == out[0]
    # status 'val' inside bootstrap_mode: the mean alone, in the validation tuple
    out, _, stop = _run("attn", 5, monkeypatch, status="val", bootstrap_mode=("val", "test"), num_bootstrap=B, fold_curr=fold)
    assert len(out) == 5 and out[0][0] == out[0][1] == out[4]["cindex"] == -stop.score
    np.testing.assert_allclose(out[0][0], per.mean(), rtol=1e-12)


def test_get_surv_metrics_raises_without_a_comparable_pair():
    from mhim_mil_amd import validate as V
    from mhim_mil_amd._lib import MhimxError
    args = types.SimpleNamespace(num_bootstrap=5, fold_curr=0)
    ev, tm, rk = torch.zeros(40, device=DEV), torch.arange(40.0, device=DEV), torch.rand(40, device=DEV)
    for boot in (False, True):
        with pytest.raises(MhimxError, match="comparable"):
            V.get_surv_metrics(args, ev, tm, rk, bootstrap=boot)
    ev[0] = 1
    assert V.get_surv_metrics(args, ev, tm, rk) == SO.cindex_pairs(ev.cpu().numpy(), tm.cpu().numpy(), rk.cpu().numpy())["cindex"]
