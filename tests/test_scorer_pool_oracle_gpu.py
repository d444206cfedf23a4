"""The one-pass ABMIL scorer + softmax pool (scorer_fused_kernel, scorer_fused_bwd_kernel, pool_finalize_kernel,
pool_finalize_tok_kernel) against the fp64 oracle under autograd on the CPU - not against another form of itself.

Fixed everywhere: E = 512, A = 128, the plain (ungated) scorer, prec = "bf16x3"; T = |N(0,1)|, wa std 0.06, ba std 0.1, wc std 0.3 (1.0 in the
peaked regime), g_z std 0.01.  The weights depend on (bias, wc std) only, never on the row count, so that the M = 1 cases can be held
against the M = 33 gradients of the same weights.

Row counts: 1 (attn = 1) | 31 / 32 / 33 (around one 32-row tile) | 95 (three tiles, the last short by one row) | 16417 = 512 * 32 + 33 (514
tiles over MAX_PART = 512 workgroups: workgroups 0 and 1 walk two tiles each - the running max / sum / pooled row are rescaled, dwc_run /
dbc_run accumulate across tiles, ridx / Ds / an_s are rewritten - and the last tile holds one row).

  A  the one-call forward: with / without the kind-4 fragment image (bit-equal), gathered out of a NaN-poisoned bag, with excluded rows,
     with the scores shifted by +-100, with a peaked softmax, with no_backward;
  B  the two-call forward (abmil_pool_fwd_split / abmil_pool_fwd_finish, mhimx_pool_io.phase 1 / 2: the finalize launch scores the K <= 6
     tail tokens itself in fp32 FMAs, with and without the transposed weight, finding the rows by tail_row0 or at the end of rows1) and the
     backward that follows it.  The riding Merge rows pass (ride_merge) is OUT OF SCOPE here: only whole-step comparisons reach it;
  C  the backward: with / without the kind-5 image (bit-equal), gathered into a sentinel-filled buffer, with excluded rows, accumulating,
     with a peaked softmax, at one row, and its dPRE image where a workgroup walks more than one tile.

Bounds (d = device - fp64 reference):
  s          |d| <= 2e-5 max|s_ref|          (TOL["bf16x3"] of tests/test_ops_gpu.py, relative to scale); called `delta` below
  stats[0]   the same (it is one of the scores)
  stats[1]   rtol 2 delta + 1e-6: every term e^{s_n - max} moves by at most e^{2 delta}; 1e-6: fp32 rounding of the sum itself
  z          atol 1.2e-5, rtol 4e-5          (test_fused_scorer_fragment_image)
  attention  atol 1e-7, rtol 2 delta; in the peaked regime |log a - log a_ref| <= 2 delta on rows with a_ref > 1e-30
  cproj      atol 2e-5, rtol 1e-5
  pscore     2e-6 + 0.5 max_c |d x_c|, x_c = a_n cproj[n, c]: the class softmax moves by at most half the largest change of its inputs
             (sum_c |d p_i / d x_c| = 2 p_i (1 - p_i) <= 1/2), |d x_c| <= a_n |d cproj| + |cproj| |d a_n| from the two bounds above; 2e-6 is
             test_pseudo_score_matches_oracle's bound on the kernel's own arithmetic
  gradients  allclose(atol = 3e-5 max|ref|, rtol = 2e-4)   (test_pool_fwd_bwd at f = 1); peaked regime: atol from a CPU model, see
             test_backward_peaked_softmax; relu: the same bound, against the reference with the kernel's side of the pre-activations
             that sit on the kink, see _relu_kinks_settled; d_bc is identically 0: absolute 1e-6

Every comparison notes its largest error over its bound in RATIOS before it asserts."""
import functools

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, A = 512, 128
ACT = {"relu": 1, "gelu": 2, "tanh": 3}
S_REL = 2e-5
Z_TOL = dict(atol=1.2e-5, rtol=4e-5)
G_ATOL, G_RTOL = 3e-5, 2e-4
SENTINEL = 7.25
# (M, activation, bias): all three activations at 33 and 16417, one elsewhere; bias on and off at every row count
CASES = [(1, "tanh", True), (1, "relu", False), (31, "gelu", True), (31, "tanh", False), (32, "relu", True), (32, "gelu", False),
         (33, "relu", True), (33, "gelu", True), (33, "tanh", True), (33, "relu", False), (33, "gelu", False), (33, "tanh", False),
         (95, "tanh", True), (95, "relu", False),
         (16417, "relu", True), (16417, "gelu", True), (16417, "tanh", True), (16417, "relu", False), (16417, "gelu", False),
         (16417, "tanh", False)]
BWD_CASES = [c for c in CASES if c[0] in (1, 33, 95, 16417)]
_id = lambda c: "%d-%s-%s" % (c[0], c[1], "bias" if c[2] else "nobias")


def _ops():
    from mhim_mil_amd import ops
    return ops


def rnd(seed, shape, std=1.0):
    return torch.from_numpy(synth.normal(seed, shape, std=std).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- inputs
def _bag_rows(M):
    return 16500 if M > 1500 else 1500


@functools.lru_cache(maxsize=None)
def _bag(R):
    """The bag the token lists are drawn from: R rows of |N(0,1)|."""
    return rnd(11, (R, E)).abs()


@functools.lru_cache(maxsize=None)
def _rows(M):
    """M distinct rows of the bag in random order; the token list of every (M, ...) case is _bag(R)[_rows(M)]."""
    return torch.from_numpy(synth.permutation(12, _bag_rows(M))[:M].copy())


@functools.lru_cache(maxsize=None)
def _tokens(M):
    return _bag(_bag_rows(M))[_rows(M)].contiguous()


@functools.lru_cache(maxsize=None)
def _weights(bias, wc_std=0.3):
    w = dict(wa=rnd(30, (A, E), std=0.06), wc=rnd(31, (1, A), std=wc_std), ba=None, bc=None)
    if bias:
        w["ba"], w["bc"] = rnd(33, (A,), std=0.1), rnd(35, (1,), std=0.1)
    return w


@functools.lru_cache(maxsize=None)
def _gz():
    return rnd(41, (E,), std=0.01)


@functools.lru_cache(maxsize=None)
def _excl_mask(M):
    """~30 % of the rows, one whole 32-row tile (tile 1: at M = 16417 both tiles of workgroup 1 are then dead and its partial is (-inf, 0))
    and the whole short last tile; by list position."""
    m = torch.from_numpy(synth.uniform(13, (M,)) < 0.3)
    m[32:64] = True
    m[(M - 1) // 32 * 32:] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- fp64 oracle
def _oracle(X, w, act, gz=None, live=None, u_err=None):
    """The pool over the tokens X[live] in fp64 (oracle.mhim_oracle), with gz under autograd.  A scorer without biases gets zero ones: the
    gradients with respect to them are what the kernel's d_ba / d_bc hold.  u_err [M, A]: added to the pre-activations (it rides in on the
    bias, which broadcasts) - the CPU model of the peaked regime's bound."""
    grad = gz is not None
    M = X.shape[0]
    leaf = lambda t: t.double().clone().requires_grad_(grad)
    X64, wa, wc = leaf(X), leaf(w["wa"]), leaf(w["wc"])
    ba = leaf(w["ba"] if w["ba"] is not None else torch.zeros(A))
    bc = leaf(w["bc"] if w["bc"] is not None else torch.zeros(1))
    s = O.scorer_logits(X64, wa, wc, act, ba=ba if u_err is None else ba[None, :] + u_err.double(), b2=bc)
    idx = torch.arange(M) if live is None else torch.nonzero(live).ravel()
    z, a_l = O.softmax_pool(X64[idx], s[idx])
    out = dict(s=s.detach(), z=z.detach(), attn=torch.zeros(M, dtype=torch.float64))
    out["attn"][idx] = a_l.detach()
    mx = s.detach()[idx].max()
    out["stats"] = torch.stack([mx, torch.exp(s.detach()[idx] - mx).sum()])
    out["delta"] = S_REL * float(s.detach()[idx].abs().max())
    if grad:
        (z * gz.double()).sum().backward()
        out.update(dT=X64.grad, d_wa=wa.grad, d_wc=wc.grad, d_ba=ba.grad, d_bc=bc.grad)
        if act == "relu":
            u = (X64 @ wa.t() + ba).detach()
            ds = out["attn"] * (X64.detach() @ gz.double() - out["z"] @ gz.double())
            out["kinks"] = [(int(n), int(a), float(ds[n] * wc.detach()[0, a]) * (-1.0 if u[n, a] > 0 else 1.0))
                            for n, a in torch.nonzero(u.abs() < S_REL * u.abs().max()).tolist()]
    return out


def _relu_kinks_settled(ref, X, wa, dT):
    """relu'(0) is a convention, and the fp64 derivative at a pre-activation that lies within the three-term product's error of 0 (|u| <
    2e-5 max|u|, TOL["bf16x3"]; ref["kinks"], ~1e-4 of the entries) is decided by rounding: there the kernel may rightly stand on the
    other side.  No bound is widened for that.  Each listed entry (n, a) either stands as in fp64 or is flipped, and a flip moves
    du[n, a] by exactly ddu = -+ ds_n wc[a], hence dT[n, :] by ddu Wa[a, :], d_wa[a, :] by ddu T[n, :] and d_ba[a] by ddu (d_wc holds
    relu(u), which is continuous).  Which entries the kernel flipped is read off its dT row (the projection of the row's residual on
    Wa[a, :] is nearer to ddu than to 0); the reference with exactly those flips applied must then meet the fixed bound in dT, d_wa and
    d_ba alike.  Returns (that reference, the number of flips)."""
    out = dict(ref, dT=ref["dT"].clone(), d_wa=ref["d_wa"].clone(), d_ba=ref["d_ba"].clone())
    X, wa, res, flips = X.double(), wa.double(), dT.double() - ref["dT"], 0
    for n, a, ddu in ref.get("kinks", ()):
        v = ddu * wa[a]
        if float(res[n] @ v) > 0.5 * float(v @ v):
            res[n] -= v
            out["dT"][n] += v
            out["d_wa"][a] += ddu * X[n]
            out["d_ba"][a] += ddu
            flips += 1
    return out, flips


@functools.lru_cache(maxsize=None)
def _ref(M, act, bias, excl=False):
    """The forward's reference (a few vectors): computed once per case, shared by the tests that use it, never modified."""
    return _oracle(_tokens(M), _weights(bias), act, live=~_excl_mask(M) if excl else None)


@functools.lru_cache(maxsize=2)
def _ref_grad(M, act, bias, excl=False):
    """The same with the fp64 gradients.  (dT is 67 MB at M = 16417: only the case at hand and its neighbour stay resident.)"""
    return _oracle(_tokens(M), _weights(bias), act, gz=_gz(), live=~_excl_mask(M) if excl else None)


RATIOS = []          # (label, largest error / bound) of every comparison of the session, in order: what a description's table is filled from


# ---------------------------------------------------------------------------------------------------------------- comparisons
def _check(label, got, ref, atol, rtol=0.0, check=True):
    """max |got - ref| / (atol + rtol |ref|) <= 1, noted in RATIOS first (check=False: noted only)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref = ref.double()
    assert torch.isfinite(got).all(), label + ": not finite"
    err, den = (got - ref).abs(), atol + rtol * ref.abs()
    ratio = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = float(ratio.max())
    RATIOS.append((label, r))
    assert r <= 1.0 or not check, "%s: max error is %.3f of its bound (first at flat index %d: got %r, ref %r)" % (
        label, r, int(ratio.argmax()), float(got.ravel()[ratio.argmax()]), float(ref.ravel()[ratio.argmax()]))


def _check_grad(label, got, ref, atol_rel=G_ATOL, check=True):
    _check(label, got, ref, atol=atol_rel * float(ref.abs().max()), rtol=G_RTOL, check=check)


def _check_pool(label, ops, st, ref, live=None, delta=None, attn_delta=None):
    """s, stats, z and the attention of one forward against the oracle's (see the module docstring for the bounds)."""
    delta = ref["delta"] if delta is None else delta
    attn_delta = delta if attn_delta is None else attn_delta
    s = st.s.cpu()
    if live is None:
        live = torch.ones(s.numel(), dtype=torch.bool)
    assert (s[~live] == float("-inf")).all(), label + ": an excluded row's score is not -inf"
    _check(label + " s", s[live], ref["s"][live], atol=delta)
    _check(label + " stats[0]", st.stats[0], ref["stats"][0], atol=delta)
    _check(label + " stats[1]", st.stats[1], ref["stats"][1], atol=0.0, rtol=2 * delta + 1e-6)
    _check(label + " z", st.z, ref["z"], **Z_TOL)
    _check(label + " attn", ops.softmax_from_stats(st.s, st.stats), ref["attn"], atol=1e-7, rtol=2 * attn_delta)


def _check_classes(label, st, ref, X, wp, bp):
    """cproj and the pseudo score against fp64 (O.pseudo_score)."""
    cp_ref = X.double() @ wp.double().t()
    _check(label + " cproj", st.cproj, cp_ref, atol=2e-5, rtol=1e-5)
    ps_ref = O.pseudo_score(X.double(), ref["attn"], wp.double(), bp.double())
    a = ref["attn"][:, None]
    dx = a * (2e-5 + 1e-5 * cp_ref.abs()) + cp_ref.abs() * (1e-7 + 2 * ref["delta"] * a)
    _check(label + " pscore", st.pscore, ps_ref, atol=2e-6 + 0.5 * dx.max(1).values)


def _scorer(ops, w, act, wa_frag=None, bc=None):
    d = lambda t: None if t is None else t.to(DEV)
    return ops.ScorerW(d(w["wa"]), d(w["wc"]), ACT[act], ba=d(w["ba"]), bc=d(w["bc"] if bc is None else bc), prec="bf16x3", wa_frag=wa_frag)


def _frag(ops, w):
    """prep kind 4: the fragment image of Wa for the forward."""
    img = torch.empty(A, E, device=DEV)
    ops.prep_batch([(ops.PREP_FRAG, w["wa"].to(DEV), img)])
    return img


def _frag_t(ops, w):
    """prep kind 5: the fragment image of Wa^T (made from the untransposed weight) for the backward."""
    img = torch.empty(E, A, device=DEV)
    ops.prep_batch([(ops.PREP_FRAG_T, w["wa"].to(DEV), img)])
    return img


def _outputs(st):
    return [t.clone() for t in (st.s, st.stats, st.z, st.cproj, st.pscore) if t is not None]


def _poisoned_bag(M):
    """The bag with every row that is not in the list filled with NaN: the kernels clamp their reads to the list's last entry, so they may
    never touch such a row."""
    T = torch.full((_bag_rows(M), E), float("nan"))
    T[_rows(M)] = _tokens(M)
    return T


# ================================================================================================================ A. one-call forward
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_vs_fp64(case):
    """Contiguous rows, class projections for C = 1 and 4 with the pseudo score; the kind-4 image run equals the on-the-fly split bit for
    bit and is then held against fp64."""
    ops = _ops()
    M, act, bias = case
    w, X, ref = _weights(bias), _tokens(M), _ref(M, act, bias)
    frag = _frag(ops, w)
    for Cc in (1, 4):
        wp, bp = rnd(53, (Cc, E), std=0.05), rnd(54, (Cc,), std=0.1)
        res = []
        for wf in (None, frag):
            st = ops.abmil_pool_fwd(_scorer(ops, w, act, wf), X.to(DEV), wp=wp.to(DEV), bp=bp.to(DEV))
            res.append(_outputs(st))
        assert len(res[0]) == 5
        for a, b in zip(*res):
            assert torch.equal(a, b), "the fragment image changes the result"
        label = "A %s C=%d" % (_id(case), Cc)
        _check_pool(label, ops, st, ref)
        _check_classes(label, st, ref, X, wp, bp)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 95], ids=_id)
def test_forward_five_classes_row_pass_form(case):
    """C = 5 > SF_MAXC = 4: the call takes the row-pass form (three-term GEMM, then score_rows_fwd_kernel); the same bounds."""
    ops = _ops()
    M, act, bias = case
    w, X, ref = _weights(bias), _tokens(M), _ref(M, act, bias)
    wp, bp = rnd(53, (5, E), std=0.05), rnd(54, (5,), std=0.1)
    st = ops.abmil_pool_fwd(_scorer(ops, w, act), X.to(DEV), wp=wp.to(DEV), bp=bp.to(DEV))
    label = "A %s C=5" % _id(case)
    _check_pool(label, ops, st, ref)
    _check_classes(label, st, ref, X, wp, bp)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_gathered_from_poisoned_bag(case):
    """rows1 = a random subset in random order of a larger bag whose other rows hold NaN: finite, and the fp64 pool of T[rows1]."""
    ops = _ops()
    M, act, bias = case
    w, ref = _weights(bias), _ref(M, act, bias)
    T, rows1 = _poisoned_bag(M).to(DEV), _rows(M).to(DEV)
    wp, bp = rnd(53, (4, E), std=0.05), rnd(54, (4,), std=0.1)
    res = []
    for wf in (None, _frag(ops, w)):
        st = ops.abmil_pool_fwd(_scorer(ops, w, act, wf), T, wp=wp.to(DEV), bp=bp.to(DEV), rows1=rows1)
        res.append(_outputs(st))
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    label = "A gather %s" % _id(case)
    _check_pool(label, ops, st, ref)
    _check_classes(label, st, ref, _tokens(M), wp, bp)


@pytest.mark.parametrize("gather", [False, True], ids=["contiguous", "gathered"])
@pytest.mark.parametrize("case", [(95, "tanh", True), (16417, "gelu", False)], ids=_id)
def test_forward_excluded_rows(case, gather):
    """excl (by SOURCE row): ~30 % of the rows, a whole tile and the whole short last tile.  The excluded rows hold ordinary values (the
    contract multiplies them by 0).  Their score is -inf exactly; the live rows and z are the fp64 pool over the live rows."""
    ops = _ops()
    M, act, bias = case
    w, ref, dead = _weights(bias), _ref(M, act, bias, excl=True), _excl_mask(M)
    if gather:
        T, rows1 = _bag(_bag_rows(M)), _rows(M)
        excl = torch.zeros(T.shape[0], dtype=torch.uint8)
        excl[rows1[dead]] = 1
        rows1 = rows1.to(DEV)
    else:
        T, rows1, excl = _tokens(M), None, dead.to(torch.uint8)
    res = []
    for wf in (None, _frag(ops, w)):
        st = ops.abmil_pool_fwd(_scorer(ops, w, act, wf), T.to(DEV), rows1=rows1, excl=excl.to(DEV))
        res.append(_outputs(st))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert torch.isfinite(st.stats).all()
    _check_pool("A excl %s %s" % (_id(case), "gathered" if gather else "contiguous"), ops, st, ref, live=~dead)


def test_forward_one_live_row():
    """M = 16417 with exactly one live row, in the SECOND of the two tiles workgroup 0 walks (tile 512): every other partial is (-inf, 0),
    and inside workgroup 0 the running state is rescaled from -inf."""
    ops = _ops()
    M, act, bias, row = 16417, "tanh", True, 512 * 32 + 7
    w, X = _weights(bias), _tokens(M)
    excl = torch.ones(M, dtype=torch.uint8)
    excl[row] = 0
    st = ops.abmil_pool_fwd(_scorer(ops, w, act, _frag(ops, w)), X.to(DEV), excl=excl.to(DEV))
    s = st.s.cpu()
    assert torch.isfinite(s[row]) and (s[excl.bool()] == float("-inf")).all()
    assert torch.isfinite(st.stats).all() and torch.isfinite(st.z).all()
    assert float(st.stats[0]) == float(s[row])
    _check("A one live row stats[1]", st.stats[1], torch.tensor(1.0, dtype=torch.float64), atol=1e-6)
    _check("A one live row z", st.z, X[row].double(), atol=1e-6 * float(X[row].max()))
    _check("A one live row s", s[row], _ref(M, act, bias)["s"][row], atol=_ref(M, act, bias)["delta"])


@pytest.mark.parametrize("shift", [100.0, -100.0], ids=["plus100", "minus100"])
@pytest.mark.parametrize("M", [33, 16417])
def test_forward_shifted_scores(M, shift):
    """bc = +-100 (e^100 overflows fp32: only a correct max subtraction survives).  The scores and stats[0] move by the shift; the
    attention, stats[1] and z stay within their bounds of the UNSHIFTED fp64 values."""
    ops = _ops()
    act = "tanh"
    w, X, ref0 = _weights(True), _tokens(M), _ref(M, "tanh", True)
    move = shift - float(w["bc"].double())
    ref = dict(ref0, s=ref0["s"] + move, stats=torch.stack([ref0["stats"][0] + move, ref0["stats"][1]]))
    res = []
    for wf in (None, _frag(ops, w)):
        st = ops.abmil_pool_fwd(_scorer(ops, w, act, wf, bc=torch.tensor([shift])), X.to(DEV))
        res.append(_outputs(st))
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # (the scores themselves: the unshifted bound and one fp32 ulp at 100 - adding bc rounds the sum there)
    _check_pool("A shift %+d M=%d" % (shift, M), ops, st, ref, delta=ref0["delta"] + 2.0 ** -17, attn_delta=ref0["delta"])


PEAK_M = 2000


@functools.lru_cache(maxsize=None)
def _peaked():
    """wc std 1.0 instead of 0.3 at M = 2000 (tanh, with biases): a score span > 30 and most of the weight on one row."""
    w, X = _weights(True, 1.0), rnd(11, (PEAK_M, E)).abs()
    ref = _oracle(X, w, "tanh", gz=_gz())
    span, top = float(ref["s"].max() - ref["s"].min()), float(ref["attn"].max())
    assert span > 30 and 0.5 < top < 0.99, "the inputs are not in the peaked regime: span %.1f, top attention %.3f" % (span, top)
    return w, X, ref


def test_forward_peaked_softmax():
    ops = _ops()
    w, X, ref = _peaked()
    res = []
    for wf in (None, _frag(ops, w)):
        st = ops.abmil_pool_fwd(_scorer(ops, w, "tanh", wf), X.to(DEV))
        res.append(_outputs(st))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    _check_pool("A peaked", ops, st, ref)
    attn = ops.softmax_from_stats(st.s, st.stats).cpu().double()
    seen = ref["attn"] > 1e-30
    assert seen.sum() > PEAK_M // 2 and (attn[seen] > 0).all()
    _check("A peaked log attn", torch.log(attn[seen]), torch.log(ref["attn"][seen]), atol=2 * ref["delta"])


@pytest.mark.parametrize("case", [(33, "gelu", True), (16417, "relu", False)], ids=_id)
def test_forward_no_backward_same_outputs(case):
    """no_backward = 1 (the scorer stores no pre-activations) changes none of s, stats, z, cproj, pscore."""
    ops = _ops()
    M, act, bias = case
    w, X = _weights(bias), _tokens(M).to(DEV)
    wp, bp = rnd(53, (4, E), std=0.05).to(DEV), rnd(54, (4,), std=0.1).to(DEV)
    sc = _scorer(ops, w, act, _frag(ops, w))
    a = _outputs(ops.abmil_pool_fwd(sc, X, wp=wp, bp=bp))
    b = _outputs(ops.abmil_pool_fwd(sc, X, wp=wp, bp=bp, no_backward=True))
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ================================================================================================================ B. two-call forward
SPLIT_K, SPLIT_LK = (1, 3, 6), (1, 33, 1000, 16417)
# (tail_row0 given, wa_t given): all four with every K, both values of each with every Lk
_SPLIT_FORMS = [(True, True), (False, False), (True, False), (False, True)]
SPLIT_CASES = [(K, Lk) + _SPLIT_FORMS[(i + j) % 4] for i, K in enumerate(SPLIT_K) for j, Lk in enumerate(SPLIT_LK)]
_sid = lambda c: "K%d-Lk%d-%s-%s" % (c[0], c[1], "row0" if c[2] else "rows1end", "wat" if c[3] else "nowat")


@functools.lru_cache(maxsize=None)
def _tail(K):
    """The K tokens behind the bag (a Merge's outputs: signed, std 0.5)."""
    return rnd(22, (K, E), std=0.5)


def _split_layout(Lk, K, tail=None):
    """As mhim.py's _bag_forward_nat builds it: T = [N + K, E], rows1 = [Lk distinct rows of 0 .. N-1 in random order | N .. N+K-1].
    Returns (T with the tail in place, rows1, N)."""
    N = _bag_rows(Lk)
    T = torch.cat([_bag(N), _tail(K) if tail is None else tail], 0)
    rows1 = torch.cat([_rows(Lk), N + torch.arange(K)])
    return T, rows1, N


def _split_forward(ops, sc, T, rows1, N, K, row0, wat):
    """Phase 1 while the tail rows hold NaN (it must not read them), the tokens written, phase 2."""
    Td = T.to(DEV)
    tail = Td[N:].clone()
    Td[N:] = float("nan")
    st, rode = ops.abmil_pool_fwd_split(sc, Td, rows1.to(DEV), K)
    assert not rode
    Td[N:] = tail
    ops.abmil_pool_fwd_finish(sc, st, wa_t=ops.transpose(sc.t[0]) if wat else None, tail_row0=N if row0 else -1)
    for t in (st.s, st.stats, st.z):
        assert torch.isfinite(t).all()
    return st, Td


def _check_split_vs_one_call(label, ops, st, one, ref):
    """Within the same bounds, not bit for bit: the tail is scored in fp32 FMAs, not as the three-term product."""
    d = ref["delta"]
    _check(label + " s vs one-call", st.s, one.s.cpu().double(), atol=d)
    _check(label + " stats[0] vs one-call", st.stats[0], one.stats[0].cpu().double(), atol=d)
    _check(label + " stats[1] vs one-call", st.stats[1], one.stats[1].cpu().double(), atol=0.0, rtol=2 * d + 1e-6)
    _check(label + " z vs one-call", st.z, one.z.cpu().double(), **Z_TOL)


@pytest.mark.parametrize("case", SPLIT_CASES, ids=_sid)
def test_split_forward_vs_fp64_and_one_call(case):
    ops = _ops()
    K, Lk, row0, wat = case
    act, bias = ("tanh", "relu", "gelu")[SPLIT_K.index(K)], SPLIT_LK.index(Lk) % 2 == 0
    w = _weights(bias)
    T, rows1, N = _split_layout(Lk, K)
    ref = _oracle(T[rows1], w, act)
    sc = _scorer(ops, w, act, _frag(ops, w))
    st, Td = _split_forward(ops, sc, T, rows1, N, K, row0, wat)
    assert st.s.numel() == Lk + K
    label = "B %s" % _sid(case)
    _check_pool(label, ops, st, ref)
    _check_split_vs_one_call(label, ops, st, ops.abmil_pool_fwd(sc, Td, None, rows1=rows1.to(DEV)), ref)


@pytest.mark.parametrize("regime", ["tail_is_max", "tail_is_nothing"])
def test_split_forward_tail_regimes(regime):
    """Lk = 1000, K = 3, relu without biases (the score is then homogeneous in the token: s(c t) = c s(t) for c > 0), one tail token scaled so
    that in fp64 it (a) tops the list's maximum by more than 5 - stats[0] comes from the tail - or (b) lies more than 30 under the list's
    minimum - it contributes nothing."""
    ops = _ops()
    K, Lk, act = 3, 1000, "relu"
    w = _weights(False)
    T, rows1, N = _split_layout(Lk, K)
    s0 = _oracle(T[rows1], w, act)["s"]
    body, ts = s0[:Lk], s0[Lk:]
    tail = _tail(K).clone()
    if regime == "tail_is_max":
        i = int(ts.argmax())
        assert ts[i] > 0
        tail[i] *= float((body.max() + 6.0) / ts[i])
    else:
        i = int(ts.argmin())
        assert ts[i] < 0
        tail[i] *= float((body.min() - 31.0) / ts[i])
    T, rows1, N = _split_layout(Lk, K, tail)
    ref = _oracle(T[rows1], w, act)
    others = torch.cat([ref["s"][:Lk + i], ref["s"][Lk + i + 1:]])
    if regime == "tail_is_max":
        assert ref["s"][Lk + i] > others.max() + 5 and ref["stats"][0] == ref["s"][Lk + i]
    else:
        assert ref["s"][Lk + i] < others.min() - 30
    sc = _scorer(ops, w, act, _frag(ops, w))
    row0, wat = (True, True) if regime == "tail_is_max" else (False, False)
    st, Td = _split_forward(ops, sc, T, rows1, N, K, row0, wat)
    label = "B %s" % regime
    _check_pool(label, ops, st, ref)
    _check_split_vs_one_call(label, ops, st, ops.abmil_pool_fwd(sc, Td, None, rows1=rows1.to(DEV)), ref)


@pytest.mark.parametrize("Lk,act,row0,wat", [(33, "tanh", True, True), (16417, "gelu", False, False)])
def test_backward_after_split_forward(Lk, act, row0, wat):
    """abmil_pool_bwd on the split forward's state against fp64 autograd: dT at the stay rows and at the K = 6 tail rows, d_wa, d_wc, d_ba.
    The only check that the finalize launch wrote the tail's pre-activations and scores where the backward reads them."""
    ops = _ops()
    K, w = 6, _weights(True)
    T, rows1, N = _split_layout(Lk, K)
    ref = _oracle(T[rows1], w, act, gz=_gz())
    sc = _scorer(ops, w, act, _frag(ops, w))
    st, Td = _split_forward(ops, sc, T, rows1, N, K, row0, wat)
    dT = torch.full((N + K, E), SENTINEL, device=DEV)
    g = ops.abmil_pool_bwd(sc, st, _gz().to(DEV), ops.transpose(sc.t[0]), need_bias=True, grads={"dT1": dT}, wa_t_frag=_frag_t(ops, w))
    label = "B bwd Lk=%d" % Lk
    dT = dT.cpu()
    scale = G_ATOL * float(ref["dT"].abs().max())
    _check(label + " dT stay rows", dT[rows1[:Lk]], ref["dT"][:Lk], atol=scale, rtol=G_RTOL)
    _check(label + " dT tail rows", dT[N:], ref["dT"][Lk:], atol=scale, rtol=G_RTOL)
    other = torch.ones(N + K, dtype=torch.bool)
    other[rows1] = False
    assert (dT[other] == SENTINEL).all()
    for k in ("d_wa", "d_wc", "d_ba"):
        _check_grad(label + " " + k, g[k], ref[k])
    assert abs(float(g["d_bc"])) < 1e-6


@pytest.mark.parametrize("K,Lk", [(0, 33), (7, 33), (3, 0)], ids=["K0", "K7", "Lk0"])
def test_split_forward_refusals(K, Lk):
    ops = _ops()
    from mhim_mil_amd import _lib as L
    N = 1500
    T = torch.zeros(N + max(K, 1), E, device=DEV)
    rows1 = torch.cat([_rows(33)[:Lk], N + torch.arange(K)]).to(DEV)
    with pytest.raises(L.MhimxError):
        ops.abmil_pool_fwd_split(_scorer(ops, _weights(False), "relu"), T, rows1, K)


# ================================================================================================================ C. backward
def _forward_for_backward(ops, w, act, M, gather=False, excl=None):
    sc = _scorer(ops, w, act, _frag(ops, w))
    if gather:
        T, rows1 = _bag(_bag_rows(M)).to(DEV), _rows(M).to(DEV)
    else:
        T, rows1 = _tokens(M).to(DEV), None
    return sc, ops.abmil_pool_fwd(sc, T, None, rows1=rows1, excl=excl), T


def _backward_both_images(ops, w, sc, st, rows_total, **kw):
    """The backward splitting Wa^T on the fly and with the kind-5 image: bit-equal; returns the image run.  dT starts as a sentinel."""
    wa_t, res = ops.transpose(sc.t[0]), []
    for wf in (None, _frag_t(ops, w)):
        dT = torch.full((rows_total, E), SENTINEL, device=DEV)
        res.append(ops.abmil_pool_bwd(sc, st, _gz().to(DEV), wa_t, need_bias=True, grads={"dT1": dT}, wa_t_frag=wf, **kw))
    for k in ("dT1", "d_wa", "d_wc", "d_ba", "d_bc"):
        assert torch.equal(res[0][k], res[1][k]), k + ": the fragment image changes the result"
    return res[1]


def _check_param_grads(label, g, ref):
    for k in ("d_wa", "d_wc", "d_ba"):
        _check_grad(label + " " + k, g[k], ref[k])
    # d_bc = sum_n ds_n is identically 0 (the softmax is shift invariant): absolute check only
    assert abs(float(g["d_bc"])) < 1e-6 and abs(float(ref["d_bc"])) < 1e-12


@pytest.mark.parametrize("gather", [False, True], ids=["contiguous", "gathered"])
@pytest.mark.parametrize("case", [c for c in BWD_CASES if c[0] > 1], ids=_id)
def test_backward_vs_fp64(case, gather):
    """dT1, d_wa, d_wc, d_ba, d_bc against fp64 autograd.  Gathered: the gradient rows land at rows1 in a sentinel-filled buffer, every
    other row keeps the sentinel bit for bit."""
    ops = _ops()
    M, act, bias = case
    w, ref = _weights(bias), _ref_grad(M, act, bias)
    sc, st, T = _forward_for_backward(ops, w, act, M, gather)
    g = _backward_both_images(ops, w, sc, st, T.shape[0])
    label = "C %s %s" % (_id(case), "gathered" if gather else "contiguous")
    dT = g["dT1"].cpu()
    if gather:
        other = torch.ones(T.shape[0], dtype=torch.bool)
        other[_rows(M)] = False
        assert (dT[other] == SENTINEL).all(), "a row outside rows1 was written"
        dT = dT[_rows(M)]
    if act == "relu":
        for k, got in (("dT", dT), ("d_wa", g["d_wa"]), ("d_ba", g["d_ba"])):           # noted, not asserted: fp64's side of every kink
            _check_grad(label + " " + k + " (no flips)", got, ref[k], check=False)
        ref, flips = _relu_kinks_settled(ref, _tokens(M), w["wa"], dT)
        RATIOS.append((label + " kink entries flipped, of %d" % len(ref["kinks"]), flips))
    _check_grad(label + " dT", dT, ref["dT"])
    _check_param_grads(label, g, ref)


@pytest.mark.parametrize("case", [c for c in BWD_CASES if c[0] == 1], ids=_id)
def test_backward_one_row(case):
    """M = 1: attn = 1, dT = g_z, and every parameter gradient is identically 0 in the reference - relative bounds are void.  dT within
    1e-6 max|g_z| of g_z; each parameter gradient below 1e-5 of the largest entry of the same fp64 gradient at M = 33 (same weights, g_z)."""
    ops = _ops()
    M, act, bias = case
    w, ref, ref33 = _weights(bias), _ref_grad(M, act, bias), _ref_grad(33, act, bias)
    gz = _gz().double()
    for k in ("d_wa", "d_wc", "d_ba", "d_bc"):
        assert float(ref[k].abs().max()) < 1e-12 * max(1.0, float(ref33[k].abs().max()))
    for gather in (False, True):
        sc, st, T = _forward_for_backward(ops, w, act, M, gather)
        g = _backward_both_images(ops, w, sc, st, T.shape[0])
        label = "C %s %s" % (_id(case), "gathered" if gather else "contiguous")
        dT = g["dT1"].cpu()
        if gather:
            other = torch.ones(T.shape[0], dtype=torch.bool)
            other[_rows(M)] = False
            assert (dT[other] == SENTINEL).all()
            dT = dT[_rows(M)]
        _check(label + " dT", dT, gz[None, :], atol=1e-6 * float(gz.abs().max()))
        for k in ("d_wa", "d_wc", "d_ba"):
            _check(label + " " + k, g[k], torch.zeros_like(ref33[k]), atol=1e-5 * float(ref33[k].abs().max()))
        assert abs(float(g["d_bc"])) < 1e-6


@pytest.mark.parametrize("gather", [False, True], ids=["contiguous", "gathered"])
@pytest.mark.parametrize("case", [(95, "tanh", True), (16417, "gelu", False)], ids=_id)
def test_backward_excluded_rows(case, gather):
    """The forward's exclusion mask: an excluded row's gradient is exactly 0, the parameter gradients are those of the live-rows pool."""
    ops = _ops()
    M, act, bias = case
    w, ref, dead = _weights(bias), _ref_grad(M, act, bias, excl=True), _excl_mask(M)
    if gather:
        excl = torch.zeros(_bag_rows(M), dtype=torch.uint8)
        excl[_rows(M)[dead]] = 1
    else:
        excl = dead.to(torch.uint8)
    sc, st, T = _forward_for_backward(ops, w, act, M, gather, excl=excl.to(DEV))
    g = _backward_both_images(ops, w, sc, st, T.shape[0])
    dT = g["dT1"].cpu()
    if gather:
        dT = dT[_rows(M)]
    assert (dT[dead] == 0).all(), "an excluded row has a gradient"
    label = "C excl %s %s" % (_id(case), "gathered" if gather else "contiguous")
    _check_grad(label + " dT", dT, ref["dT"])
    _check_param_grads(label, g, ref)


@pytest.mark.parametrize("deferred", [False, True], ids=["immediate", "reduce_list"])
@pytest.mark.parametrize("case", [(95, "tanh", True), (16417, "relu", False)], ids=_id)
def test_backward_accumulate(case, deferred):
    """accumulate = 1 into pre-filled d_wa / d_wc == base + the plain result to fp32 rounding (1e-6 of the largest entry), with the final
    reductions run at once and queued on a ReduceList that is then flushed."""
    ops = _ops()
    M, act, bias = case
    w, ref = _weights(bias), _ref_grad(M, act, bias)
    sc, st, T = _forward_for_backward(ops, w, act, M)
    wa_t, gz = ops.transpose(sc.t[0]), _gz().to(DEV)
    plain = ops.abmil_pool_bwd(sc, st, gz, wa_t)
    base = {"d_wa": rnd(71, (A, E)) * float(ref["d_wa"].abs().max()), "d_wc": rnd(72, (1, A)) * float(ref["d_wc"].abs().max())}
    acc = {k: v.clone().to(DEV) for k, v in base.items()}
    lst = ops.ReduceList() if deferred else None
    ops.abmil_pool_bwd(sc, st, gz, wa_t, grads=acc, accumulate=True, defer=lst)
    if deferred:
        ops.reduce_flush(lst)
    for k in ("d_wa", "d_wc"):
        want = base[k].double() + plain[k].cpu().double()
        _check("C accumulate %s %s %s" % (_id(case), "list" if deferred else "now", k), acc[k], want, atol=1e-6 * float(want.abs().max()))


def _bf16_split(x):
    hi = x.float().bfloat16().float()
    return hi.double(), (x.float() - hi).bfloat16().double()


def test_backward_peaked_softmax():
    """The forward's peaked inputs.  The fixed 3e-5 is wrong here: the forward's error alone moves the gradients by more (the softmax is
    steep).  The bound is computed from the reference, on the CPU: the error of the three-term split of u (T and Wa split into bf16 hi / lo,
    hi hi + lo hi + hi lo, rounded to fp32) is injected into a second fp64 forward / backward; 4 x the largest change of each gradient,
    relative to its largest entry, is that gradient's atol (4: what the model leaves out - the backward's own three-term product, the fp32
    accumulation order, __expf)."""
    ops = _ops()
    w, X, ref = _peaked()
    th, tl = _bf16_split(X)
    wh, wl = _bf16_split(w["wa"])
    u3 = (th @ wh.t() + tl @ wh.t() + th @ wl.t()).float().double()
    model = _oracle(X, w, "tanh", gz=_gz(), u_err=u3 - X.double() @ w["wa"].double().t())
    sc = _scorer(ops, w, "tanh", _frag(ops, w))
    st = ops.abmil_pool_fwd(sc, X.to(DEV))
    g = _backward_both_images(ops, w, sc, st, PEAK_M)
    for k, name in (("dT1", "dT"), ("d_wa", "d_wa"), ("d_wc", "d_wc"), ("d_ba", "d_ba")):
        moved = float((model[name] - ref[name]).abs().max() / ref[name].abs().max())
        RATIOS.append(("C peaked %s: the CPU model moves it by this share of its max" % name, moved))
        assert 0 < moved < 1e-3
        _check_grad("C peaked " + name, g[k], ref[name], atol_rel=4 * moved)
    assert abs(float(g["d_bc"])) < 1e-6


def _dpre_image_two_pass(ops, dT0, dact, rows, n, n_img):
    """The reference route of test_pool_backward_writes_its_rows_of_the_dpre_image: the fp32 gradient rows dT0, then
    mhimx_rows_dpre_image over a list in which the rows behind n_img are masked out.  Returns (image, bias gradient)."""
    from mhim_mil_amd import _lib as L
    lib = L.lib()
    tiles = -(-n // 32)
    keep = torch.zeros(tiles * 32, dtype=torch.uint8, device=DEV)
    keep[:n_img] = 1
    img = torch.zeros(lib.mhimx_wgrad_image_bytes(tiles * 32, E) // 4, device=DEV)
    b, ws = torch.empty(E, device=DEV), torch.empty(tiles * E, device=DEV)
    dHg = torch.zeros(tiles * 32, E, device=DEV)
    dHg[:n] = dT0[rows]
    dact_g = torch.zeros(tiles * 32, E, device=DEV, dtype=torch.float16)
    dact_g[:n] = dact[rows]
    L.check(lib.mhimx_rows_dpre_image_k(ops._stream(), dHg.data_ptr(), dact_g.data_ptr(), keep.data_ptr(), tiles * 32, E, img.data_ptr(),
                                        b.data_ptr(), 0, ws.data_ptr(), ws.numel() * 4, None), "mhimx_rows_dpre_image_k")
    return img, b


def test_backward_dpre_image_past_one_tile_per_workgroup():
    """mhimx_pool_grad.img with n = 16417 tokens gathered out of a 16500-row bag and img_rows = 16411: workgroups 0 and 1 write two tiles
    of the image each.  The image is byte-identical to the two-pass route, the six rows behind img_rows keep their fp32 dT bit for bit,
    img_part.sum(0) is the column sum of dT * dact."""
    ops = _ops()
    n, n_img, act, bias = 16417, 16411, "tanh", False
    w = _weights(bias)
    sc, st, T = _forward_for_backward(ops, w, act, n, gather=True)
    R, rows = T.shape[0], _rows(n).to(DEV)
    wa_t, gz = ops.transpose(sc.t[0]), _gz().to(DEV)
    dact = (rnd(6, (R, E)).to(DEV) * 0.7).half()
    dT0 = torch.zeros(R, E, device=DEV)
    ops.abmil_pool_bwd(sc, st, gz, wa_t, grads={"dT1": dT0})
    img0, b0 = _dpre_image_two_pass(ops, dT0, dact, rows, n, n_img)
    tiles = -(-n // 32)
    dT1 = torch.zeros(R, E, device=DEV)
    img1 = torch.full_like(img0, float("nan"))
    part = torch.full((tiles, E), float("nan"), device=DEV)
    ops.abmil_pool_bwd(sc, st, gz, wa_t, grads={"dT1": dT1}, img=img1, img_dact=dact, img_part=part, img_rows=n_img)
    torch.cuda.synchronize()
    assert torch.equal(img0.view(torch.int32), img1.view(torch.int32))
    tail = rows[n_img:]
    assert tail.numel() == 6 and torch.equal(dT1[tail], dT0[tail])
    touched = torch.zeros(R, dtype=torch.bool, device=DEV)
    touched[tail] = True
    assert (dT1[~touched] == 0).all()                                      # the image rows' fp32 gradient never went to memory
    _check_grad("C image dT (two-pass route)", dT0[rows].cpu(), _ref_grad(n, act, bias)["dT"])
    ref_b = (dT0[rows[:n_img]].double() * dact[rows[:n_img]].double()).sum(0).cpu()
    tol = 2e-6 * float(ref_b.abs().max()) + 1e-9
    _check("C image img_part.sum(0)", part.double().sum(0), ref_b, atol=tol)
    _check("C image two-pass bias gradient", b0, ref_b, atol=tol)
