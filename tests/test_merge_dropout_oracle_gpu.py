"""Merge (LayerNorm -> cross attention of k global queries over R rows -> to_out -> EMA) with its dropout ON, against the fp64 oracle
(O.merge_tokens with injected keep-masks, autograd for the backward).  GPU box only.

Every training step runs Merge with dropout 0.1 on the attention weights and on the to_out result (mhim.py: Merge(dropout=0.1)); the other
parity tests switch it off.  Here the expected keep-masks are NOT a Python restatement of the counter hash: they are read from the device
through a kernel that is pinned on its own (tests/test_ops_gpu.py::test_gemm_nt_dropout_mask_and_hash) - the non-zero pattern of
ops.gemm_nt(ones, ones, drop_p, drop_seed, drop_tick, prec="f32") is drop_keep(eff_seed(seed, tick), row m, col n, p) (csrc/gemm.hip).
The contract of the Merge kernels (csrc/mca.hip, mca_fused.hip, mca2_rows.hpp, mca2_side.hpp):

  attention keep-mask [8, k, R]   row = slot h * k + i, column = POSITION r in the merge list (not the bag row id), seed s
  output keep-mask    [k, 512]    row = token i, column = e, seed (s + 0x9E3779B97F4A7C15) mod 2^64

both with the device tick folded in by eff_seed.  Kernel forms, as csrc/mca.hip dispatches them (merge2_ok / mca_fused_ok):

  rows16   projection-free form (csrc/mca2.hip: E = 512, 8 x 64 heads, k <= 6, R <= 32768, not exact f32), 16-row tiles: R <= 4096
  rows32   the same with 32-row tiles: R > 4096 (8200 rows = 257 tiles: past one 256-tile chunk of the partial merge)
  general  csrc/mca.hip's own path (K / V projection by GEMM, mca_fwd_part_kernel, mca_bwd_dkv_kernel): k > 6, or prec = "f32"
  tile     the general path with the prep-time fragment image of Wkv (mca_fused.hip): k > 6 only - merge2_ok is asked first, so with
           k <= 6 a MergeW that carries wkv_frag still takes the projection-free form; (33, 7) is the smallest k that reaches it

Bounds: those tests/test_ops_gpu.py::test_merge_fwd_bwd holds with dropout off - forward atol 5e-6 f, rtol 1e-5 f, gradients
atol 5e-5 f max|ref|, rtol 3e-4 f, f = 1 for exact f32 and 4 otherwise (for f = 4 these ARE the bounds of
test_merge_sharded_rows_equal_the_whole_block, which the many-row and the sharded cases take) - times (1 - p)^-2: each of the two masks in
series scales what passes it, and its rounding error, by 1 / (1 - p).  The updated queries q_new = mm q + (1 - mm) z carry (1 - mm) of the
tokens' error on top of the fp32 rounding that test bounds by atol 1e-7, rtol 1e-6.
Every comparison prints its worst error and the worst ratio error / bound before it asserts (pytest -s shows them)."""
import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O
from tests.test_ops_gpu import rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 512
GOLD = 0x9E3779B97F4A7C15
SEED, TICK = 1000, 3                   # (with these, the p = 0.5 cases below have slots with every column dropped AND slots with one kept)
GRADS = {"d_ln_w": "merge.norm.weight", "d_ln_b": "merge.norm.bias", "d_wkv": "merge.attn.to_kv.weight", "d_wq": "merge.attn.to_q.weight",
         "d_wo": "merge.attn.to_out.0.weight", "d_bo": "merge.attn.to_out.0.bias"}
GRAD_SHAPES = {"d_ln_w": (E,), "d_ln_b": (E,), "d_wkv": (1024, E), "d_wq": (512, E), "d_wo": (E, 512), "d_bo": (E,)}


def _ops():
    from mhim_mil_amd import ops
    return ops


def _tick(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def device_masks(k, R, p, seed, tick):
    """(attention keep-mask [8, k, R], output keep-mask [k, 512]) as the device's own keep law draws them (module docstring)."""
    ops = _ops()
    ones = lambda m: torch.ones(m, 64, device=DEV)
    a = ops.gemm_nt(ones(8 * k), ones(R), drop_p=p, drop_seed=seed, drop_tick=tick, prec="f32").cpu()
    o = ops.gemm_nt(ones(k), ones(E), drop_p=p, drop_seed=(seed + GOLD) % 2 ** 64, drop_tick=tick, prec="f32").cpu()
    for m in (a, o):                                                   # kept: 64 / (1 - p); dropped: an exact zero
        assert bool(((m == 0) | ((m * (1 - p) - 64).abs() < 1e-3)).all())
    return (a != 0).view(8, k, R), o != 0


def _scale(p):
    return (1.0 - p) ** -2


def _fwd_bound(prec, p):
    f = 1.0 if prec == "f32" else 4.0
    return 5e-6 * f * _scale(p), 1e-5 * f * _scale(p)


def _grad_bound(prec, p):
    f = 1.0 if prec == "f32" else 4.0
    return 5e-5 * f * _scale(p), 3e-4 * f * _scale(p)


def _q_bound(prec, p, mm):
    a, r = _fwd_bound(prec, p)
    return 1e-7 + (1 - mm) * a, 1e-6 + (1 - mm) * r


def _close(what, name, got, ref, atol, rtol, rel_to=None):
    """|got - ref| <= atol + rtol |rel_to or ref|, element-wise; the figures first."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, dtype=np.float64).reshape(got.shape)
    rel = np.abs(ref if rel_to is None else np.asarray(rel_to.detach().cpu(), dtype=np.float64).reshape(got.shape))
    err = np.abs(got - ref)
    ratio = err / (atol + rtol * rel)
    print(f"[merge_dropout] {what} {name}: max |err| = {err.max():.3e} (max |ref| = {np.abs(ref).max():.3e}), worst err / bound = {ratio.max():.3f}")
    assert np.isfinite(got).all(), f"{what} {name}: not finite"
    assert ratio.max() <= 1.0, f"{what} {name}: max |err| = {err.max():.3e}, worst err / bound = {ratio.max():.3f} (atol {atol:.3e}, rtol {rtol:.3e})"


def _params(k, seed=60):
    """Merge's parameters as tests/test_ops_gpu.py::_merge_fwd_bwd builds them: norm.weight moved off 1, norm.bias and the to_out bias
    non-zero (the dropped-sum statistic of the projection-free form exists only for the bias)."""
    sd = synth.mhim_state(7, input_dim=64, merge_k=k)
    p = {kk: torch.from_numpy(v).double() for kk, v in sd.items() if kk.startswith("merge.")}
    p["merge.norm.weight"] = p["merge.norm.weight"] + rnd(seed + 1, (E,), std=0.1).double()
    p["merge.norm.bias"] = rnd(seed + 2, (E,), std=0.1).double()
    p["merge.attn.to_out.0.bias"] = rnd(seed + 3, (E,), std=0.1).double()
    for kk in p:
        p[kk].requires_grad_(kk != "merge.global_q_mm")
    return p


class _Dev:
    """The fp32 device copies of one parameter set and the MergeW structs made from them."""

    def __init__(self, p, k, frag=False):
        ops = _ops()
        f32 = lambda t: t.detach().float().contiguous().to(DEV)
        self.k = k
        self.q = f32(p["merge.global_q_mm"]).reshape(k, E)
        self.w = [f32(p[n]) for n in ("merge.norm.weight", "merge.norm.bias", "merge.attn.to_kv.weight", "merge.attn.to_q.weight",
                                      "merge.attn.to_out.0.weight", "merge.attn.to_out.0.bias")]
        self.tr = (ops.transpose(self.w[2]), ops.transpose(self.w[3]), ops.transpose(self.w[4]))
        self.img = None
        if frag:
            self.img = torch.empty_like(self.w[2])
            ops.prep_batch([(ops.PREP_FRAG, self.w[2], self.img)])

    def mw(self, mm, prec, p, seed, tick, **kw):
        return _ops().MergeW(self.q, *self.w, mm, prec=prec, transposes=self.tr, drop_p=p, drop_seed=seed, drop_tick=tick, wkv_frag=self.img, **kw)


def _oracle(p, X, mm, masks, drop_p, dz):
    """(z, q_new) and, in X.grad / p[..].grad, the gradients of sum(z * dz)."""
    z, q_new = O.merge_tokens(X, p, mm, True, attn_mask=masks[0], out_mask=masks[1], p=drop_p)
    (z * dz.double()).sum().backward()
    return z.detach(), q_new.detach()


def _uncancelled_scale(p, X, mm, masks, drop_p, dz, name):
    """max |gradient| of parameter ``name`` with the softmax's normaliser held constant: ds = P dP, the first of the two terms of
    ds = P (dP - sum P dP).  The scale for a gradient whose reference vanishes IDENTICALLY because those two terms cancel (R = 1: the
    softmax over one row is 1 whatever its logit, so d_wq = 0) - max |ref| = 0 is no scale, and what a kernel leaves there is the rounding
    residue of two terms of this size, computed along different paths."""
    from unittest import mock

    def softmax_fixed_normaliser(x, dim=-1):
        e = (x - x.max(dim, keepdim=True).values.detach()).exp()
        return e / e.sum(dim, keepdim=True).detach()

    q = {kk: v.detach().clone().requires_grad_(v.requires_grad) for kk, v in p.items()}
    with mock.patch.object(torch, "softmax", softmax_fixed_normaliser):
        z, _ = O.merge_tokens(X.detach(), q, mm, True, attn_mask=masks[0], out_mask=masks[1], p=drop_p)
        (z * dz.double()).sum().backward()
    return float(q[name].grad.abs().max())


def _compare_grads(what, g, dX, X, p, prec, drop_p, zero_scale=None):
    """zero_scale(name): the scale of a parameter gradient whose reference is identically zero (_uncancelled_scale); without it such a
    gradient has to be zero exactly."""
    atol, rtol = _grad_bound(prec, drop_p)
    ref = X.grad
    _close(what, "dX", dX, ref, atol * float(ref.abs().max()), rtol)
    for key, nm in GRADS.items():
        ref = p[nm].grad
        scale = float(ref.abs().max())
        if scale == 0.0 and zero_scale is not None:
            scale = zero_scale(nm)
            print(f"[merge_dropout] {what} {key}: the reference is identically zero; scale of its cancelling terms = {scale:.3e}")
        _close(what, key, g[key], ref, atol * scale, rtol)


def _run(what, R, k, drop_p, prec="bf16x3", frag=False, mm=0.9999, seed=SEED, tick_v=TICK, gathered=False, degenerate=False):
    """One stand-alone merge_fwd / merge_bwd against the oracle.  Returns what the tolerance-free checks need."""
    ops = _ops()
    p = _params(k)
    dev = _Dev(p, k, frag)
    tick = _tick(tick_v)
    masks = device_masks(k, R, drop_p, seed, tick)
    if degenerate:                                                       # a slot whose softmax row is dropped whole, beside one that is not
        kept = masks[0].reshape(8 * k, R).sum(1)
        assert int((kept == 0).sum()) >= 1 and int((kept > 0).sum()) >= 1, "pick another seed: no fully dropped slot / no live slot"
    X = (rnd(64, (R, E)).abs() * 0.7).double().requires_grad_(True)
    dz = rnd(65, (k, E), std=0.1)
    z, q_new = _oracle(p, X, mm, masks, drop_p, dz)
    if gathered:                                                         # the list is a shuffled subset of a bag; every other bag row is NaN
        Nbag = 2 * R + 61
        ids = torch.from_numpy(np.ascontiguousarray(synth.permutation(66, Nbag)[:R]).astype(np.int64))
        Xd = torch.full((Nbag, E), float("nan"))
        Xd[ids] = X.detach().float()
        Xd, rows = Xd.to(DEV), ids.to(DEV)
    else:
        Xd, rows = X.detach().float().contiguous().to(DEV), None
    mw = dev.mw(mm, prec, drop_p, seed, tick, x_rows=rows)
    zd, qn, ws = ops.merge_fwd(mw, Xd)
    _close(what, "z", zd, z, *_fwd_bound(prec, drop_p))
    _close(what, "q_new", qn, q_new, *_q_bound(prec, drop_p, mm))
    if gathered:
        dXbuf = torch.full((Xd.shape[0], E), float("nan"), device=DEV)
        g = ops.merge_bwd(mw, Xd, dz.to(DEV), ws, splits=4, grads={"dX": dXbuf})
        torch.cuda.synchronize()
        written = ~torch.isnan(dXbuf).all(1).cpu()
        assert set(np.nonzero(written.numpy())[0].tolist()) == set(ids.tolist()), "dX: not exactly the listed rows were written"
        dX = dXbuf[rows]
    else:
        g = ops.merge_bwd(mw, Xd, dz.to(DEV), ws, splits=4)
        dX = g["dX"]
    _compare_grads(what, g, dX, X, p, prec, drop_p, zero_scale=lambda nm: _uncancelled_scale(p, X, mm, masks, drop_p, dz, nm))
    return dict(p=p, dev=dev, X=X, Xd=Xd, dz=dz, z=zd, q_new=qn, masks=masks, g=g, oracle_z=z, oracle_q=q_new)


# ------------------------------------------------------------------------------------------------------ 2. kernel level, every form
CASES = [
    pytest.param(1, 5, 0.5, "bf16x3", False, True, id="rows16-R1-k5-p0.5"),
    pytest.param(3, 1, 0.5, "bf16x3", False, True, id="rows16-R3-k1-p0.5"),
    pytest.param(33, 6, 0.1, "bf16x3", False, False, id="rows16-R33-k6"),
    pytest.param(970, 5, 0.1, "bf16x3", False, False, id="rows16-R970-k5"),
    pytest.param(4096, 5, 0.1, "bf16x3", False, False, id="rows16-R4096-k5"),
    pytest.param(300, 5, 0.1, "f16s", False, False, id="rows16-R300-k5-f16s"),
    pytest.param(4097, 5, 0.1, "bf16x3", False, False, id="rows32-R4097-k5"),
    pytest.param(8200, 3, 0.1, "bf16x3", False, False, id="rows32-R8200-k3"),
    pytest.param(300, 10, 0.1, "bf16x3", False, False, id="general-R300-k10"),
    pytest.param(33, 5, 0.1, "f32", False, False, id="general-R33-k5-f32"),
    pytest.param(2000, 16, 0.1, "bf16x3", True, False, id="tile-R2000-k16"),
    pytest.param(33, 7, 0.1, "bf16x3", True, False, id="tile-R33-k7"),
]


@pytest.mark.parametrize("R,k,drop_p,prec,frag,degenerate", CASES)
def test_merge_with_dropout_vs_oracle(R, k, drop_p, prec, frag, degenerate):
    """z, q_new, dX and the six parameter gradients of merge_fwd / merge_bwd with dropout p, every kernel form (module docstring)."""
    _run(f"R={R} k={k} p={drop_p} {prec}{' frag' if frag else ''}", R, k, drop_p, prec, frag, degenerate=degenerate)


def test_merge_with_dropout_gathered_rows():
    """(970, 5, 0.25) with x_rows a shuffled subset of a bag whose other rows are NaN: the mask column is the list position (a kernel that
    hashed the bag row id misses the oracle), dX lands in exactly the listed rows of a NaN-filled buffer."""
    _run("gathered R=970 k=5 p=0.25", 970, 5, 0.25, gathered=True)


def test_merge_with_dropout_ema_uses_the_dropped_tokens():
    """mm = 0.9: q_new = mm q + (1 - mm) z moves by a tenth of z, so the comparison sees which z went into it - the oracle's q_new with the
    masks lies far outside the bound of its q_new without them."""
    R, k, drop_p, mm = 300, 5, 0.1, 0.9
    r = _run("ema R=300 k=5 mm=0.9", R, k, drop_p, mm=mm)
    _, q_plain = O.merge_tokens(r["X"].detach(), {kk: v.detach() for kk, v in r["p"].items()}, mm, True)
    atol, rtol = _q_bound("bf16x3", drop_p, mm)
    gap = ((q_plain - r["oracle_q"]).abs() / (atol + rtol * r["oracle_q"].abs())).max()
    assert float(gap) > 100.0, f"the dropped and the plain tokens give queries only {float(gap):.1f} bounds apart"


def test_merge_with_dropout_exact_properties():
    """What needs no tolerance, on (970, 5, 0.1): the zero pattern of z is the output mask; same seed and tick, same bits; tick t + 1 draws
    gemm_nt's pattern of tick t + 1, another one than tick t's, and the tokens follow the attention mask of t + 1 too; a seed above 2^32
    draws by its high word (other masks than the low word alone) and the kernels follow it, forward and backward."""
    ops = _ops()
    R, k, drop_p = 970, 5, 0.1
    r = _run("exact R=970 k=5", R, k, drop_p)
    assert torch.equal(r["z"].cpu() != 0, r["masks"][1])
    dev, Xd, dz = r["dev"], r["Xd"], r["dz"].to(DEV)
    mw = dev.mw(0.9999, "bf16x3", drop_p, SEED, _tick(TICK))
    z2, q2, ws2 = ops.merge_fwd(mw, Xd)
    g2 = ops.merge_bwd(mw, Xd, dz, ws2, splits=4)
    assert torch.equal(z2, r["z"]) and torch.equal(q2, r["q_new"])
    for key in ("dX",) + tuple(GRADS):
        assert torch.equal(g2[key], r["g"][key]), key
    # the tick
    t1 = _tick(TICK + 1)
    m1 = device_masks(k, R, drop_p, SEED, t1)
    assert not torch.equal(m1[0], r["masks"][0]) and not torch.equal(m1[1], r["masks"][1])
    z3, _, _ = ops.merge_fwd(dev.mw(0.9999, "bf16x3", drop_p, SEED, t1), Xd)
    assert torch.equal(z3.cpu() != 0, m1[1]) and not torch.equal(z3.cpu() != 0, r["masks"][1])
    p0 = {kk: v.detach() for kk, v in r["p"].items()}
    z_ref, _ = O.merge_tokens(r["X"].detach(), p0, 0.9999, True, attn_mask=m1[0], out_mask=m1[1], p=drop_p)
    _close("exact tick + 1", "z", z3, z_ref, *_fwd_bound("bf16x3", drop_p))
    # the high word of the seed
    hi = SEED + (7 << 32)
    rh = _run("exact seed > 2^32", R, k, drop_p, seed=hi)
    assert not torch.equal(rh["masks"][0], r["masks"][0]) and not torch.equal(rh["masks"][1], r["masks"][1])
    assert torch.equal(rh["z"].cpu() != 0, rh["masks"][1])


@pytest.mark.parametrize("R,k", [pytest.param(970, 5, id="rows16-R970-k5"), pytest.param(300, 10, id="general-R300-k10")])
def test_merge_with_dropout_accumulates_and_defers(R, k):
    """accumulate=True onto non-zero gradient buffers, immediately and with the final reductions queued on a ReduceList and flushed: both
    hold the oracle's gradient + what the buffers held, at the gradient bound (taken on the gradient, not on the sum)."""
    ops = _ops()
    drop_p = 0.1
    r = _run(f"accumulate R={R} k={k}", R, k, drop_p)
    p, dev, Xd, dz = r["p"], r["dev"], r["Xd"], r["dz"].to(DEV)
    atol, rtol = _grad_bound("bf16x3", drop_p)
    base = {key: rnd(70 + i, GRAD_SHAPES[key]) * float(p[nm].grad.abs().max()) for i, (key, nm) in enumerate(GRADS.items())}
    for deferred in (False, True):
        mw = dev.mw(0.9999, "bf16x3", drop_p, SEED, _tick(TICK))
        _, _, ws = ops.merge_fwd(mw, Xd)
        bufs = {key: v.clone().to(DEV) for key, v in base.items()}
        lst = ops.ReduceList() if deferred else None
        g = ops.merge_bwd(mw, Xd, dz, ws, splits=4, grads=dict(bufs), accumulate=True, defer=lst)
        if deferred:
            ops.reduce_flush(lst)
        torch.cuda.synchronize()
        what = f"accumulate R={R} k={k} {'deferred' if deferred else 'immediate'}"
        _close(what, "dX", g["dX"], r["X"].grad, atol * float(r["X"].grad.abs().max()), rtol)
        for key, nm in GRADS.items():
            ref = p[nm].grad
            assert g[key].data_ptr() == bufs[key].data_ptr()
            _close(what, key, g[key], ref + base[key].double(), atol * float(ref.abs().max()), rtol, rel_to=ref)


# ------------------------------------------------------------------------------------------------------ 3. composite forms
def test_ridden_rows_pass_with_dropout_equals_the_plain_forward():
    """The rows pass of the prepared projection-free form riding in the student's scorer launch (abmil_pool_fwd_split(ride_merge=...), then
    merge_fwd(rows_done=True)) at p = 0.1: tokens, queries and - from the workspace that pass left - every gradient equal a plain
    merge_fwd / merge_bwd bit for bit (which the cases above hold against the oracle)."""
    from mhim_mil_amd import _lib as L
    ops = _ops()
    N, R, Lk, k, A, drop_p = 1200, 333, 500, 5, 128, 0.1                   # 333 rows: 20 tiles of 16 and one of 13
    p = _params(k)
    dev = _Dev(p, k)
    Hbuf = torch.zeros(N + k, E, device=DEV)
    Hbuf[:N] = (rnd(81, (N, E)).abs() * 0.7).to(DEV)
    perm = torch.from_numpy(synth.permutation(82, N).copy()).to(DEV)
    merge_rows, stay = perm[:R].contiguous(), perm[R:R + Lk]
    rows1 = torch.cat([stay, N + torch.arange(k, device=DEV)]).contiguous()
    sc = ops.ScorerW(rnd(83, (A, E), std=0.05).to(DEV), rnd(84, (1, A), std=0.3).to(DEV), L.ACT["relu"], prec="bf16x3")
    dz = rnd(85, (k, E), std=0.1).to(DEV)
    tick = _tick(TICK)
    plain = dev.mw(0.9999, "bf16x3", drop_p, SEED, tick, x_rows=merge_rows)
    z0, q0, ws0 = ops.merge_fwd(plain, Hbuf)
    dX0 = torch.zeros(N + k, E, device=DEV)
    g0 = ops.merge_bwd(plain, Hbuf, dz, ws0, splits=4, grads={"dX": dX0})
    prepared = dev.mw(0.9999, "bf16x3", drop_p, SEED, tick, x_rows=merge_rows, prepared=True)
    ws1 = prepared.ws_for(R, DEV)
    ops.prep_batch([(ops.PREP_MERGE, prepared, (ws1, R))])
    st, rode = ops.abmil_pool_fwd_split(sc, Hbuf, rows1, k, ride_merge=(prepared, Hbuf, ws1))
    assert rode, "the rows pass did not ride"
    z1, q1, _ = ops.merge_fwd(prepared, Hbuf, ws=ws1, rows_done=True)
    dX1 = torch.zeros(N + k, E, device=DEV)
    g1 = ops.merge_bwd(prepared, Hbuf, dz, ws1, splits=4, grads={"dX": dX1})
    torch.cuda.synchronize()
    assert torch.equal(z1, z0) and torch.equal(q1, q0)
    assert int((z0 == 0).sum()) > 0 and torch.equal(z0.cpu() != 0, device_masks(k, R, drop_p, SEED, tick)[1])
    assert torch.equal(dX1, dX0) and float(dX0[merge_rows].abs().max()) > 0
    for key in GRADS:
        assert torch.equal(g1[key], g0[key]), key


@pytest.mark.parametrize("R,W,order", [pytest.param(45, 3, "shuffled", id="R45-W3-shuffled"), pytest.param(970, 2, "ascending", id="R970-W2")])
def test_sharded_merge_with_dropout_vs_oracle(R, W, order):
    """merge_fwd_part / merge_fwd_finish / merge_bwd(own=...) over W shards of the bag, p = 0.1: every shard draws the columns of the WHOLE
    list (the oracle gets the whole-list masks), finishes with equal bits, and tokens and summed gradients meet
    tests/test_round4_gpu.py::test_merge_sharded_rows_equal_the_whole_block's bounds x (1 - p)^-2."""
    ops = _ops()
    k, drop_p, mm = 5, 0.1, 0.9999
    what = f"sharded R={R} W={W}"
    Nbag = 4 * R + 7 * W
    p = _params(k, seed=160)
    dev = _Dev(p, k)
    tick = _tick(TICK)
    masks = device_masks(k, R, drop_p, SEED, tick)
    Hbag = rnd(164, (Nbag, E)).abs() * 0.7
    ids = synth.permutation(165, Nbag)[:R]
    ids = np.ascontiguousarray(np.sort(ids) if order == "ascending" else ids).astype(np.int64)
    X = Hbag[torch.from_numpy(ids)].double().requires_grad_(True)
    dz = rnd(166, (k, E), std=0.1)
    z, q_ref = _oracle(p, X, mm, masks, drop_p, dz)
    rows = torch.from_numpy(ids).to(DEV)
    bounds = [Nbag * r // W for r in range(W + 1)]
    mws, parts, wss, Hloc = [], [], [], []
    for r in range(W):
        lo, n = bounds[r], bounds[r + 1] - bounds[r]
        mw = dev.mw(mm, "bf16x3", drop_p, SEED, tick, x_rows=rows, own=(lo, n), rep=1.0 if r == 0 else 0.0)
        h = Hbag[lo:lo + n].to(DEV).contiguous()
        part, ws = ops.merge_fwd_part(mw, h)
        mws.append(mw); parts.append(part); wss.append(ws); Hloc.append(h)
    allparts = torch.stack(parts).contiguous()
    zs = [ops.merge_fwd_finish(mws[r], allparts, wss[r]) for r in range(W)]
    for zr, qr in zs:
        assert torch.equal(zr, zs[0][0]) and torch.equal(qr, zs[0][1])
    assert torch.equal(zs[0][0].cpu() != 0, masks[1])
    _close(what, "z", zs[0][0], z, *_fwd_bound("bf16x3", drop_p))
    _close(what, "q_new", zs[0][1], q_ref, *_q_bound("bf16x3", drop_p, mm))
    total = {kk: 0 for kk in GRADS}
    dX = torch.zeros((R, E))
    for r in range(W):
        lo, n = bounds[r], bounds[r + 1] - bounds[r]
        dH = torch.full((n, E), float("nan"), device=DEV)
        g = ops.merge_bwd(mws[r], Hloc[r], dz.to(DEV), wss[r], grads={"dX": dH})
        torch.cuda.synchronize()
        own = (ids >= lo) & (ids < lo + n)
        written = ~torch.isnan(dH[:, 0]).cpu().numpy()
        assert set(np.nonzero(written)[0].tolist()) == set((ids[own] - lo).tolist())
        dX[torch.from_numpy(np.nonzero(own)[0])] = dH[torch.from_numpy(ids[own] - lo).to(DEV)].cpu()
        for kk in GRADS:
            total[kk] = total[kk] + g[kk].double().cpu()
    _compare_grads(what, total, dX, X, p, "bf16x3", drop_p)


# ------------------------------------------------------------------------------------------------------ 4. the native train calls
# tests/test_step_middle_gpu.py's trainers (D = 256, merge_k = 5, feature dropout 0.25 on both models), Merge's dropout left at 0.1.
MERGE_P = 0.1
MERGE_NAMES = tuple(GRADS.values())


def _trainer_with_merge_dropout(accum=1):
    from tests.test_step_middle_gpu import _trainer
    tr = _trainer(True, 0.5, accum=accum)
    tr.s.merge.dropout = tr.t.merge.dropout = MERGE_P                  # (_mk switched it off; the step's cfg reads it on every call)
    return tr


def _token_pattern_is(tokens, R, seed, tick, what):
    """The zero pattern of a bag's tokens is the output keep-mask of its Merge seed at the step's tick value."""
    out_mask = device_masks(5, R, MERGE_P, seed, tick)[1]
    got = tokens.cpu() != 0
    assert 0 < int((~got).sum()) and torch.equal(got, out_mask), f"{what}: {int((got != out_mask).sum())} token elements off the output mask"
    return got


def test_step_run_with_merge_dropout_vs_oracle():
    """mhimx_step_run (forward_backward, update = 0) on a bag of 600 rows, Merge dropout 0.1 beside the 0.25 feature dropouts: the row list,
    the teacher scores and the projection keep-masks are read back as tests/test_single_pass_gpu.py::
    test_production_step_with_dropout_vs_oracle_c2 does, the Merge masks come from seeds.mca and the tick value the call ran at (the
    preparation launch advances the counter first: the value it holds after the call).  Against O.train_step in fp64: logits at that test's
    1e-4, Merge's parameter gradients at its 2e-3 of scale / 2e-3 relative, the student's tokens at 1e-4 absolute (the bound
    tests/test_step_middle_gpu.py gives tokens and logits alike, both functions of the projected feature rows) - each x (1 - p)^-2; the
    tokens' zero pattern is the output mask exactly."""
    from tests.test_single_pass_gpu import _draws_from_device
    from tests.test_step_middle_gpu import D, KM, N1, V2, _bags, _record_seeds
    (x,), (y,) = _bags([N1], 400)
    tr = _trainer_with_merge_dropout()
    drawn = _record_seeds(tr)
    logits, losses = tr.forward_backward(x, y)
    torch.cuda.synchronize()
    assert tr.last["exec"] is True and len(drawn) == 4 and abs(float(tr._exec["cfg"].merge_drop_p) - MERGE_P) < 1e-7
    tick, mca, R = tr.tick.clone(), drawn[3], int(tr.last["R"])
    keep_t, keep_s = (tr.last["H_teacher"] != 0).cpu(), (tr.last["H_student"] != 0).cpu()
    rows, score = tr.last["rows"].cpu().numpy(), tr.last["score"].cpu().numpy()
    tokens = tr.last["tokens"].clone()
    attn_mask, out_mask = device_masks(KM, R, MERGE_P, mca, tick)
    _token_pattern_is(tokens, R, mca, tick, "step")
    cfg = dict(V2, attn2score=True, dropout=0.25)
    k, n_sel, _ = O.mask_count(N1, cfg["mask_ratio_h"], cfg["mask_ratio_hr"])
    perm, shuf = _draws_from_device(score, rows, R, N1, k, n_sel)
    base = synth.mhim_state(7, input_dim=D, merge_k=KM)
    stu, tea = O.as_torch(base, torch.float64), O.as_torch(synth.spread_teacher(base), torch.float64)
    bag = x[0].cpu().double()
    merge_kw = dict(attn_mask=attn_mask, out_mask=out_mask, p=MERGE_P)
    _, _, _, info = O.train_step(bag, int(y), stu, tea, {}, O.Cfg(**cfg), 1, perm=perm, ids_shuffle=shuf, aux_alpha=0.5, mm=0.9997,
                                 score_override=torch.from_numpy(score), drop_mask_t=keep_t, drop_mask_s=keep_s, merge_kw=merge_kw)
    h = O.feature(bag, stu, cfg["act"], keep_s, 0.25)
    z_ref, _ = O.merge_tokens(h[torch.from_numpy(rows[:R].copy())], stu, cfg["merge_mm"], True, **merge_kw)
    s = _scale(MERGE_P)
    _close("step", "tokens", tokens, z_ref, 1e-4 * s, 0.0)
    _close("step", "logits", logits.reshape(-1), info["logits"].reshape(-1), 1e-4 * s, 0.0)
    gv = tr.flat.grad_views
    for name in MERGE_NAMES:
        ref = info["grads"][name]
        _close("step", "grad " + name, gv[name], ref, 2e-3 * s * float(ref.abs().max()), 2e-3 * s)


def _merge_grads_close(tr, g_win, g_sum, what):
    """The ragged comparison of tests/test_step_middle_gpu.py (_grads_close: atol = rtol = 2e-3 of scale) on Merge's six gradients."""
    fl = tr.flat
    for name in MERGE_NAMES:
        sl = slice(fl.offsets[name], fl.offsets[name] + fl.grad_views[name].numel())
        ref = g_sum[sl]
        _close(what, "grad " + name, g_win[sl], ref, 2e-3 * float(ref.abs().max()), 2e-3)


def test_same_shape_window_with_merge_dropout_vs_single_bag_steps():
    """mhimx_window_run over two bags of 600 rows, Merge dropout 0.1: every bag's rows, score, tokens and logits are bit-equal to
    mhimx_step_run(update = 0) on that bag alone with the bag's seeds (tests/test_step_middle_gpu.py's relation - the batched launches
    derive bag b's Merge seed through bag_mca_seed); each bag's token zero pattern is the output mask of ITS seed and the two differ;
    Merge's accumulated gradients equal the single-bag gradients summed / 2 at the bound that file gives a window's gradient."""
    from mhim_mil_amd import _lib as L
    from tests.test_step_middle_gpu import N1, _alone, _bags, _equal, _record_seeds
    xs, ys = _bags([N1, N1], 410)
    tr, tr1 = _trainer_with_merge_dropout(accum=2), _trainer_with_merge_dropout()
    q0, tick0 = tr.s.merge.global_q_mm.data.clone(), tr.tick.clone()
    drawn = _record_seeds(tr)
    tr.window_step(xs, ys, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == "mhimx_window_run" and len(drawn) == 8
    tick = tr.tick.clone()
    (cnt, _), = tr._exec["layouts"].values()
    per = [{k: p[k].clone() for k in ("rows", "score", "tokens", "logits")} for p in tr.last["bags"]]
    g_win = tr.flat.grad.clone()
    pats, g_sum = [], 0
    for j in range(2):
        seeds = L.StepSeeds(drop_teacher=drawn[2 * j], drop_student=drawn[2 * j + 1], select=drawn[4 + 2 * j], mca=drawn[5 + 2 * j])
        one, g_one = _alone(tr1, xs[j], ys[j], cnt, seeds, q0, tick0)
        assert torch.equal(tr1.tick, tick)
        for key in ("rows", "score", "tokens", "logits"):
            _equal(per[j][key], one[key], f"bag {j} {key}")
        pats.append(_token_pattern_is(per[j]["tokens"], int(cnt.R), drawn[5 + 2 * j], tick, f"bag {j}"))
        g_sum = g_sum + g_one.double() / 2
    assert drawn[5] != drawn[7] and not torch.equal(pats[0], pats[1])
    _merge_grads_close(tr, g_win, g_sum, "window")


def test_same_shape_window_merge_seed_alone_sets_the_pattern():
    """One bag twice in a window, every seed scripted.  The same seeds for both: equal rows and bit-equal tokens.  Only the Merge seed of
    the second bag changed: equal rows still, and each bag's tokens carry the output mask of its own seed - two different patterns."""
    from tests.test_step_middle_gpu import N1, _bags
    (x,), _ = _bags([N1], 430)
    xs, ys = [x, x.clone()], [torch.tensor([1], device=DEV), torch.tensor([1], device=DEV)]
    a, b, c, d, d2 = 1111, 2222 + (3 << 32), 3333, 4444 + (5 << 32), 5555
    for mca1, same in ((d, True), (d2, False)):
        tr = _trainer_with_merge_dropout(accum=2)           # (a fresh accumulation window each time)
        script = iter([a, b, a, b, c, d, c, mca1])          # (both bags' dropout seeds first, then bag after bag select and Merge)
        for m in (tr.s, tr.t):
            m._next_seed = lambda teacher=False, _it=script: next(_it)
        tr.window_step(xs, ys, update=False)
        torch.cuda.synchronize()
        assert tr.last["exec"] == "mhimx_window_run" and next(script, None) is None
        tick = tr.tick.clone()
        bags = tr.last["bags"]
        R = int(bags[0]["R"])
        assert torch.equal(bags[0]["rows"], bags[1]["rows"]) and torch.equal(bags[0]["score"], bags[1]["score"])
        p0 = _token_pattern_is(bags[0]["tokens"], R, d, tick, "bag 0")
        p1 = _token_pattern_is(bags[1]["tokens"], R, mca1, tick, "bag 1")
        if same:
            assert torch.equal(bags[0]["tokens"], bags[1]["tokens"])
        else:
            assert not torch.equal(p0, p1)


def test_ragged_window_with_merge_dropout_vs_single_bag_steps():
    """mhimx_ragged_window_run over bags {64, 600, 333}, Merge dropout 0.1, against mhimx_step_run(update = 0) on each bag alone with the
    window's seeds, by tests/test_step_middle_gpu.py's relations for a ragged window: row lists bit-equal, score atol 1e-4 / rtol 2e-3,
    tokens and logits 1e-4 absolute (a dropped token element is an exact zero on both sides), Merge's gradients against the single-bag
    gradients summed / 3 at atol = rtol = 2e-3 of scale; every bag's token zero pattern is the output mask of its own Merge seed, and the
    three patterns differ."""
    from tests.test_step_middle_gpu import RAGGED, _alone, _bags, _equal
    xs, ys = _bags(RAGGED, 420)
    n = len(RAGGED)
    tr, tr1 = _trainer_with_merge_dropout(accum=n), _trainer_with_merge_dropout()
    q0, tick0 = tr.s.merge.global_q_mm.data.clone(), tr.tick.clone()
    tr.window_step(xs, ys, update=False)
    torch.cuda.synchronize()
    assert tr.last["exec"] == "mhimx_ragged_window_run"
    tick, table = tr.tick.clone(), tr.last["table"]
    per = [{k: p[k].clone() for k in ("rows", "score", "tokens", "logits")} for p in tr.last["bags"]]
    g_win = tr.flat.grad.clone()
    g_sum, seen, pats = 0, set(), []
    for j in range(n):
        one, g_one = _alone(tr1, xs[j], ys[j], table[j].cnt, table[j].seeds, q0, tick0)
        assert torch.equal(tr1.tick, tick)
        _equal(per[j]["rows"], one["rows"], f"ragged bag {j} rows")
        _close(f"ragged bag {j}", "score", per[j]["score"], one["score"], 1e-4, 2e-3)
        _close(f"ragged bag {j}", "tokens", per[j]["tokens"], one["tokens"], 1e-4, 0.0)
        _close(f"ragged bag {j}", "logits", per[j]["logits"], one["logits"], 1e-4, 0.0)
        mca = int(table[j].seeds.mca)
        pats.append(_token_pattern_is(per[j]["tokens"], int(table[j].cnt.R), mca, tick, f"ragged bag {j}"))
        _token_pattern_is(one["tokens"], int(table[j].cnt.R), mca, tick, f"bag {j} alone")
        seen.add(mca)
        g_sum = g_sum + g_one.double() / n
    assert len(seen) == n and not any(torch.equal(pats[i], pats[j]) for i in range(n) for j in range(i))
    _merge_grads_close(tr, g_win, g_sum, "ragged window")
    tr.flat.grad.zero_()
