"""The tail of every train step (csrc/optim.hip) against plain fp64 references computed on the CPU from the same fp32 inputs and the fp32
values of the by-value constants - not against another form of itself, except where the contract IS bit equality.

Which case reaches what
  head_fast_kernel<2>   test_head_matches_fp64[1-1 | 1-2 | 200-2 | 512-4]; accumulate / NULL gradients / autograd form on 200-2, peaked on 512-4
  head_fast_kernel<4>   test_head_matches_fp64[513-3 | 1000-4 | 1024-1]; accumulate / NULL gradients / autograd form / peaked on 1000-4
  head_kernel           test_head_matches_fp64[1025-2 | 512-5 | 300-16 | 2048-2 | 5000-3]; accumulate / NULL / autograd on 300-16, peaked on 5000-3
  dsmil_head_kernel     test_dsmil_head_matches_fp64, test_dsmil_head_label_free_forms
  adam_ema_kernel       vector path: every aligned case; scalar path: test_update_plain[1-1 | 3-3 | 5-8 | 4098-4103 | 1023-1030] (the tail and the
                        quad that straddles n_train), test_update_unaligned (everything), test_update_slabs[...-unaligned]; the grid-stride
                        loop: test_update_plain[2098179-2098183]
  each term             test_update_terms (weight decay, eps, grad_scale, betas, step 1 / 2 / 1000 / 100000)
  step_dev, schedules   test_update_device_step, test_update_schedules
  g_extra slabs         test_update_slabs (extra_lo, extra_only, the straddling quad, both paths)
  grad_sumsq_kernel     test_update_clipping (with grad_scale, slabs + extra_lo + extra_only, weight decay; one block and 1024 blocks)
  fold                  test_update_fold_* (bit-equal to mhimx_reduce_flush + an update without the list, and inside the oracle bounds)

Buffer discipline: every device buffer is a view into a larger NaN-filled allocation whose guard elements must still be NaN afterwards;
what the contract says is not read is NaN: slab elements below extra_lo and behind n_train (up to the pitch), g from extra_lo on under
extra_only, g behind n_train, g under a non-accumulating reduction job, ws before a clipping call, d_wp / d_bp without accumulate.

Bounds (u = 2^-24; derived from operation counts, never from what the kernels return; no element is left out)
  heads      logits atol 2e-6 rtol 1e-5 | losses atol 2e-5 rtol 1e-5 | gradients atol 1e-7 rtol 2e-4   (test_head_fwd_bwd, tests/test_ops_gpu.py)
             peaked case: the same rtol, atol x max(1, largest |fp64 result| of that tensor): the logits, the log-softmax terms and z are
             50 - 160 there and an fp32 rounding is relative to them; never below the unpeaked atol, since softmax - onehot carries an
             absolute error of u whatever the size of the result
  DSMIL head losses rtol 2e-5 (atol 0) | g_lb, g_li 1e-5 max|ref| | g_B 1e-4 max|ref|                   (test_dsmil_head_kernel)
  update     S = (|g| + sum|slab|) |grad_scale coef| + wd |w|;   k = fp32 additions on the longest chain into one summed gradient element
             |m - m64| <= (6 + k) u (b1 |m0| + (1 - b1) S)        |v - v64| <= (10 + 2k) u (b2 v0 + (1 - b2) S^2)
             p from the kernel's own m, v:  D = (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),  |p - (p0 - D)| <= u |p0 - D| + 8 u |D|
             teacher from the kernel's own p:  |t - t64| <= 3 u (mm |t0| + (1 - mm) |p|)
  k          0 without slabs; n_extra with slabs; a reduction job of G slabs (reduce_jobs.hpp, fold_sum4): the running sum s0 takes
             G // 4 + G % 4 values, i.e. max(G // 4 + G % 4 - 1, 0) rounded additions, then (s0 + s1) + (s2 + s3) and the accumulate: + 3.
             (For G % 4 == 0 that is G / 4 + 2; it exceeds G / 4 + 3 by at most G % 4 - 1 - (G % 4) / 4 < 2 when G % 4 != 0.)
             A kind-0 job of G <= 32 partials: one value per row group, then G - 1 rounded additions of non-zeros and the accumulate: G.
  clipping   coef = min(1, c / (sqrt(SS) + 1e-6)) in fp64 from the same inputs, SS = sum v_i^2, v_i = (g + slabs)_i grad_scale.  The kernels'
             sum of squares passes at most 24 rounded additions (grad_sumsq_kernel: <= 4 serial per thread at 1 048 581 elements - five
             elements, the first addition is to 0 - and 8 tree levels; adam_ema_kernel: 3 serial over the 1024 parts and 8 tree levels),
             the square root halves that, then the root and the division: the coefficient is within 14 u, which joins k where coef < 1
             (k += 14).  coef = 1 exactly when the norm is below c: bit-equal to the call without clipping.

fold with zero_grad = 0 is not compared: a folded job's sum never reaches g (it is added in registers), a flushed one's does; the
trainers always clear the gradient.  Jobs with overlapping outputs are not part of the contract.

Every comparison notes its largest error over its bound in RATIOS before it asserts; with MHIMX_ORACLE_RATIOS=<path> in the environment
the list is written there as JSON when the module is done (profiles/head_optim_oracle.md is filled from it)."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from mhim_mil_amd import synth
from oracle import mhim_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
NAN = float("nan")
PAD = 8                # guard floats on either side of every buffer (32 bytes: the view stays 16-byte aligned)
RATIOS = []            # (label, largest error / bound), in order


def f32(x):
    return float(np.float32(x))


def rnd(seed, shape, std=1.0):
    return torch.from_numpy(synth.normal(seed, shape, std=std).astype(np.float32))


def _note(label, r):
    RATIOS.append((label, float(r)))


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    if os.environ.get("MHIMX_ORACLE_RATIOS"):
        with open(os.environ["MHIMX_ORACLE_RATIOS"], "w") as f:
            json.dump(RATIOS, f)


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ratio(err, bound):
    """max err / bound; 0 / 0 = 0, x / 0 = inf."""
    err, bound = err.double().reshape(-1), bound.double().reshape(-1)
    if err.numel() == 0:
        return 0.0
    assert torch.isfinite(err).all() and torch.isfinite(bound).all()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def _close(label, got, ref, atol, rtol=0.0):
    got = got.detach().double().cpu().reshape(-1)
    ref = ref.detach().double().reshape(-1)
    assert got.shape == ref.shape, label
    assert torch.isfinite(got).all(), label + ": not finite"
    r = _ratio((got - ref).abs(), atol + rtol * ref.abs())
    _note(label, r)
    assert r <= 1.0, "%s: largest error is %.4g of its bound" % (label, r)


class Buf:
    """``n`` floats at element ``off`` of a NaN-filled allocation of off + n + PAD (off = PAD: 16-byte aligned, PAD + 1: not)."""

    def __init__(self, data, off=PAD):
        data = data.reshape(-1)
        self.n, self.off = data.numel(), off
        self.store = torch.full((off + self.n + PAD,), NAN, dtype=torch.float32, device=DEV)
        self.t = self.store[off:off + self.n]
        self.t.copy_(data)
        assert (self.t.data_ptr() % 16 == 0) == (off % 4 == 0)

    @classmethod
    def nans(cls, n, off=PAD):
        return cls(torch.full((n,), NAN), off)

    def cpu(self):
        return self.t.detach().cpu().clone()

    def guards_intact(self):
        s = self.store.detach().cpu()
        return bool(torch.isnan(s[:self.off]).all() and torch.isnan(s[self.off + self.n:]).all())


def _p(x):
    from mhim_mil_amd import ops
    return ops._p(x.t if isinstance(x, Buf) else x)


# ================================================================================================================== A. heads
MAIN, AUX, INV = 0.7, 0.3, 0.125
LOGIT_TOL, LOSS_TOL, GRAD_TOL = (2e-6, 1e-5), (2e-5, 1e-5), (1e-7, 2e-4)
HEAD_SHAPES = {"fast2": [(1, 1), (1, 2), (200, 2), (512, 4)], "fast4": [(513, 3), (1000, 4), (1024, 1)],
               "generic": [(1025, 2), (512, 5), (300, 16), (2048, 2), (5000, 3)]}
ALL_HEAD_SHAPES = [s for k in ("fast2", "fast4", "generic") for s in HEAD_SHAPES[k]]
ONE_PER_KERNEL = [(200, 2), (1000, 4), (300, 16)]
PEAKED_SHAPES = [(512, 4), (1000, 4), (5000, 3)]
_sid = lambda s: "%d-%d" % s


def _head_call(z, t, wp, bp, label, E, Cc, temp_t, main, aux, inv, logits, losses, g_z, d_wp, d_bp, accumulate, g_logits_in, g_cl_in):
    from mhim_mil_amd import _lib as L, ops
    L.check(L.lib().mhimx_head_fwd_bwd(ops._stream(), _p(z), None if t is None else _p(t), _p(wp), None if bp is None else _p(bp),
                                       None if label is None else _p(label), E, Cc, float(temp_t), float(main), float(aux), float(inv),
                                       _p(logits), _p(losses), _p(g_z), None if d_wp is None else _p(d_wp),
                                       None if d_bp is None else _p(d_bp), int(accumulate), None if g_logits_in is None else _p(g_logits_in),
                                       None if g_cl_in is None else _p(g_cl_in)), "mhimx_head_fwd_bwd")


@functools.lru_cache(maxsize=None)
def _head_inputs(E, Cc, peaked=False, temp_t=0.1):
    """z, t, wp, bp (+ non-zero accumulation bases).  peaked: z spread over +-80, t / temp_t over +-150, the rows of wp scaled so that the
    logits are -50, +50, 10, -20: the arg max is class 1, so that neither label 0 nor label C - 1 is (for the arg max class the fp64
    gradient is ~1e-40 and softmax - 1 is exactly 0 in fp32 - the absolute regime that the unpeaked cases' atol covers)."""
    seed = 1000 + 17 * E + Cc
    d = dict(z=rnd(seed, (E,), std=0.5), t=rnd(seed + 1, (E,), std=0.5), wp=rnd(seed + 2, (Cc, E), std=0.06), bp=rnd(seed + 3, (Cc,), std=0.1),
             dwp0=rnd(seed + 4, (Cc, E), std=0.2), dbp0=rnd(seed + 5, (Cc,), std=0.2), gl=rnd(seed + 6, (Cc,), std=0.3))
    if peaked:
        lin = torch.linspace(-1.0, 1.0, E, dtype=torch.float64)
        d["z"] = (80.0 * lin[torch.from_numpy(synth.permutation(seed + 7, E).copy())]).float()
        d["t"] = (150.0 * f32(temp_t) * lin[torch.from_numpy(synth.permutation(seed + 8, E).copy())]).float()
        lg = d["wp"].double() @ d["z"].double()
        want = torch.tensor([-50.0, 50.0, 10.0, -20.0], dtype=torch.float64)[:Cc]
        d["wp"] = (d["wp"].double() * (want / lg)[:, None]).float()
    return d


def _head_run(inp, E, Cc, label, aux, bias, temp_t, main=MAIN, aux_alpha=AUX, inv=INV, accumulate=0, grads=True, g_logits_in=None,
              g_cl_in=None):
    """One launch on guarded buffers; returns the outputs on the CPU."""
    z, wp = Buf(inp["z"]), Buf(inp["wp"])
    t = Buf(inp["t"]) if aux else None
    bp = Buf(inp["bp"]) if bias else None
    lab = None if label is None else torch.tensor([label], dtype=torch.int64, device=DEV)
    logits, losses, g_z = Buf.nans(Cc), Buf.nans(3), Buf.nans(E)
    d_wp = (Buf(inp["dwp0"]) if accumulate else Buf.nans(Cc * E)) if grads else None
    d_bp = (Buf(inp["dbp0"]) if accumulate else Buf.nans(Cc)) if grads else None
    gl = None if g_logits_in is None else Buf(g_logits_in)
    gc = None if g_cl_in is None else Buf(torch.tensor([g_cl_in], dtype=torch.float32))
    _head_call(z, t, wp, bp, lab, E, Cc, temp_t, main, aux_alpha, inv, logits, losses, g_z, d_wp, d_bp, accumulate, gl, gc)
    bufs = [b for b in (z, t, wp, bp, logits, losses, g_z, d_wp, d_bp, gl, gc) if b is not None]
    out = dict(logits=logits.cpu(), losses=losses.cpu(), g_z=g_z.cpu())
    if grads:
        out.update(d_wp=d_wp.cpu().view(Cc, E), d_bp=d_bp.cpu())
    assert all(b.guards_intact() for b in bufs), "a guard element was written"
    for b, name in ((z, "z"), (wp, "wp"), (t, "t"), (bp, "bp")):
        assert b is None or _same_bits(b.cpu(), inp[name]), name + " was modified"
    return out


def _head_ref(inp, label, aux, bias, temp_t, main=MAIN, aux_alpha=AUX, inv=INV, g_logits_in=None, g_cl_in=None):
    """fp64 autograd of (main CE(wp z + bp) + aux soft_target_ce(z, t, temp_t)) inv_accum; label None: the vector-Jacobian product with the
    upstream g_logits_in (as given) and g_cl_in (or aux) times inv_accum."""
    main, aux_alpha, inv, T = f32(main), f32(aux_alpha), f32(inv), f32(temp_t)
    z = inp["z"].double().requires_grad_()
    wp = inp["wp"].double().requires_grad_()
    bp = (inp["bp"].double() if bias else torch.zeros(wp.shape[0], dtype=torch.float64)).requires_grad_()   # (bp = NULL: d_bp is that of a zero bias)
    logits = wp @ z + bp
    zero = torch.zeros((), dtype=torch.float64)
    cl = O.soft_target_ce(z, inp["t"].double(), T) if aux else zero
    if label is not None:
        ce = O.cross_entropy(logits, label)
        total = (main * ce + aux_alpha * cl) * inv
        losses = [main * ce + aux_alpha * cl, ce, cl]
    else:
        a = f32(g_cl_in) if g_cl_in is not None else aux_alpha
        total = a * inv * cl + (0.0 * logits).sum()
        if g_logits_in is not None:
            total = total + (g_logits_in.double() * logits).sum()
        losses = [a * cl, zero, cl]
    total.backward()
    g = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    return dict(logits=logits.detach(), losses=torch.stack([torch.as_tensor(l, dtype=torch.float64).detach() for l in losses]), g_z=g(z),
                d_wp=g(wp), d_bp=g(bp))


def _head_check(label, out, ref, peaked=False):
    """peaked: atol x max(1, max|ref|) per tensor (see the module docstring)."""
    for name, tol in (("logits", LOGIT_TOL), ("losses", LOSS_TOL), ("g_z", GRAD_TOL), ("d_wp", GRAD_TOL), ("d_bp", GRAD_TOL)):
        if name not in out:
            continue
        s = max(1.0, float(ref[name].abs().max())) if peaked else 1.0
        _close("%s %s" % (label, name), out[name], ref[name], tol[0] * s, tol[1])


@pytest.mark.parametrize("shape", ALL_HEAD_SHAPES, ids=_sid)
def test_head_matches_fp64(shape):
    """Label 0 and C - 1, aux term on / off, bias given / NULL, temp_t 0.1 / 1.0: logits, the three losses, g_z, d_wp, d_bp."""
    E, Cc = shape
    inp = _head_inputs(E, Cc)
    for label in sorted({0, Cc - 1}):
        for aux in (True, False):
            for bias in (True, False):
                for temp_t in (0.1, 1.0):
                    out = _head_run(inp, E, Cc, label, aux, bias, temp_t)
                    ref = _head_ref(inp, label, aux, bias, temp_t)
                    _head_check("A %d-%d y%d %s %s T%g" % (E, Cc, label, "aux" if aux else "noaux", "bias" if bias else "nobias", temp_t),
                                out, ref)


@pytest.mark.parametrize("shape", ONE_PER_KERNEL, ids=_sid)
def test_head_accumulate_and_null_gradients(shape):
    """accumulate = 1 into non-zero d_wp / d_bp is base + (the accumulate = 0 result): one fp32 addition per element, bit for bit, in all
    three kernels.  d_wp = d_bp = NULL leaves logits, losses and g_z bit-identical."""
    E, Cc = shape
    inp = _head_inputs(E, Cc)
    label = Cc - 1
    r0 = _head_run(inp, E, Cc, label, True, True, 0.1)
    r1 = _head_run(inp, E, Cc, label, True, True, 0.1, accumulate=1)
    r2 = _head_run(inp, E, Cc, label, True, True, 0.1, grads=False)
    assert _same_bits(r1["d_wp"], inp["dwp0"] + r0["d_wp"]) and _same_bits(r1["d_bp"], inp["dbp0"] + r0["d_bp"])
    for name in ("logits", "losses", "g_z"):
        assert _same_bits(r1[name], r0[name]) and _same_bits(r2[name], r0[name]), name
    _head_check("A %d-%d accumulate base" % shape, r0, _head_ref(inp, label, True, True, 0.1))


@pytest.mark.parametrize("shape", ONE_PER_KERNEL, ids=_sid)
def test_head_autograd_form(shape):
    """label = NULL.  With g_logits_in / g_cl_in: the gradients are the fp64 vector-Jacobian product with those upstream values;
    losses = {g_cl_in cl, 0, cl} (include/mhimx.h).  Without either: the logit path contributes nothing (d_wp = d_bp = 0 exactly), the
    distillation term is scaled by aux_alpha inv_accum and losses = {aux_alpha cl, 0, cl}."""
    E, Cc = shape
    inp = _head_inputs(E, Cc)
    for aux in (True, False):
        out = _head_run(inp, E, Cc, None, aux, True, 0.1, g_logits_in=inp["gl"], g_cl_in=0.37)
        ref = _head_ref(inp, None, aux, True, 0.1, g_logits_in=inp["gl"], g_cl_in=0.37)
        _head_check("A %d-%d autograd %s" % (E, Cc, "aux" if aux else "noaux"), out, ref)
        assert float(out["losses"][1]) == 0.0
        out = _head_run(inp, E, Cc, None, aux, True, 0.1)
        ref = _head_ref(inp, None, aux, True, 0.1)
        _head_check("A %d-%d autograd no upstream %s" % (E, Cc, "aux" if aux else "noaux"), out, ref)
        assert float(out["losses"][1]) == 0.0 and float(out["d_wp"].abs().max()) == 0.0 and float(out["d_bp"].abs().max()) == 0.0
        if not aux:
            assert float(out["g_z"].abs().max()) == 0.0 and float(out["losses"].abs().max()) == 0.0


@pytest.mark.parametrize("shape", PEAKED_SHAPES, ids=_sid)
def test_head_peaked(shape):
    """z over +-80, logits about +-50, t / temp_t over +-150: finite, and inside the same relative bounds - the max-subtraction carries it."""
    E, Cc = shape
    inp = _head_inputs(E, Cc, peaked=True, temp_t=0.1)
    assert float(inp["z"].abs().max()) == 80.0 and abs(float((inp["t"].double() / f32(0.1)).abs().max()) - 150.0) < 1e-3
    for label in (0, Cc - 1):
        out = _head_run(inp, E, Cc, label, True, True, 0.1)
        ref = _head_ref(inp, label, True, True, 0.1)
        assert 40.0 < float(ref["logits"].abs().max()) < 60.0 and int(ref["logits"].argmax()) == 1
        _head_check("A %d-%d peaked y%d" % (E, Cc, label), out, ref, peaked=True)


# ================================================================================================================== B. DSMIL head
DSMIL_SHAPES = [(1, 1), (2, 512), (3, 100), (3, 257), (16, 256), (16, 1000)]


def _dsmil_call(lb, li, label, Bs, Bt, Cc, V, temp_t, main, aux, inv, losses, g_lb, g_li, g_B, g_cl_in):
    from mhim_mil_amd import _lib as L, ops
    q = lambda x: None if x is None else _p(x)
    L.check(L.lib().mhimx_dsmil_head(ops._stream(), q(lb), q(li), q(label), q(Bs), q(Bt), Cc, V, float(temp_t), float(main), float(aux),
                                     float(inv), q(losses), q(g_lb), q(g_li), q(g_B), q(g_cl_in)), "mhimx_dsmil_head")


@functools.lru_cache(maxsize=None)
def _dsmil_inputs(Cc, V):
    g = torch.Generator().manual_seed(500 + 31 * Cc + V)
    return dict(lb=torch.randn(Cc, generator=g), li=torch.randn(Cc, generator=g), Bs=torch.randn(Cc, V, generator=g),
                Bt=torch.randn(Cc, V, generator=g) * 0.3)


def _dsmil_run(inp, Cc, V, label, with_bt, temp_t, main, aux, inv, want_gB=True, g_cl_in=None):
    lb, li = (Buf(inp["lb"]), Buf(inp["li"])) if label is not None else (None, None)
    lab = None if label is None else torch.tensor([label], dtype=torch.int64, device=DEV)
    Bs = Buf(inp["Bs"])
    Bt = Buf(inp["Bt"]) if with_bt else None
    losses = Buf.nans(3)
    g_lb, g_li = (Buf.nans(Cc), Buf.nans(Cc)) if label is not None else (None, None)
    g_B = Buf.nans(Cc * V) if want_gB else None
    gc = None if g_cl_in is None else Buf(torch.tensor([g_cl_in], dtype=torch.float32))
    _dsmil_call(lb, li, lab, Bs, Bt, Cc, V, temp_t, main, aux, inv, losses, g_lb, g_li, g_B, gc)
    out = dict(losses=losses.cpu())
    for name, b in (("g_lb", g_lb), ("g_li", g_li), ("g_B", g_B)):
        if b is not None:
            out[name] = b.cpu()
    assert all(b.guards_intact() for b in (lb, li, Bs, Bt, losses, g_lb, g_li, g_B, gc) if b is not None), "a guard element was written"
    return out


def _dsmil_ref(inp, label, with_bt, temp_t, main, aux, inv):
    main, aux, inv, T = f32(main), f32(aux), f32(inv), f32(temp_t)
    lb, li, Bs = (inp[k].double().requires_grad_() for k in ("lb", "li", "Bs"))
    zero = torch.zeros((), dtype=torch.float64)
    ce = O.cross_entropy(0.5 * (lb + li), label) if label is not None else zero
    cl = O.soft_target_ce(Bs, inp["Bt"].double(), T).mean() if with_bt else zero
    total = (main * ce + aux * cl) * inv + 0.0 * (lb.sum() + li.sum() + Bs.sum())
    total.backward()
    return dict(losses=torch.stack([(main * ce + aux * cl).detach(), ce.detach(), cl.detach()]), g_lb=lb.grad, g_li=li.grad, g_B=Bs.grad)


def _dsmil_check(label, out, ref):
    _close(label + " losses", out["losses"], ref["losses"], 0.0, 2e-5)
    for name, rel in (("g_lb", 1e-5), ("g_li", 1e-5), ("g_B", 1e-4)):
        if name in out:
            _close("%s %s" % (label, name), out[name], ref[name], rel * float(ref[name].abs().max()))


@pytest.mark.parametrize("shape", DSMIL_SHAPES, ids=_sid)
def test_dsmil_head_matches_fp64(shape):
    """Label 0 and C - 1; Bt given, and Bt = NULL for which g_B is all zeros and cl = 0; temp_t 0.1 and 1.0."""
    Cc, V = shape
    inp = _dsmil_inputs(Cc, V)
    for label in sorted({0, Cc - 1}):
        for with_bt in (True, False):
            for temp_t in (0.1, 1.0):
                out = _dsmil_run(inp, Cc, V, label, with_bt, temp_t, MAIN, AUX, INV)
                ref = _dsmil_ref(inp, label, with_bt, temp_t, MAIN, AUX, INV)
                _dsmil_check("B %d-%d y%d %s T%g" % (Cc, V, label, "Bt" if with_bt else "noBt", temp_t), out, ref)
                assert _same_bits(out["g_lb"], out["g_li"])
                if not with_bt:
                    assert float(out["g_B"].abs().max()) == 0.0 and float(out["losses"][2]) == 0.0


@pytest.mark.parametrize("shape", DSMIL_SHAPES, ids=_sid)
def test_dsmil_head_label_free_forms(shape):
    """The two forms of dsmil.py's SoftTargetCE (main_alpha 0, aux_alpha 1, inv_accum 1): losses only, then g_B with the upstream g_cl_in."""
    Cc, V = shape
    inp = _dsmil_inputs(Cc, V)
    for temp_t in (0.1, 1.0):
        out = _dsmil_run(inp, Cc, V, None, True, temp_t, 0.0, 1.0, 1.0, want_gB=False)
        ref = _dsmil_ref(inp, None, True, temp_t, 0.0, 1.0, 1.0)
        _dsmil_check("B %d-%d forward T%g" % (Cc, V, temp_t), out, ref)
        assert float(out["losses"][1]) == 0.0
        out = _dsmil_run(inp, Cc, V, None, True, temp_t, 0.0, 1.0, 1.0, g_cl_in=3.0)
        ref = _dsmil_ref(inp, None, True, temp_t, 0.0, 3.0, 1.0)
        _dsmil_check("B %d-%d backward T%g" % (Cc, V, temp_t), out, ref)
    out = _dsmil_run(inp, Cc, V, None, False, 0.1, 0.0, 1.0, 1.0, g_cl_in=3.0)
    assert float(out["g_B"].abs().max()) == 0.0 and float(out["losses"].abs().max()) == 0.0


# ================================================================================================================== C. the update
HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5, grad_scale=1.0, ema_mm=0.9997)


def _optim_call(**kw):
    from mhim_mil_amd import ops
    return ops.optim_step(**kw)


def _flush_call(lst):
    from mhim_mil_amd import ops
    ops.reduce_flush(lst)


def _job_k(kind, G):
    """Rounded fp32 additions on the longest chain of one reduction job, the accumulate included (module docstring)."""
    return G if kind == 0 else max(G // 4 + G % 4 - 1, 0) + 3


def _spec(n_train, n_all, **kw):
    s = dict(n_train=n_train, n_all=n_all, seed=7, gstd=1e-3, step=3, step_dev=None, lr_table=None, mm_table=None, zero_grad=True, teacher=True,
             unaligned=(), n_extra=0, pitch=0, extra_lo=0, extra_only=False, clip=None, jobs=(), g_tail=(), hyper=dict(HYPER))
    hyper = {k: kw.pop(k) for k in list(kw) if k in HYPER}
    s.update(kw)
    s["hyper"].update(hyper)
    return s


def _inputs(s):
    """fp32 inputs on the CPU.  NaN where the contract says nothing is read."""
    n, N, gstd = s["n_train"], s["n_all"], s["gstd"]
    gen = torch.Generator().manual_seed(s["seed"] + 13 * N)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    inp = dict(p=0.1 * r(N), m=gstd * r(N), v=(gstd * r(N)) ** 2, t=0.1 * r(N), g=gstd * r(N))
    inp["g"][n:] = NAN
    if s["g_tail"]:
        inp["g"][n:n + len(s["g_tail"])] = torch.tensor(s["g_tail"])
    if s["extra_only"]:
        inp["g"][s["extra_lo"]:n] = NAN
    if s["n_extra"]:
        inp["slabs"] = gstd * r(s["n_extra"], s["pitch"])
        inp["slabs"][:, n:] = NAN
        inp["slabs"][:, :s["extra_lo"]] = NAN
    inp["other"] = gstd * r(64)
    inp["parts"] = []
    for (kind, where, off, cnt, G, acc) in s["jobs"]:
        ld = cnt if kind == 1 else cnt + 8
        inp["parts"].append(gstd * r(G, ld))
        if where == "g" and not acc:
            inp["g"][off:off + cnt] = NAN
    return inp


def _run_update(s, inp, fold=False, flush_first=False):
    """One mhimx_optim_step on guarded device copies of ``inp``; the reduction jobs of s['jobs'] go on a list that is either folded
    (fold = True), or flushed by mhimx_reduce_flush before an update without the list (flush_first = True)."""
    from mhim_mil_amd import _lib as L, ops
    n, N, h = s["n_train"], s["n_all"], s["hyper"]
    off = lambda name: PAD + 1 if name in s["unaligned"] else PAD
    b = {k: Buf(inp[k], off(k)) for k in ("p", "g", "m", "v", "t")}
    other = Buf(inp["other"])
    slabs = None
    if s["n_extra"]:
        slabs_store = torch.full((PAD + inp["slabs"].numel() + PAD,), NAN, device=DEV)
        slabs = slabs_store[PAD:PAD + inp["slabs"].numel()].view(s["n_extra"], s["pitch"])
        slabs.copy_(inp["slabs"])
    ws = Buf.nans(1024) if s["clip"] else None
    dev = lambda x, dt: None if x is None else torch.tensor(x, dtype=dt, device=DEV)
    lst = None
    if s["jobs"]:
        lst = ops.ReduceList()
        parts = [x.to(DEV) for x in inp["parts"]]
        for (kind, where, o, cnt, G, acc), pt in zip(s["jobs"], parts):
            out = (b["g"].t if where == "g" else other.t)[o:o + cnt]
            if kind == 1:
                ops.reduce_slabs_job(lst, pt, out, accumulate=acc)
            else:
                lst.c.j[lst.c.n] = L.ReduceJob(kind=0, accumulate=int(acc), parts=ops._p(pt), out=ops._p(out), G=G, W=cnt, ld=pt.shape[1], K1=0,
                                               K2=0, ldo=0)
                lst.c.n += 1
                lst.keep.append(pt)
        if flush_first:
            _flush_call(lst)
            assert lst.c.n == 0
    _optim_call(p=b["p"].t, g=b["g"].t, m=b["m"].t, v=b["v"].t, teacher=b["t"].t if s["teacher"] else None, n_train=n, step=s["step"],
                step_dev=dev(None if s["step_dev"] is None else [s["step_dev"]], torch.int64), lr_table=dev(s["lr_table"], torch.float32),
                mm_table=dev(s["mm_table"], torch.float32), zero_grad=s["zero_grad"], g_extra=slabs, clip_norm=s["clip"],
                ws=None if ws is None else ws.t, fold=lst if fold else None, extra_lo=s["extra_lo"], extra_only=s["extra_only"], **h)
    if lst is not None:
        assert lst.c.n == 0 and not lst.keep, "the list is empty after the call"
    out = {k: b[k].cpu() for k in b}
    out["other"] = other.cpu()
    assert all(x.guards_intact() for x in list(b.values()) + [other] + ([ws] if ws else [])), "a guard element was written"
    if slabs is not None:
        assert _same_bits(slabs_store[PAD:-PAD].cpu(), inp["slabs"].reshape(-1)) and bool(torch.isnan(slabs_store[:PAD]).all()) \
            and bool(torch.isnan(slabs_store[-PAD:]).all())
    return out


def _summed_gradient(s, inp):
    """fp64 sum of everything that makes up the gradient on [0, n_train), in the kernel's order of terms; A = the sum of magnitudes;
    k = rounded fp32 additions on the longest chain into each element."""
    n = s["n_train"]
    g = inp["g"][:n].double()
    read = ~torch.isnan(g)
    gs = torch.where(read, g, torch.zeros_like(g))
    A = gs.abs()
    k = torch.zeros(n, dtype=torch.float64)
    for (kind, where, off, cnt, G, acc), pt in zip(s["jobs"], inp["parts"]):
        if where != "g" or off >= n:
            continue
        hi = min(off + cnt, n)
        gs[off:hi] += pt.double()[:, :hi - off].sum(0)
        A[off:hi] += pt.double()[:, :hi - off].abs().sum(0)
        k[off:hi] += _job_k(kind, G)
    lo = s["extra_lo"]
    for z in range(s["n_extra"]):
        gs[lo:] += inp["slabs"][z, lo:n].double()
        A[lo:] += inp["slabs"][z, lo:n].double().abs()
        k[lo:] += 1
    assert torch.isfinite(gs).all()
    return gs, A, k


def _norm64(s, inp):
    gs, _, _ = _summed_gradient(s, inp)
    return float(torch.sqrt(((gs * f32(s["hyper"]["grad_scale"])) ** 2).sum()))


def _check_update(label, s, inp, out):
    """Moments against fp64, p from the kernel's own moments, the teacher from the kernel's own p; bits of everything behind n_train."""
    n, N = s["n_train"], s["n_all"]
    h = {k: f32(v) for k, v in s["hyper"].items()}
    b1, b2, eps, wd, gsc, lr, mm = (h[k] for k in ("beta1", "beta2", "eps", "weight_decay", "grad_scale", "lr", "ema_mm"))
    t = s["step_dev"] if s["step_dev"] is not None else s["step"]
    if s["lr_table"]:
        lr = f32(s["lr_table"][min(t - 1, len(s["lr_table"]) - 1)])
    if s["mm_table"]:
        mm = f32(s["mm_table"][min(t - 1, len(s["mm_table"]) - 1)])
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p0, m0, v0, t0 = (inp[k].double() for k in ("p", "m", "v", "t"))
    gs, A, k = _summed_gradient(s, inp)
    coef = 1.0
    if s["clip"] and n > 0:
        vv = gs * gsc
        SS = float((vv ** 2).sum())
        coef = min(1.0, f32(s["clip"]) / (math.sqrt(SS) + f32(1e-6)))
        if coef < 1.0:
            k = k + 14.0
    gi = gs * (gsc * coef) + wd * p0[:n]
    S = A * abs(gsc * coef) + wd * p0[:n].abs()
    m64 = b1 * m0[:n] + (1.0 - b1) * gi
    v64 = b2 * v0[:n] + (1.0 - b2) * gi * gi
    m, v, p, tea = (out[x].double() for x in ("m", "v", "p", "t"))
    em, ev = (m[:n] - m64).abs(), (v[:n] - v64).abs()
    bm, bv = U * (b1 * m0[:n].abs() + (1.0 - b1) * S), U * (b2 * v0[:n] + (1.0 - b2) * S * S)
    rm, rv = _ratio(em, (6.0 + k) * bm), _ratio(ev, (10.0 + 2.0 * k) * bv)
    _note(label + " m", rm)
    _note(label + " v", rv)
    D = (lr / bc1) * m[:n] / (v[:n].sqrt() / math.sqrt(bc2) + eps)
    pref = p0[:n] - D
    rp = _ratio((p[:n] - pref).abs(), U * pref.abs() + 8.0 * U * D.abs())
    _note(label + " p", rp)
    rt = 0.0
    if s["teacher"]:
        t64 = mm * t0 + (1.0 - mm) * p
        rt = _ratio((tea - t64).abs(), 3.0 * U * (mm * t0.abs() + (1.0 - mm) * p.abs()))
        _note(label + " teacher", rt)
    else:
        assert _same_bits(out["t"], inp["t"]), label + ": teacher = NULL, yet the buffer changed"
    assert rm <= 1.0 and rv <= 1.0 and rp <= 1.0 and rt <= 1.0, "%s: m %.4g v %.4g p %.4g teacher %.4g of their bounds" % (label, rm, rv, rp, rt)
    for name in ("p", "m", "v"):
        assert _same_bits(out[name][n:], inp[name][n:]), "%s: %s behind n_train changed" % (label, name)
    if not s["jobs"]:
        if s["zero_grad"]:
            assert _same_bits(out["g"][:n], torch.zeros(n)), label + ": zero_grad left something"
            assert _same_bits(out["g"][n:], inp["g"][n:])
        else:
            assert _same_bits(out["g"], inp["g"]), label + ": g changed without zero_grad"
        assert _same_bits(out["other"], inp["other"])


PLAIN_SIZES = [(1, 1), (3, 3), (4, 4), (5, 8), (4098, 4103), (1023, 1030), (0, 64), (5000, 5100), (2098179, 2098183)]


@pytest.mark.parametrize("size", PLAIN_SIZES, ids=_sid)
def test_update_plain(size):
    """Random m0, v0 >= 0, p ~ 0.1 randn; zero_grad on / off; with a teacher and without."""
    n, N = size
    for zero_grad in (True, False):
        for teacher in (True, False):
            s = _spec(n, N, zero_grad=zero_grad, teacher=teacher)
            inp = _inputs(s)
            _check_update("C1 %d-%d %s %s" % (n, N, "zero" if zero_grad else "keep", "teacher" if teacher else "noteacher"), s, inp,
                          _run_update(s, inp))


TERMS = {"weight_decay": dict(weight_decay=0.05, gstd=1e-3), "eps": dict(eps=1e-3, gstd=1e-4, step=1000), "grad_scale": dict(grad_scale=0.125),
         "betas": dict(beta1=0.8, beta2=0.99), "step1": dict(step=1), "step2": dict(step=2), "step1000": dict(step=1000),
         "step100000": dict(step=100000), "all": dict(weight_decay=0.05, eps=1e-3, grad_scale=0.125, beta1=0.8, beta2=0.99, step=2)}


@pytest.mark.parametrize("term", sorted(TERMS))
def test_update_terms(term):
    """Each term of the update made large enough that dropping or misplacing it breaks a bound: weight decay comparable to the gradient,
    eps dominating the denominator, a gradient scale, other betas, and steps whose bias corrections differ by orders of magnitude."""
    s = _spec(5000, 5100, **TERMS[term])
    inp = _inputs(s)
    if term == "eps":
        h = s["hyper"]
        assert f32(h["eps"]) > 3 * float(inp["v"].sqrt().median()) / math.sqrt(1 - f32(h["beta2"]) ** s["step"])
    _check_update("C2 " + term, s, inp, _run_update(s, inp))


def test_update_unaligned():
    """p, g, m, v and the teacher one float into their storage: the whole update takes the scalar path, inside the same bounds."""
    for size in ((5000, 5100), (4098, 4103)):
        s = _spec(*size, unaligned=("p", "g", "m", "v", "t"), weight_decay=0.05)
        inp = _inputs(s)
        out = _run_update(s, inp)
        _check_update("C3 unaligned %d-%d" % size, s, inp, out)
        al = _run_update(dict(s, unaligned=()), inp)
        _note("C3 unaligned %d-%d: tensors (of p, m, v, teacher) whose bits equal the aligned run" % size,
              sum(_same_bits(out[k], al[k]) for k in ("p", "m", "v", "t")))
    for name in ("p", "g", "m", "v", "t"):                                   # one unaligned buffer is enough to leave the vector path
        s = _spec(1023, 1030, unaligned=(name,))
        inp = _inputs(s)
        _check_update("C3 unaligned %s alone" % name, s, inp, _run_update(s, inp))


def test_update_device_step():
    """step_dev holds 7 while the host step says 1: the bias corrections are those of t = 7.  step_dev holds 1: the host-step-1 result."""
    s = _spec(5000, 5100, step=1, step_dev=7)
    inp = _inputs(s)
    _check_update("C4 step_dev 7 host 1", s, inp, _run_update(s, inp))
    s = _spec(5000, 5100, step=0, step_dev=7)
    _check_update("C4 step_dev 7 host 0", s, inp, _run_update(s, inp))
    s = _spec(5000, 5100, step=1, step_dev=1)
    _check_update("C4 step_dev 1 host 1", s, inp, _run_update(s, inp))
    s = _spec(5000, 5100, step=1)
    _check_update("C4 host 1", s, inp, _run_update(s, inp))


LR_TABLE = [1e-3, 8e-4, 6e-4, 4e-4, 2e-4]
MM_TABLE = [0.99, 0.992, 0.994, 0.996, 0.9997]


@pytest.mark.parametrize("table", ["lr", "mm", "both"])
def test_update_schedules(table):
    """Tables of five entries at t = 1, 3, 5, 6 and 50 (the last entry is held), the step on the host and on the device (where the host's
    says something else)."""
    kw = dict(lr_table=LR_TABLE if table != "mm" else None, mm_table=MM_TABLE if table != "lr" else None)
    for t in (1, 3, 5, 6, 50):
        for on_dev in (False, True):
            s = _spec(1023, 1030, step=(t + 1 if on_dev else t), step_dev=(t if on_dev else None), lr=7e-3, ema_mm=0.5, **kw)
            inp = _inputs(s)
            _check_update("C4 %s table t%d %s" % (table, t, "dev" if on_dev else "host"), s, inp, _run_update(s, inp))


# (extra_lo, extra_only, zero_grad, unaligned)
SLAB_CASES = [(0, False, True, False), (1024, False, True, False), (1024, True, True, False), (1024, True, False, False), (0, True, True, False),
              (1024, True, True, True), (0, False, False, True)]


@pytest.mark.parametrize("n_extra", [1, 3, 8])
@pytest.mark.parametrize("case", SLAB_CASES, ids=lambda c: "lo%d-%s-%s-%s" % (c[0], "only" if c[1] else "sum", "zero" if c[2] else "keep",
                                                                                 "unaligned" if c[3] else "aligned"))
def test_update_slabs(case, n_extra):
    """n_train = 4098 (the quad that straddles it adds its slabs on the scalar path), pitch 4104 with NaN padding, NaN below extra_lo, NaN in
    g from extra_lo on under extra_only.  Reference: the fp64 sum in slab order."""
    lo, only, zg, ua = case
    s = _spec(4098, 4103, n_extra=n_extra, pitch=4104, extra_lo=lo, extra_only=only, zero_grad=zg, unaligned=("p", "g", "m", "v", "t") if ua else ())
    inp = _inputs(s)
    _check_update("C5 S%d lo%d %s %s %s" % (n_extra, lo, "only" if only else "sum", "zero" if zg else "keep", "unaligned" if ua else "aligned"),
                  s, inp, _run_update(s, inp))


CLIP_COMBOS = {"plain": dict(), "scale": dict(grad_scale=0.125), "decay": dict(weight_decay=0.05),
               "slabs": dict(grad_scale=0.125, n_extra=3, extra_lo=1024, extra_only=True, weight_decay=0.05)}


@pytest.mark.parametrize("combo", sorted(CLIP_COMBOS))
@pytest.mark.parametrize("n_train", [1, 1000, 1048581])
def test_update_clipping(n_train, combo):
    """Norm above clip_norm (coefficient 0.5) and below it (coefficient exactly 1: the bits of the same call without clipping).  The norm is
    of the scaled, summed gradient over [0, n_train); the decay is added after clipping.  ws is NaN before the call."""
    kw = dict(CLIP_COMBOS[combo])
    if kw.get("n_extra"):
        kw["pitch"] = (n_train + 5 + 3) // 4 * 4
        if n_train <= 1024:
            kw.update(extra_lo=0, extra_only=n_train == 1000)
    s = _spec(n_train, n_train + 5, **kw)
    inp = _inputs(s)
    norm = _norm64(s, inp)
    assert norm > 1e-6
    above = dict(s, clip=0.5 * norm)
    _check_update("C6 n%d %s above" % (n_train, combo), above, inp, _run_update(above, inp))
    below = dict(s, clip=2.0 * norm)
    out = _run_update(below, inp)
    _check_update("C6 n%d %s below" % (n_train, combo), below, inp, out)
    plain = _run_update(s, inp)
    for name in ("p", "m", "v", "t", "g"):
        assert _same_bits(out[name], plain[name]), "coefficient 1: %s differs from the call without clipping" % name


# ------------------------------------------------------------------------------------------------------------------ folded reductions
def _fold_case(label, s):
    """Folded == flushed + plain update, bit for bit, on identical copies; and the folded result inside the oracle bounds."""
    assert s["zero_grad"]
    inp = _inputs(s)
    folded = _run_update(s, inp, fold=True)
    flushed = _run_update(s, inp, flush_first=True)
    for name in ("p", "m", "v", "t", "g", "other"):
        assert _same_bits(folded[name], flushed[name]), "%s: %s differs from reduce_flush + update" % (label, name)
    _check_update(label, s, inp, folded)
    n = s["n_train"]
    assert _same_bits(folded["g"][:n], torch.zeros(n))
    # what the flushed jobs left outside [0, n_train): the fp64 sums
    for (kind, where, off, cnt, G, acc), pt in zip(s["jobs"], inp["parts"]):
        base = inp["other"] if where == "other" else inp["g"]
        lo = off if where == "other" else max(off, n)
        if lo >= off + cnt:
            continue
        ref = pt.double()[:, lo - off:cnt].sum(0) + (base[lo:off + cnt].double() if acc else 0.0)
        mag = pt.double()[:, lo - off:cnt].abs().sum(0) + (base[lo:off + cnt].double().abs() if acc else 0.0)
        got = folded["other" if where == "other" else "g"][lo:off + cnt].double()
        r = _ratio((got - ref).abs(), _job_k(kind, G) * U * mag)
        _note("%s job outside [0, n_train) G%d" % (label, G), r)
        assert r <= 1.0


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("G", [1, 3, 4, 8, 13, 64])
def test_update_fold_one_job(G, accumulate):
    _fold_case("C7 one job G%d acc%d" % (G, accumulate), _spec(5000, 5100, jobs=((1, "g", 1000, 512, G, accumulate),)))


FOUR_JOBS = ((1, "g", 0, 256, 3, 0), (1, "g", 512, 1024, 8, 1), (1, "g", 2000, 4, 13, 0), (1, "g", 4000, 996, 64, 1))


def test_update_fold_four_jobs():
    _fold_case("C7 four jobs", _spec(5000, 5100, jobs=FOUR_JOBS))
    _fold_case("C7 four jobs, decay, no teacher", _spec(5000, 5100, jobs=FOUR_JOBS, weight_decay=0.05, teacher=False))


def test_update_fold_six_eligible_jobs():
    """Four are folded, two are flushed."""
    jobs = FOUR_JOBS + ((1, "g", 1600, 128, 1, 1), (1, "g", 3000, 512, 4, 0))
    _fold_case("C7 six jobs", _spec(5000, 5100, jobs=jobs))


def test_update_fold_mixed_list():
    """Eligible jobs among one of each ineligible kind: n % 4 != 0, off % 4 != 0, G = 65, an output reaching past n_train / 4 * 4 (and past
    n_train: its last two elements land in g behind the trained range), an output outside g, and a kind-0 job."""
    jobs = ((1, "g", 0, 64, 8, 1), (1, "g", 100, 6, 3, 0), (1, "g", 202, 8, 4, 1), (1, "g", 300, 16, 65, 0), (1, "g", 1000, 128, 1, 0),
            (1, "g", 4092, 8, 13, 1), (1, "other", 16, 16, 4, 1), (0, "g", 400, 40, 5, 1), (1, "g", 2000, 1024, 64, 1))
    # (the job that reaches past n_train accumulates: the two elements of g behind n_train that it reads hold numbers)
    _fold_case("C7 mixed list", _spec(4098, 4103, jobs=jobs, g_tail=(3e-4, -7e-4)))


def test_update_fold_unaligned_p():
    """p one float into its storage: nothing is folded, the whole list is flushed, the update takes the scalar path."""
    _fold_case("C7 unaligned p", _spec(5000, 5100, jobs=FOUR_JOBS, unaligned=("p",)))


def test_update_fold_with_clipping():
    """clip_norm: the norm needs the final gradient, so the whole list is flushed."""
    s = _spec(5000, 5100, jobs=FOUR_JOBS)
    s["clip"] = 0.5 * _norm64(s, _inputs(s))
    _fold_case("C7 clipping", s)
