"""Nystrom / TransMIL encoder over the HIP primitives.

Mirrors the reference's ``SAttention`` (mhim_modules/baseline.py:222-288), ``TransLayer`` (:196-220),
``NystromAttention`` (nystrom_attention.py:30-152) and ``PPEG`` (emb_position.py:85-120): same parameter
names/shapes, same math incl. the quirks (front zero-padding whose pad tokens stay unmasked keys, global-max
pseudo-inverse scaling, dim_head = 64, 256 landmarks).

Every arithmetic step is a kernel of libmhimx.so.  The encoder is *composed* from primitives — GEMMs (nt / nn / tn),
row softmax, landmark means, a*I+b*X, pseudo-inverse init, depth-wise residual conv, PPEG stencil, LayerNorm — each
wrapped in a ``torch.autograd.Function`` whose backward is again kernels, so torch contributes only the graph
bookkeeping, views and copies (cat / slice / zero-fill).  q, k, v stay packed in the [n_pad, 1536] to_qkv output; a
per-head matrix is (pointer offset, row pitch), never a permuted copy.
"""
from __future__ import annotations

import os
import ctypes as C
import math

import torch
from torch import nn

from . import _lib as L
from . import ops

HEADS, DH, INNER, LANDMARKS, PINV_ITERS, CONV_K = 8, 64, 512, 256, 6, 33


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


_PREC = "bf16x3"


def set_precision(p):
    global _PREC
    _PREC = p


# --------------------------------------------------------------------------------------------------- raw GEMMs
def _gemm(mode, a, a_off, lda, b, b_off, ldb, c, c_off, ldc, M, N, K, accumulate=False, alpha=1.0, bias=None):
    """One strided GEMM on raw (tensor, element offset, row pitch) operands.
    nt: C[M,N] = A[M,K] B[N,K]^T ; nn: C[M,N] = A[M,K] B[K,N] ; tn: C[M,N] = A[K,M]^T B[K,N]."""
    lib = L.lib()
    prec = L.PREC[_PREC]
    if mode == "tn":
        splits = 1
        ws = None
        if K >= 4096:
            splits = min(32, max(1, K // 2048))
            ws = torch.empty(splits * M * N, device=c.device)
        g = L.GemmTN(A=_ptr(a, a_off), lda=lda, B=_ptr(b, b_off), ldb=ldb, rows=None, C=_ptr(c, c_off), ldc=ldc, M=K, K1=M, K2=N,
                     splits=splits, ws=None if ws is None else _ptr(ws), accumulate=int(accumulate), prec=prec,
                     ws_floats=0 if ws is None else ws.numel())
        L.check(lib.mhimx_gemm_tn(_st(), C.byref(g)), "mhimx_gemm_tn")
        return
    g = L.GemmNT(A=_ptr(a, a_off), lda=lda, rows=None, B=_ptr(b, b_off), ldb=ldb, C=_ptr(c, c_off), ldc=ldc, M=M, N=N, K=K,
                 bias=None if bias is None else _ptr(bias), accumulate=int(accumulate), prec=prec)
    if mode == "nt":
        assert alpha == 1.0
        L.check(lib.mhimx_gemm_nt(_st(), C.byref(g)), "mhimx_gemm_nt")
    else:
        splits, ws = 1, None
        if K >= 4096 and M * N <= 256 * 256:
            splits = min(64, max(1, K // 1024))
            ws = torch.empty(splits * M * N, device=c.device)
        L.check(lib.mhimx_gemm_nn(_st(), C.byref(g), float(alpha), splits, None if ws is None else _ptr(ws)), "mhimx_gemm_nn")


class Op:
    """Per-head operand descriptor: head h is the (rows x cols) matrix at t.data + base + h*head_off with row pitch ld."""

    def __init__(self, t, base, head_off, ld, rows, cols):
        self.t, self.base, self.head_off, self.ld, self.rows, self.cols = t, base, head_off, ld, rows, cols

    def like(self, t):
        return Op(t, self.base, self.head_off, self.ld, self.rows, self.cols)

    def off(self, h):
        return self.base + h * self.head_off


def batched(t):
    """[B, R, Cc] contiguous batch of matrices."""
    B, R, Cc = t.shape
    return Op(t, 0, R * Cc, Cc, R, Cc)


_MODE = {"nt": 0, "nn": 1, "tn": 2}
BATCHED = True


def _heads_mm(mode, A: Op, Bo: Op, Co: Op, heads, accumulate=False):
    if mode == "nt":
        M, N, K = A.rows, Bo.rows, A.cols
    elif mode == "nn":
        M, N, K = A.rows, Bo.cols, A.cols
    else:
        M, N, K = A.cols, Bo.cols, A.rows
    aligned = K % 4 == 0 and A.ld % 4 == 0 and A.head_off % 4 == 0 and (mode != "nt" or (Bo.ld % 4 == 0 and Bo.head_off % 4 == 0))
    if not BATCHED or (mode != "tn" and not aligned):
        for h in range(heads):
            _gemm(mode, A.t, A.off(h), A.ld, Bo.t, Bo.off(h), Bo.ld, Co.t, Co.off(h), Co.ld, M, N, K, accumulate=accumulate)
        return
    # all heads in ONE launch; a long reduction (K = tokens) is split so that the launch still fills the 256 CUs
    splits, ws = 1, None
    if mode != "nt" and K >= 2048:
        tiles = heads * ((M + 127) // 128) * ((N + 127) // 128)
        splits = max(1, min((1024 + tiles - 1) // tiles, K // 256, 65535 // heads))
        if mode == "tn" and M <= 16 and heads == 1:          # thin left operand: a streaming kernel, one short row chunk per workgroup
            splits = max(1, min(512, K // 16))               # (~20 rows per thread; the slabs are summed 32 at a time per column)
        if splits > 1:
            ws = torch.empty(heads * splits * M * N, device=Co.t.device)
    g = L.GemmNT(A=_ptr(A.t, A.base), lda=A.ld, rows=None, B=_ptr(Bo.t, Bo.base), ldb=Bo.ld, C=_ptr(Co.t, Co.base), ldc=Co.ld, M=M, N=N,
                 K=K, accumulate=int(accumulate), prec=L.PREC[_PREC])
    L.check(L.lib().mhimx_gemm_batched(_st(), _MODE[mode], C.byref(g), heads, A.head_off, Bo.head_off, Co.head_off, 1.0, splits,
                                       None if ws is None else _ptr(ws)), "mhimx_gemm_batched")


class HeadsMatmul(torch.autograd.Function):
    """C_h = op(A_h, B_h) for every head, operands addressed in place inside larger tensors (no permute copies).
    Backward writes dA / dB straight into zero-filled tensors shaped like the parents."""

    @staticmethod
    def forward(ctx, a_t, b_t, mode, a_desc, b_desc, c_shape, c_desc, heads):
        A, Bo = Op(a_t, *a_desc), Op(b_t, *b_desc)
        c_t = torch.empty(c_shape, device=a_t.device)
        Co = Op(c_t, *c_desc)
        _heads_mm(mode, A, Bo, Co, heads)
        ctx.save_for_backward(a_t, b_t)
        ctx.cfg = (mode, a_desc, b_desc, c_desc, heads)
        return c_t

    @staticmethod
    def backward(ctx, dc):
        a_t, b_t = ctx.saved_tensors
        mode, a_desc, b_desc, c_desc, heads = ctx.cfg
        dc = dc.contiguous()
        A, Bo, dC = Op(a_t, *a_desc), Op(b_t, *b_desc), Op(dc, *c_desc)
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.zeros_like(a_t)
            dA = A.like(da)
            if mode == "nt":
                _heads_mm("nn", dC, Bo, dA, heads)          # dA = dC B
            elif mode == "nn":
                _heads_mm("nt", dC, Bo, dA, heads)          # dA = dC B^T
            else:
                _heads_mm("nt", Bo, dC, dA, heads)          # dA = B dC^T
        if ctx.needs_input_grad[1]:
            db = torch.zeros_like(b_t)
            dB = Bo.like(db)
            if mode == "nt":
                _heads_mm("tn", dC, A, dB, heads)           # dB = dC^T A
            elif mode == "nn":
                _heads_mm("tn", A, dC, dB, heads)           # dB = A^T dC
            else:
                _heads_mm("nn", A, dC, dB, heads)           # dB = A dC
        return da, db, None, None, None, None, None, None


def heads_mm(a_t, b_t, mode, a_desc, b_desc, c_shape, c_desc, heads=HEADS):
    return HeadsMatmul.apply(a_t, b_t, mode, a_desc, b_desc, c_shape, c_desc, heads)


# --------------------------------------------------------------------------------------------------- primitives
class Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha):
        x = x.contiguous()
        y = torch.empty_like(x)
        Lr = x.shape[-1]
        L.check(L.lib().mhimx_softmax_rows(_st(), _ptr(x), _ptr(y), x.numel() // Lr, Lr, float(alpha)), "softmax_rows")
        ctx.save_for_backward(y)
        ctx.alpha = alpha
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        Lr = y.shape[-1]
        L.check(L.lib().mhimx_softmax_rows_bwd(_st(), _ptr(y), _ptr(dy), _ptr(dx), y.numel() // Lr, Lr, float(ctx.alpha)),
                "softmax_rows_bwd")
        return dx, None


class LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        y, mean, rstd = _layernorm_fwd(x, w, b)
        ctx.save_for_backward(x, w, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        M, E = x.shape
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(w)
        ws = torch.empty(2 * 512 * E, device=x.device)
        L.check(L.lib().mhimx_layernorm_bwd(_st(), _ptr(dy), _ptr(x), M, E, _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dw),
                                            _ptr(db), 0, _ptr(ws)), "layernorm_bwd")
        return dx, dw, db


class Linear(torch.autograd.Function):
    """y = dropout(x W^T + b) with the counter-based dropout stream (p = 0: none)."""

    @staticmethod
    def forward(ctx, x, w, b, drop_p, seed, tick):
        x = x.contiguous()
        y = ops.gemm_nt(x, w, bias=b, drop_p=drop_p, drop_seed=seed, drop_tick=tick, prec=_PREC)
        ctx.save_for_backward(x, w)
        ctx.cfg = (drop_p, seed, tick, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        drop_p, seed, tick, has_b = ctx.cfg
        dy = dy.contiguous()
        M, N = dy.shape
        dy = _redraw_mask(dy, drop_p, seed, tick, False)               # (ops.gemm_nt drew it: never the projection kernel's stream)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _gemm("nn", dy, 0, N, w, 0, w.shape[1], dx, 0, x.shape[1], M, x.shape[1], N)
        if ctx.needs_input_grad[1]:
            if N <= 16 and M >= 4096 and _PREC != "f32":
                # a few output rows (DSMIL's instance classifier, 512 -> C): the streaming thin-left-operand kernel instead of 128 x 128
                # tiles that are 98 % padding (4 tiles x 8 slabs = 32 workgroups: 167 us at M = 9705; this: ~20 us)
                dw = torch.empty((N, x.shape[1]), device=x.device)
                _heads_mm("tn", Op(dy, 0, 0, N, M, N), Op(x, 0, 0, x.shape[1], M, x.shape[1]), Op(dw, 0, 0, x.shape[1], N, x.shape[1]), 1)
            else:
                dw = ops.gemm_tn(dy, x, splits=8 if M >= 4096 else 1, prec=_PREC)
        if has_b and ctx.needs_input_grad[2]:
            db = ops.colsum(dy)
        return dx, dw, db, None, None, None


class Landmarks(torch.autograd.Function):
    """Means of l consecutive tokens of the q and k columns of qkv [n_pad, 1536] -> [256, 1024]."""

    @staticmethod
    def forward(ctx, qkv, l):
        T = qkv.shape[0]
        out = torch.empty((T // l, 2 * INNER), device=qkv.device)
        L.check(L.lib().mhimx_landmark_mean(_st(), _ptr(qkv), qkv.shape[1], T, l, 2 * INNER, _ptr(out)), "landmark_mean")
        ctx.cfg = (T, l, qkv.shape[1])
        return out

    @staticmethod
    def backward(ctx, dout):
        T, l, ld = ctx.cfg
        dq = torch.zeros((T, ld), device=dout.device)
        L.check(L.lib().mhimx_landmark_mean_bwd(_st(), _ptr(dout.contiguous()), T, l, 2 * INNER, _ptr(dq), ld, 0), "landmark_mean_bwd")
        return dq, None


class AffineIdent(torch.autograd.Function):
    """a*I + b*x on [B, n, n]."""

    @staticmethod
    def forward(ctx, x, a, b):
        x = x.contiguous()
        y = torch.empty_like(x)
        L.check(L.lib().mhimx_affine_ident(_st(), _ptr(x), _ptr(y), x.shape[0], x.shape[1], float(a), float(b)), "affine_ident")
        ctx.b = b
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        L.check(L.lib().mhimx_affine_ident(_st(), _ptr(dy), _ptr(dx), dy.shape[0], dy.shape[1], 0.0, float(ctx.b)), "affine_ident")
        return dx, None, None


def _bmm_affine(mode, a, b, out, alpha, ident, accumulate=False):
    """out[h] (+)= ident * I + alpha * op(a[h], b[h]) on contiguous [B, n, n] batches (mhimx_bmm_affine)."""
    B, n, _ = a.shape
    g = L.GemmNT(A=_ptr(a), lda=n, rows=None, B=_ptr(b), ldb=n, C=_ptr(out), ldc=n, M=n, N=n, K=n, accumulate=int(bool(accumulate)),
                 prec=L.PREC[_PREC])
    L.check(L.lib().mhimx_bmm_affine(_st(), _MODE[mode], C.byref(g), B, n * n, n * n, n * n, float(alpha), float(ident)), "mhimx_bmm_affine")
    return out


def _bmm_pair(p0, p1):
    """Two independent products (mode, a, b, out, alpha, accumulate) on [B, 256, 256] batches in ONE launch (mhimx_bmm_affine_pair)."""
    gs = []
    for (mode, a, b, out, alpha, acc) in (p0, p1):
        n = a.shape[-1]
        gs.append((_MODE[mode], L.GemmNT(A=_ptr(a), lda=n, rows=None, B=_ptr(b), ldb=n, C=_ptr(out), ldc=n, M=n, N=n, K=n,
                                         accumulate=int(bool(acc)), prec=L.PREC[_PREC]), float(alpha)))
    B, n, _ = p0[1].shape
    if n != 256:
        for (mode, a, b, out, alpha, acc) in (p0, p1):
            _bmm_affine(mode, a, b, out, alpha, 0.0, accumulate=acc)
        return
    L.check(L.lib().mhimx_bmm_affine_pair(_st(), gs[0][0], C.byref(gs[0][1]), gs[0][2], 0.0, gs[1][0], C.byref(gs[1][1]), gs[1][2], 0.0, B, n * n),
            "mhimx_bmm_affine_pair")


class MatmulAffine(torch.autograd.Function):
    """ident * I + alpha * (a @ b) on [B, n, n] in ONE launch (the pseudo-inverse iteration's "c I - M N" steps)."""

    @staticmethod
    def forward(ctx, a, b, ident, alpha):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        ctx.alpha = alpha
        return _bmm_affine("nn", a, b, torch.empty_like(a), alpha, ident)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        dy = dy.contiguous()
        da = _bmm_affine("nt", dy, b, torch.empty_like(a), ctx.alpha, 0.0) if ctx.needs_input_grad[0] else None      # alpha dy b^T
        db = _bmm_affine("tn", a, dy, torch.empty_like(b), ctx.alpha, 0.0) if ctx.needs_input_grad[1] else None      # alpha a^T dy
        return da, db, None, None


_CHAIN = os.environ.get("MHIMX_PINV_CHAIN", "1") != "0"
# MHIMX_PINV_LEVELS=3: the pseudo-inverse iteration in its expanded, three-level form (round 5, VERDICT r4 item 2a: 19 grid-wide stages of two
# products instead of 26 of one, the backward 4 stages per iteration instead of 5).  Built, parity-tested (tests/test_chain_gpu.py, the g7 / c3
# checks pass with it) and MEASURED EQUAL: the chain launches of a c3 step total 27.66 ms over 29 steps either way (profiles/r05_pinv_levels.md)
# - a stage's cost follows its outputs and hand-over (two products and five images per stage cost 7-8 us, one product 5 us), not its count.
_PINV3 = os.environ.get("MHIMX_PINV_LEVELS", "4") == "3"
_CTRS = {}


def _chain_counters(dev):
    """The counter block of mhimx_bmm_chain (include/mhimx.h), one per (device, stream): zero between launches by the kernel's contract."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    c = _CTRS.get(key)
    if c is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("mhimx_bmm_chain: run one eager step on the capture stream first (its counters are allocated and zeroed there)")
        c = _CTRS[key] = torch.zeros(1024, dtype=torch.int32, device=dev)     # the 513 words of mhimx_bmm_chain (+ room for the CH_PROF stamps)
    return c


def _step(kind, A=None, B=None, C=None, PN=None, PT=None, PN2=None, PT2=None, D=None, D2=None, alpha=1.0, ident=0.0, alpha2=0.0, ident2=0.0,
          dscale=1.0, d2scale=1.0):
    """One mhimx_bmm_step (include/mhimx.h) from tensors."""
    P = lambda t: _ptr(t) if t is not None else None
    return L.BmmStep(P(A), P(B), P(C), P(PN), P(PT), P(PN2), P(PT2), P(D), P(D2), alpha, ident, alpha2, ident2, dscale, d2scale, kind)


_IDLE = lambda: L.BmmStep(None, None, None, None, None, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1)


def _run_chain(steps, groups, dev):
    """steps: stage-major list (groups entries per stage) -> one mhimx_bmm_chain launch."""
    arr = (L.BmmStep * len(steps))(*steps)
    L.check(L.lib().mhimx_bmm_chain(_st(), arr, len(steps) // groups, groups, _ptr(_chain_counters(dev))), "mhimx_bmm_chain")


def chain_gave_up(dev):
    """True if a chain launch on this device ever gave up waiting for a workgroup (counters[512], mhimx.h) - synchronises; for tests."""
    return any(int(c[512].item()) != 0 for (d, _), c in _CTRS.items() if d == dev.index)


def _landmark_pinv_forward(lm, scale):
    """The landmark-only part of the block: attn2 = softmax(scale q~ k~^T) and its iterative pseudo-inverse (nystrom_attention.py:12-27,
    :115,:130): z0 = a2^T / (max col sum * max row sum), six iterations, every intermediate kept for the backward.  Depends on the
    landmark means alone, so a sequence-parallel layer runs it replicated on every rank."""
    lib = L.lib()
    m, dev = LANDMARKS, lm.device
    ql, kl = Op(lm, 0, DH, 2 * INNER, m, DH), Op(lm, INNER, DH, 2 * INNER, m, DH)
    a2 = torch.empty((HEADS, m, m), device=dev)
    _heads_mm("nt", ql, kl, batched(a2), HEADS)                       # q~ k~^T       nystrom:115
    L.check(lib.mhimx_softmax_rows(_st(), _ptr(a2), _ptr(a2), HEADS * m, m, float(scale)), "softmax_rows")
    # pseudo-inverse (nystrom_attention.py:12-27): z0 = a2^T / (max col sum * max row sum), six iterations, every intermediate kept
    z = torch.empty_like(a2)
    stats = torch.empty(4, device=dev)
    ws = torch.empty(2 * HEADS * m, device=dev)
    L.check(lib.mhimx_pinv_init(_st(), _ptr(a2), HEADS, m, _ptr(z), _ptr(stats), _ptr(ws)), "pinv_init")
    z0, chain = z, []
    if _CHAIN and _PREC == "bf16x3":
        # the 24 products as ONE persistent launch (mhimx_bmm_chain): matrices travel as split images (bf16 hi + lo planes, "N" as stored /
        # "T" transposed - the bytes of the fp32 matrix), every product also leaves the images the BACKWARD chain multiplies by; only the
        # result z exists in fp32
        if not _PINV3:
            img = lambda: torch.empty_like(a2)
            steps, a2N, a2T, zN, zT = [], img(), img(), img(), img()
            steps.append(_step(1, A=a2, PN=a2N, PT=a2T))
            steps.append(_step(1, A=z, PN=zN, PT=zT))
            for it in range(PINV_ITERS):
                azN, azT, t1N, t1T, t2N, t2T, t3N, t3T, znN, znT = (img() for _ in range(10))
                last = it == PINV_ITERS - 1
                zn = img() if last else None
                steps.append(_step(0, A=a2N, B=zT, PN=azN, PT=azT, PN2=t1N, PT2=t1T, alpha=1.0, alpha2=-1.0, ident2=7.0))   # az = a2 z, t1 = 7 I - az
                steps.append(_step(0, A=azN, B=t1T, PN=t2N, PT=t2T, alpha=-1.0, ident=15.0))                               # t2 = 15 I - az t1
                steps.append(_step(0, A=azN, B=t2T, PN=t3N, PT=t3T, alpha=-1.0, ident=13.0))                               # t3 = 13 I - az t2
                steps.append(_step(0, A=zN, B=t3T, C=zn, PN=None if last else znN, PT=None if last else znT, alpha=0.25))  # z' = 0.25 z t3
                chain.append((zN, zT, azT, t1N, t2N, t3N, a2T))
                z, zN, zT = zn, znN, znT
            _run_chain(steps, 1, dev)
            return a2, z, z0, stats, chain
        # (round 5) the iteration z' = 1/4 z (13 I - M (15 I - M (7 I - M))), M = a2 z, in its EXPANDED form: three dependent levels instead of
        # Horner's four -   M = a2 z;   P = z M  ||  N' = -15 I + 7 M - M M;   z' = 1/4 P N' + 13/4 z   - 18 grid-wide stages instead of 24
        # (a stage is ~4-5 us of hand-over around ~0.8 us of product).  Same polynomial; the rounding differs (3.25 z - 2.25 z at
        # convergence instead of z (13 - 9) / 4), inside the g7 / c3 tolerances.
        img = lambda: torch.empty_like(a2)
        steps, a2N, a2T, zN, zT = [], img(), img(), img(), img()
        steps += [_step(1, A=a2, PN=a2N, PT=a2T), _step(1, A=z, PN=zN, PT=zT)]
        zf = z                                                          # the fp32 iterate (the addend of the last level)
        for it in range(PINV_ITERS):
            M, MN, MT, PNi, PTi, NpN, NpT, zn = (img() for _ in range(8))
            last = it == PINV_ITERS - 1
            znN, znT = (None, None) if last else (img(), img())
            steps += [_step(0, A=a2N, B=zT, C=M, PN=MN, PT=MT), _IDLE(),                                          # M = a2 z
                      _step(0, A=zN, B=MT, PN=PNi, PT=PTi),                                                       # P = z M
                      _step(0, A=MN, B=MT, PN=NpN, PT=NpT, alpha=-1.0, ident=-15.0, D=M, dscale=7.0),             # N' = -15 I + 7 M - M M
                      _step(0, A=PNi, B=NpT, C=zn, PN=znN, PT=znT, alpha=0.25, D=zf, dscale=3.25), _IDLE()]        # z' = 1/4 P N' + 13/4 z
            chain.append((zN, zT, MN, MT, PNi, PTi, NpN, a2T))
            zf, zN, zT = zn, znN, znT
        _run_chain(steps, 2, dev)
        return a2, zf, z0, stats, chain
    for _ in range(PINV_ITERS):
        az, t1 = torch.empty_like(a2), torch.empty_like(a2)                 # az = a2 z and t1 = 7 I - az from ONE launch
        g_ = L.GemmNT(A=_ptr(a2), lda=m, rows=None, B=_ptr(z), ldb=m, C=_ptr(az), ldc=m, M=m, N=m, K=m, accumulate=0, prec=L.PREC[_PREC])
        L.check(lib.mhimx_bmm_affine2(_st(), _MODE["nn"], C.byref(g_), HEADS, m * m, m * m, m * m, 1.0, 0.0, _ptr(t1), -1.0, 7.0), "mhimx_bmm_affine2")
        t2 = _bmm_affine("nn", az, t1, torch.empty_like(a2), -1.0, 15.0)
        t3 = _bmm_affine("nn", az, t2, torch.empty_like(a2), -1.0, 13.0)
        zn = _bmm_affine("nn", z, t3, torch.empty_like(a2), 0.25, 0.0)
        chain.append((z, az, t1, t2, t3))
        z = zn
    return a2, z, z0, stats, chain


def _landmark_pinv_backward(lm, scale, a2, z0, stats, chain, dz, dlm, accumulate=True):
    """Backward of _landmark_pinv_forward: dz (gradient of the pseudo-inverse) -> the S2 terms of dq~ / dk~, ADDED into dlm
    (``accumulate=False``: written into it - a buffer of its own when the chain runs on a side stream)."""
    lib = L.lib()
    m, dev = LANDMARKS, lm.device
    ql, kl = Op(lm, 0, DH, 2 * INNER, m, DH), Op(lm, INNER, DH, 2 * INNER, m, DH)
    dql, dkl = ql.like(dlm), kl.like(dlm)
    # pseudo-inverse, backwards through the six iterations
    da2 = torch.empty_like(a2)
    first = True
    if len(chain[0]) == 7:
        # the images the forward chain left: the whole backward as TWO launches of mhimx_bmm_chain, two independent products per stage
        # (256 workgroups).  Per iteration, with dz the gradient of z' = 0.25 zp t3 (reference order nystrom_attention.py:21-25, reversed):
        #   1: dzp' = 0.25 dz t3^T          | dt3 = 0.25 zp^T dz
        #   2: daz' = -dt3 t2^T             | dt2 = -az^T dt3
        #   3: u    = daz' - dt2 t1^T       | w   = az^T dt2          (= -dt1: t1 = 7 I - az)
        #   4: daz  = u + w  (images only)
        #   5: da2 (+)= daz zp^T            | dzp = dzp' + a2^T daz   (the next iteration's dz)
        img = lambda: torch.empty_like(a2)
        dzN, dzT = img(), img()
        steps = [_step(1, A=dz, PN=dzN, PT=dzT), _IDLE()]
        for k, (zN, zT, azT, t1N, t2N, t3N, a2T) in enumerate(reversed(chain)):
            dzp, dt3N, dt3T, dazp, dt2N, dt2T, w, dazN, dazT, ndzN, ndzT = (img() for _ in range(11))
            last = k == PINV_ITERS - 1
            steps += [_step(0, A=dzN, B=t3N, C=dzp, alpha=0.25), _step(0, A=zT, B=dzT, PN=dt3N, PT=dt3T, alpha=0.25),
                      _step(0, A=dt3N, B=t2N, C=dazp, alpha=-1.0), _step(0, A=azT, B=dt3T, PN=dt2N, PT=dt2T, alpha=-1.0),
                      _step(0, A=dt2N, B=t1N, C=dazp, D=dazp, alpha=-1.0), _step(0, A=azT, B=dt2T, C=w, alpha=1.0),
                      _step(1, A=dazp, D=w, PN=dazN, PT=dazT), _IDLE(),
                      _step(0, A=dazN, B=zN, C=da2, D=None if first else da2, alpha=1.0),
                      _step(0, A=a2T, B=dazT, C=dzp if last else None, D=dzp, PN=None if last else ndzN, PT=None if last else ndzT, alpha=1.0)]
            dz, dzN, dzT, first = dzp, ndzN, ndzT, False
            if k == PINV_ITERS // 2 - 1:
                _run_chain(steps, 2, dev)
                steps = []
        _run_chain(steps, 2, dev)
        chain = ()
    elif len(chain[0]) == 8:
        # the images the forward chain left: the whole backward as TWO launches of mhimx_bmm_chain, two independent products per stage
        # (256 workgroups), FOUR stages per iteration.  With G the gradient of z' = 1/4 P N' + 13/4 z, P = z M, N' = -15 I + 7 M - M M, M = a2 z:
        #   1: dP  = 1/4 G N'^T                      | dN' = 1/4 P^T G
        #   2: U   = 7 dN' - dN' M^T                 | V   = -M^T dN'
        #   3: dM  = z^T dP + U + V  (images)        | dz' = dP M^T + 13/4 G
        #   4: da2 (+)= dM z^T                       | dz  = a2^T dM + dz'      (the next iteration's G)
        # (an X^T operand is the other image of X: N image of X^T = T image of X)
        img = lambda: torch.empty_like(a2)
        G, GN, GT = dz, img(), img()
        steps = [_step(1, A=G, PN=GN, PT=GT), _IDLE()]
        for k, (zN, zT, MN, MT, PNi, PTi, NpN, a2T) in enumerate(reversed(chain)):
            dPN, dPT, dNp, dNpN, dNpT, U, V, dMN, dMT, dzp = (img() for _ in range(10))
            last = k == PINV_ITERS - 1
            nGN, nGT = (None, None) if last else (img(), img())
            steps += [_step(0, A=GN, B=NpN, PN=dPN, PT=dPT, alpha=0.25), _step(0, A=PTi, B=GT, C=dNp, PN=dNpN, PT=dNpT, alpha=0.25),
                      _step(0, A=dNpN, B=MN, C=U, alpha=-1.0, D=dNp, dscale=7.0), _step(0, A=MT, B=dNpT, C=V, alpha=-1.0),
                      _step(0, A=zT, B=dPT, PN=dMN, PT=dMT, alpha=1.0, D=U, D2=V), _step(0, A=dPN, B=MN, C=dzp, alpha=1.0, D=G, dscale=3.25),
                      _step(0, A=dMN, B=zN, C=da2, D=None if first else da2, alpha=1.0),
                      _step(0, A=a2T, B=dMT, C=dzp, D=dzp, PN=nGN, PT=nGT, alpha=1.0)]
            G, GN, GT, first = dzp, nGN, nGT, False
            if k == PINV_ITERS // 2 - 1:
                _run_chain(steps, 2, dev)
                steps = []
        _run_chain(steps, 2, dev)
        dz = G
        chain = ()
    for (zp, az, t1, t2, t3) in reversed(chain):                                  # four pairs of independent products per iteration
        dzp, dt3, daz, dt2, dt1 = (torch.empty_like(dz) for _ in range(5))
        _bmm_pair(("nt", dz, t3, dzp, 0.25, False), ("tn", zp, dz, dt3, 0.25, False))        # z' = 0.25 zp t3
        _bmm_pair(("nt", dt3, t2, daz, -1.0, False), ("tn", az, dt3, dt2, -1.0, False))      # t3 = 13 I - az t2
        _bmm_pair(("nt", dt2, t1, daz, -1.0, True), ("tn", az, dt2, dt1, -1.0, False))       # t2 = 15 I - az t1
        L.check(lib.mhimx_axpby(_st(), _ptr(dt1), _ptr(daz), daz.numel(), -1.0, 1.0), "axpby")      # t1 = 7 I - az
        _bmm_pair(("nt", daz, zp, da2, 1.0, not first), ("tn", a2, daz, dzp, 1.0, True))      # az = a2 zp
        dz, first = dzp, False
    dinit = torch.empty_like(a2)
    ws2 = torch.empty(256, device=dev)
    L.check(lib.mhimx_pinv_init_bwd(_st(), _ptr(dz), _ptr(z0), _ptr(stats), HEADS, m, _ptr(dinit), _ptr(ws2)), "pinv_init_bwd")
    L.check(lib.mhimx_axpby(_st(), _ptr(dinit), _ptr(da2), da2.numel(), 1.0, 1.0), "axpby")
    L.check(lib.mhimx_softmax_rows_bwd(_st(), _ptr(a2), _ptr(da2), _ptr(da2), HEADS * m, m, float(scale)), "softmax_rows_bwd")
    ds2 = batched(da2)
    _heads_mm("nn", ds2, kl, dql, HEADS, accumulate=accumulate)        # s2 = q~ k~^T: dq~ += ds2 k~
    _heads_mm("tn", ds2, ql, dkl, HEADS, accumulate=accumulate)        #               dk~ += ds2^T q~


# The pseudo-inverse chain (24 dependent launches of 128 workgroups forward, 24 pairs backward: ~8-13 us each, latency-bound) depends on
# the landmark means alone; the streamed token passes beside it (a3 v forward; its backward) fill the chip with thousands of workgroups.
# They are independent, but the chain runs inline on the one stream.  MEASURED (round 3, c3, same box, hipGraph replay): 11.07 ms with the
# chain on a side stream (a second branch of the captured hipGraph) against 10.88 ms on one stream - six fork / join pairs per step cost
# more in cross-queue signalling (~60 us each on this ROCm build) than the overlapped launches save; the accumulation window of the ABMIL
# trainer forks once per 8 bags and gains 1.7x from the same mechanism.


def _core_forward(qkv, conv_w, l, scale):
    """The block between to_qkv and to_out (nystrom_attention.py:93-136) on the streamed kernels; returns (out [T, 512], saved)."""
    lib = L.lib()
    T, ld = qkv.shape
    m, dev = LANDMARKS, qkv.device
    lm = torch.empty((m, 2 * INNER), device=dev)
    L.check(lib.mhimx_landmark_mean(_st(), _ptr(qkv), ld, T, l, 2 * INNER, _ptr(lm)), "landmark_mean")
    ql, kl = Op(lm, 0, DH, 2 * INNER, m, DH), Op(lm, INNER, DH, 2 * INNER, m, DH)
    no = ops.NysOperands(qkv, lm, scale)
    a2, z, z0, stats, chain = _landmark_pinv_forward(lm, scale)        # the landmark-only chain
    a3v, lse3 = ops.nys_a3v_fwd(no)                                    # softmax_n(q~ k^T) v   nystrom:116,131,133
    w2 = _heads_product("nn", z, a3v, m, DH)                            # pinv (a3 v)
    wc = conv_w.reshape(HEADS, -1).contiguous()
    out = torch.empty((T, INNER), device=dev)
    L.check(lib.mhimx_resconv(_st(), _ptr(qkv, 2 * INNER), ld, _ptr(wc), wc.shape[1], DH, T, INNER, _ptr(out), INNER, 0, 0),
            "resconv")                                                # out = res_conv(v)   nystrom:135-136 (written FIRST: the
    out, lse1 = ops.nys_out_fwd(no, w2, out, accumulate=True)          # attention adds to it in its epilogue - one pass over out less)
    return out, (qkv, lm, a2, z, z0, stats, chain, a3v, w2, wc, lse1, lse3, no.ws, l, scale, conv_w.shape)


def _core_backward(saved, dout):
    """Gradients of _core_forward w.r.t. qkv and the residual-convolution weight."""
    lib = L.lib()
    qkv, lm, a2, z, z0, stats, chain, a3v, w2, wc, lse1, lse3, nws, l, scale, wshape = saved
    T, ld = qkv.shape
    m, dev, KS = LANDMARKS, qkv.device, wc.shape[1]
    ql, kl = Op(lm, 0, DH, 2 * INNER, m, DH), Op(lm, INNER, DH, 2 * INNER, m, DH)
    no = ops.NysOperands(qkv, lm, scale, ws=nws)
    dqkv = torch.empty_like(qkv)                                       # every column block is written before it is added to
    dlm = torch.empty_like(lm)
    dql, dkl = ql.like(dlm), kl.like(dlm)
    # residual convolution: dv = flip-conv(dout), d(conv weight)
    L.check(lib.mhimx_resconv(_st(), _ptr(dout), INNER, _ptr(wc), KS, DH, T, INNER, _ptr(dqkv, 2 * INNER), ld, 0, 1), "resconv")
    dwc = torch.empty_like(wc)
    ws = torch.empty(lib.mhimx_resconv_dw_ws_floats(T, INNER, DH, KS), device=dev)
    L.check(lib.mhimx_resconv_dw(_st(), _ptr(dout), INNER, _ptr(qkv, 2 * INNER), ld, KS, DH, T, INNER, _ptr(dwc), _ptr(ws)), "resconv_dw")
    # out = a1 w2: dq, the S1 term of dk~, dw2 = a1^T dout
    dw2 = ops.nys_out_bwd(no, w2, dout, lse1, dqkv, dlm)
    # w2 = z a3v
    dz = _heads_product("nt", dw2, a3v, m, m)                          # dz = dw2 a3v^T
    dlm2 = torch.empty_like(dlm)
    _landmark_pinv_backward(lm, scale, a2, z0, stats, chain, dz, dlm2, accumulate=False)
    da3v = _heads_product("tn", z, dw2, m, DH)                         # da3v = z^T dw2
    # a3v = a3 v: dk, dv +=, the S3 term of dq~
    ops.nys_a3v_bwd(no, a3v, da3v, lse3, dqkv, dlm, accumulate_dv=True)
    L.check(lib.mhimx_axpby(_st(), _ptr(dlm2), _ptr(dlm), dlm.numel(), 1.0, 1.0), "axpby")      # + the attn2 terms
    L.check(lib.mhimx_landmark_mean_bwd(_st(), _ptr(dlm), T, l, 2 * INNER, _ptr(dqkv), ld, 1), "landmark_mean_bwd")
    return dqkv, dwc.reshape(wshape)



class NystromCore(torch.autograd.Function):
    """The attention block between to_qkv and to_out (nystrom_attention.py:93-136) as ONE autograd node with a hand-written backward:
    landmark means, the three score products, their softmaxes, the pseudo-inverse, a1 (pinv (a3 v)) and the residual convolution.
    attn1 [n, 256] and attn3 [256, n] are NEVER materialised (csrc/nys_flash.hip): a3 v is an online-softmax pass over the tokens,
    a1 w2 a second pass, and the backward recomputes every score tile from q / k with the saved log-sum-exps (two passes per product:
    one for the token-side gradients, one for the landmark-side reductions).  Every gradient lands in ONE dqkv buffer; no torch
    arithmetic touches token data.
    Returns (out [T, 512], lm, z, lse3) - the last three (not differentiable) for the cls-row attention map of return_attn."""

    @staticmethod
    def forward(ctx, qkv, conv_w, l, scale):
        out, saved = _core_forward(qkv, conv_w, l, scale)
        ctx.saved = saved
        lm, z, lse3 = saved[1], saved[3], saved[11]
        ctx.mark_non_differentiable(lm, z, lse3)
        return out, lm, z, lse3

    @staticmethod
    def backward(ctx, dout, _g1, _g2, _g3):
        saved, ctx.saved = ctx.saved, None
        dqkv, dwc = _core_backward(saved, dout.contiguous())
        return dqkv, dwc, None, None


# ------------------------------------------------------------------------------------------------ the layer shell
# What TransLayerFn and nystrom_sharded.ShardedTransLayerFn launch alike around their cores ("the layer shell"): plain
# functions of views, a tick or None and flags the caller computed.  ``big``: the single-pass projection kernel and ITS dropout stream.
def _layernorm_fwd(x, w, b):
    """LayerNorm of the rows of x [M, E] (contiguous) -> (xn, mean [M], rstd [M])."""
    M, E = x.shape
    xn = torch.empty_like(x)
    mean, rstd = torch.empty(M, device=x.device), torch.empty(M, device=x.device)
    L.check(L.lib().mhimx_layernorm_fwd(_st(), _ptr(x), M, E, _ptr(w), _ptr(b), _ptr(xn), _ptr(mean), _ptr(rstd)), "layernorm_fwd")
    return xn, mean, rstd


def _layernorm_bwd_res(dxn, x, ln_w, mean, rstd, dy):
    """LayerNorm backward with the residual's gradient added inside: dx = LayerNorm'(dxn) + dy -> (dx, d weight, d bias)."""
    M, E = x.shape
    dx, dlw, dlb = torch.empty_like(x), torch.empty_like(ln_w), torch.empty_like(ln_w)
    ws = torch.empty(2 * 512 * E, device=x.device)
    L.check(L.lib().mhimx_layernorm_bwd_res(_st(), _ptr(dxn), _ptr(x), M, E, _ptr(ln_w), _ptr(mean), _ptr(rstd), _ptr(dy), _ptr(dx),
                                            _ptr(dlw), _ptr(dlb), 0, _ptr(ws)), "layernorm_bwd_res")
    return dx, dlw, dlb


def _to_qkv(xn, w_qkv, qkv, big):
    """qkv [rows of xn, 1536] = xn w_qkv^T (no bias), written into the caller's rows."""
    if big:
        # to_qkv on the single-pass projection kernel (one "model" of width 1536: raw fp32 rows split on their way into LDS,
        # 160 x 256 tiles; 330 -> ~270 us at n = 50 000)
        ops.bag_project(xn, [ops.ProjHead(ops.pair_planes(w_qkv), None, out=qkv)], act=0)
    else:
        ops.gemm_nt(xn, w_qkv, out=qkv, prec=_PREC)


def _to_out_res(a, w_out, b_out, x, drop_p, seed, tick, big):
    """y = x + dropout(a w_out^T + b_out) (nystrom_attention.py:60-63, baseline.py:213-218); tick: the device step counter or None."""
    if big:                                   # to_out on the projection kernel too (bias + its own dropout stream in the epilogue; 154 -> ~85 us)
        return ops.bag_project(a, [ops.ProjHead(ops.pair_planes(w_out), b_out, drop_p=drop_p, drop_seed=seed, resid=x)], act=0,
                               drop_tick=tick if drop_p > 0 else None)[0].out                             # y = x + dropout(to_out(.)): one launch
    y = ops.gemm_nt(a, w_out, bias=b_out, drop_p=drop_p, drop_seed=seed, drop_tick=tick, prec=_PREC)
    L.check(L.lib().mhimx_axpby(_st(), _ptr(x), _ptr(y), y.numel(), 1.0, 1.0), "axpby")                   # y += x
    return y


def _redraw_mask(dy, drop_p, seed, tick, big):
    """dy under the forward's dropout mask again, from the stream of the kernel that drew it (dy itself where nothing was dropped)."""
    if not drop_p > 0:
        return dy
    M, N = dy.shape
    g = torch.empty_like(dy)
    fn = L.lib().mhimx_dropout_apply_proj if big else L.lib().mhimx_dropout_apply
    L.check(fn(_st(), _ptr(dy), _ptr(g), M, N, float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF, None if tick is None else _ptr(tick)),
            "dropout_apply")
    return g


def _linear_wgrad(dy, a, pair, want_bias=True):
    """(d weight = dy^T a, d bias = column sums of dy or None) of y = a W^T + b; pair: the matrix-core-image weight-gradient pair
    (csrc/wgrad.hip), where the caller found it applicable (ops.bag_wgrad_ok)."""
    n = dy.shape[0]
    if pair:
        return ops.bag_wgrad(dy, None, a, None, n, want_bias=want_bias)
    return ops.gemm_tn(dy, a, splits=8 if n >= 4096 else 1, prec=_PREC), ops.colsum(dy) if want_bias else None


def _heads_product(mode, a, b, rows, cols):
    """op(a_h, b_h) of two contiguous batches of per-head matrices -> a fresh [8, rows, cols]."""
    c = torch.empty((HEADS, rows, cols), device=a.device)
    _heads_mm(mode, batched(a), batched(b), batched(c), HEADS)
    return c


def _cls_row(qkv, row, lm, z, scale):
    """u [8, 256] = softmax(scale q_cls k~^T) z, q_cls in row ``row`` of qkv: attn1's cls row times the pseudo-inverse (nystrom:143-150)."""
    m = LANDMARKS
    ld = qkv.shape[1]
    a1c = torch.empty((HEADS, 1, m), device=qkv.device)                    # attn1's cls row: softmax(scale q_cls k~^T)
    _heads_mm("nt", Op(qkv, row * ld, DH, ld, 1, DH), Op(lm, INNER, DH, 2 * INNER, m, DH), batched(a1c), HEADS)
    L.check(L.lib().mhimx_softmax_rows(_st(), _ptr(a1c), _ptr(a1c), HEADS, m, float(scale)), "softmax_rows")
    return _heads_product("nn", a1c, z, 1, m).reshape(HEADS, m)


def _cls_attention(qkv, lm, z, lse3, pad, scale):
    """nystrom:143-150: the cls token's attention row [8, T] = (attn1[cls] pinv) attn3, without attn1 / attn3."""
    return ops.nys_cls_attn(ops.NysOperands(qkv, lm, scale), lse3, _cls_row(qkv, pad, lm, z, scale))


class TransLayerFn(torch.autograd.Function):
    """y = x + to_out(Nystrom(to_qkv(LayerNorm(x))))  (baseline.py:213-218, nystrom_attention.py:65-152) as ONE autograd node.
    The front zero padding (nystrom:70-73) is a zero fill of the first rows of the qkv buffer (to_qkv has no bias), the last-n-rows
    slice (nystrom:142) a pointer offset, and the residual's gradient is added inside the LayerNorm backward: no cat / slice copy, no
    zero-filled gradient, no autograd addition touches token data."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w_qkv, w_out, b_out, conv_w, drop_p, seed, tick, scale, need_attn):
        x = x.contiguous()
        n = x.shape[0]
        m, dev = LANDMARKS, x.device
        pad = (m - n % m) % m
        T, l = n + pad, math.ceil(n / m)
        big = n >= 2048 and _PREC == "bf16x3"              # from the tokens without the padding: the projection kernels see those rows only
        xn, mean, rstd = _layernorm_fwd(x, ln_w, ln_b)
        qkv = torch.empty((T, 3 * INNER), device=dev)
        if pad:
            qkv[:pad].zero_()
        _to_qkv(xn, w_qkv, qkv[pad:], big)
        out, saved = _core_forward(qkv, conv_w, l, scale)
        y = _to_out_res(out[pad:], w_out, b_out, x, drop_p, seed, tick, big)
        ctx.saved = (x, xn, mean, rstd, ln_w, w_qkv, w_out, out, saved)
        ctx.cfg = (pad, drop_p, seed, tick, big)
        if not need_attn:
            return y
        lm, z, lse3 = saved[1], saved[3], saved[11]
        r = _cls_attention(qkv, lm, z, lse3, pad, scale)
        attn, v = r[:, pad + 1:], qkv[pad + 1:, 2 * INNER:]
        ctx.mark_non_differentiable(attn, v)
        return y, attn, v

    @staticmethod
    def backward(ctx, dy, *_):
        x, xn, mean, rstd, ln_w, w_qkv, w_out, out, saved = ctx.saved
        ctx.saved = None
        pad, drop_p, seed, tick, big = ctx.cfg
        dy = dy.contiguous()
        n, E = x.shape
        T, dev = n + pad, x.device
        g = _redraw_mask(dy, drop_p, seed, tick, big)
        dout = torch.empty((T, INNER), device=dev)
        if pad:
            dout[:pad].zero_()
        if big:                                    # data gradients as products with the transposed weights on the projection kernel
            ops.bag_project(g, [ops.ProjHead(ops.pair_planes_t(w_out), None, out=dout[pad:])], act=0)
        elif n >= 2048 and _PREC != "f32":
            ops.gemm_nt(g, ops.transpose(w_out), out=dout[pad:], prec=_PREC)
        else:
            _gemm("nn", g, 0, E, w_out, 0, INNER, dout, pad * INNER, INNER, n, INNER, E)
        wg = big and ops.bag_wgrad_ok(x, INNER, n)                                    # the matrix-core-image weight-gradient pair (csrc/wgrad.hip)
        dw_out, db_out = _linear_wgrad(g, out[pad:], wg)
        dqkv, dwc = _core_backward(saved, dout)
        dxn = torch.empty_like(x)
        if big:
            ops.bag_project(dqkv[pad:], [ops.ProjHead(ops.pair_planes_t(w_qkv), None, out=dxn)], act=0)
        elif n >= 2048 and _PREC != "f32":
            ops.gemm_nt(dqkv[pad:], ops.transpose(w_qkv), out=dxn, prec=_PREC)
        else:
            _gemm("nn", dqkv, pad * 3 * INNER, 3 * INNER, w_qkv, 0, E, dxn, 0, E, n, E, 3 * INNER)
        dw_qkv, _ = _linear_wgrad(dqkv[pad:], xn, wg, want_bias=False)
        dx, dlw, dlb = _layernorm_bwd_res(dxn, x, ln_w, mean, rstd, dy)
        return dx, dlw, dlb, dw_qkv, dw_out, db_out, dwc, None, None, None, None, None


class PinvInit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        a = a.contiguous()
        B, n, _ = a.shape
        z = torch.empty_like(a)
        stats = torch.empty(4, device=a.device)
        ws = torch.empty(2 * B * n, device=a.device)
        L.check(L.lib().mhimx_pinv_init(_st(), _ptr(a), B, n, _ptr(z), _ptr(stats), _ptr(ws)), "pinv_init")
        ctx.save_for_backward(z, stats)
        return z

    @staticmethod
    def backward(ctx, dz):
        z, stats = ctx.saved_tensors
        dz = dz.contiguous()
        B, n, _ = z.shape
        da = torch.empty_like(z)
        ws = torch.empty(256, device=z.device)
        L.check(L.lib().mhimx_pinv_init_bwd(_st(), _ptr(dz), _ptr(z), _ptr(stats), B, n, _ptr(da), _ptr(ws)), "pinv_init_bwd")
        return da


class ResConv(torch.autograd.Function):
    """Depth-wise 33-tap convolution along tokens of the v columns of qkv -> [n_pad, 512]."""

    @staticmethod
    def forward(ctx, qkv, w):
        T, ld = qkv.shape
        out = torch.empty((T, INNER), device=qkv.device)
        w2 = w.reshape(HEADS, -1).contiguous()
        L.check(L.lib().mhimx_resconv(_st(), _ptr(qkv, 2 * INNER), ld, _ptr(w2), w2.shape[1], DH, T, INNER, _ptr(out), INNER, 0, 0),
                "resconv")
        ctx.save_for_backward(qkv, w2)
        ctx.wshape = w.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, w2 = ctx.saved_tensors
        dout = dout.contiguous()
        T, ld = qkv.shape
        KS = w2.shape[1]
        dq = dw = None
        if ctx.needs_input_grad[0]:
            dq = torch.zeros_like(qkv)
            L.check(L.lib().mhimx_resconv(_st(), _ptr(dout), INNER, _ptr(w2), KS, DH, T, INNER, _ptr(dq, 2 * INNER), ld, 0, 1), "resconv")
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w2)
            ws = torch.empty(L.lib().mhimx_resconv_dw_ws_floats(T, INNER, DH, KS), device=qkv.device)
            L.check(L.lib().mhimx_resconv_dw(_st(), _ptr(dout), INNER, _ptr(qkv, 2 * INNER), ld, KS, DH, T, INNER, _ptr(dw), _ptr(ws)),
                    "resconv_dw")
            dw = dw.reshape(ctx.wshape)
        return dq, dw


class PPEG(torch.autograd.Function):
    """y = PPEG(x) (emb_position.py:85-120).  skip > 0: the first `skip` rows (the cls token: baseline.py:265-266
    `cat([x[:1], ppeg(x[1:])])`) pass through unchanged and the stencil runs on the rest - the kernels take the row offset as a pointer
    offset, so neither the slice, the cat, nor their zero-filled / summed gradients exist."""

    @staticmethod
    def forward(ctx, x, w7, w5, w3, b7, b5, b3, grid=0, skip=0):
        x = x.contiguous()
        N, Cc = x.shape[0] - skip, x.shape[1]
        ctx.grid, ctx.skip = int(grid), int(skip)
        wc, bc = torch.empty((Cc, 49), device=x.device), torch.empty(Cc, device=x.device)
        lib = L.lib()
        L.check(lib.mhimx_ppeg_combine(_st(), _ptr(w7.contiguous()), _ptr(w5.contiguous()), _ptr(w3.contiguous()), _ptr(b7), _ptr(b5),
                                       _ptr(b3), Cc, _ptr(wc), _ptr(bc)), "ppeg_combine")
        y = torch.empty_like(x)
        if skip:
            y[:skip].copy_(x[:skip])
        L.check(lib.mhimx_ppeg_fwd(_st(), _ptr(x, skip * Cc), N, Cc, _ptr(wc), _ptr(bc), _ptr(y, skip * Cc), int(grid)), "ppeg_fwd")
        ctx.save_for_backward(x, wc)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wc = ctx.saved_tensors
        dy = dy.contiguous()
        skip = ctx.skip
        N, Cc = x.shape[0] - skip, x.shape[1]
        dx, dwc, dbc = torch.empty_like(x), torch.empty_like(wc), torch.empty(Cc, device=x.device)
        if skip:
            dx[:skip].copy_(dy[:skip])
        ws = torch.empty(L.lib().mhimx_ppeg_bwd_ws_floats(N, Cc), device=x.device)
        L.check(L.lib().mhimx_ppeg_bwd(_st(), _ptr(dy, skip * Cc), _ptr(x, skip * Cc), N, Cc, _ptr(wc), _ptr(dx, skip * Cc), _ptr(dwc), _ptr(dbc),
                                       _ptr(ws), ctx.grid), "ppeg_bwd")
        g = dwc.view(Cc, 1, 7, 7)
        # the three kernels were summed centre-aligned into one 7x7 stencil: their gradients are its centred windows
        return (dx, g.contiguous(), g[:, :, 1:6, 1:6].contiguous(), g[:, :, 2:5, 2:5].contiguous(), dbc, dbc.clone(), dbc.clone(), None, None)


class Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        y = a.contiguous().clone()
        L.check(L.lib().mhimx_axpby(_st(), _ptr(b.contiguous()), _ptr(y), y.numel(), 1.0, 1.0), "axpby")
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


# --------------------------------------------------------------------------------------------------- modules
class _P(nn.Module):
    def __init__(self, **tensors):
        super().__init__()
        for k, v in tensors.items():
            setattr(self, k, nn.Parameter(v) if v is not None else None)


def _lin(i, o, bias=True):
    w = torch.empty(o, i)
    nn.init.xavier_normal_(w)
    return _P(weight=w, bias=torch.zeros(o) if bias else None)


class _Slot(nn.Module):
    pass


class NystromAttention(nn.Module):
    """Parameters + forward of modules/nystrom_attention.NystromAttention (dim 512, 8 x 64, 256 landmarks, 6 pinv iters)."""

    def __init__(self, dim=512, dropout=0.1):
        super().__init__()
        self.to_qkv = _lin(dim, 3 * INNER, bias=False)
        self.to_out = nn.Sequential(_lin(INNER, dim), _Slot())
        w = torch.empty(HEADS, 1, CONV_K, 1)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.res_conv = _P(weight=w)
        self.dropout = dropout
        self.scale = DH ** -0.5

    def forward(self, x, return_attn=False, no_norm=False, seed=0, tick=None, training=False):
        """x [n, dim] -> out [n, dim] (+ views: cls-row attention [8, n-1] and v [n-1, (8 64)] when return_attn)."""
        n, dim = x.shape
        m = LANDMARKS
        pad = (m - n % m) % m
        if pad:
            x = torch.cat([x.new_zeros(pad, dim), x], 0)                      # nystrom_attention.py:70-73 (front padding)
        T = x.shape[0]
        l = math.ceil(n / m)
        qkv = Linear.apply(x, self.to_qkv.weight, None, 0.0, 0, None)          # [T, 1536]: q | k | v, heads = 64-column groups
        ld = 3 * INNER
        p = self.dropout if training else 0.0
        if _PREC != "f32" and not (return_attn and no_norm):
            # one autograd node for the whole block (hand-written backward, no torch arithmetic on token data)
            out, lm, z, lse3 = NystromCore.apply(qkv, self.res_conv.weight, l, self.scale)
            y = Linear.apply(out[pad:], self.to_out[0].weight, self.to_out[0].bias, p, seed, tick)   # last n rows (nystrom:142)
            if not return_attn:
                return y
            with torch.no_grad():                                              # nystrom:143-150: the cls token's attention row
                r = _cls_attention(qkv, lm, z, lse3, pad, self.scale)
                return y, r[:, pad + 1:], qkv[pad + 1:, 2 * INNER:]
        lm = Landmarks.apply(qkv, l)                                          # [256, 1024]: q~ | k~
        q_d, k_d, v_d = (0, DH, ld, T, DH), (INNER, DH, ld, T, DH), (2 * INNER, DH, ld, T, DH)
        ql_d, kl_d = (0, DH, 2 * INNER, m, DH), (INNER, DH, 2 * INNER, m, DH)
        bat = lambda r, c: (0, r * c, c, r, c)
        s1 = heads_mm(qkv, lm, "nt", q_d, kl_d, (HEADS, T, m), bat(T, m))     # q k~^T        nystrom:114
        s2 = heads_mm(lm, lm, "nt", ql_d, kl_d, (HEADS, m, m), bat(m, m))     # q~ k~^T       nystrom:115
        s3 = heads_mm(lm, qkv, "nt", ql_d, k_d, (HEADS, m, T), bat(m, T))     # q~ k^T        nystrom:116
        a1, a2, a3 = Softmax.apply(s1, self.scale), Softmax.apply(s2, self.scale), Softmax.apply(s3, self.scale)
        z = _pinv(a2)
        a3v = heads_mm(a3, qkv, "nn", bat(m, T), v_d, (HEADS, m, DH), bat(m, DH))         # a3 v          [8,256,64]
        w2 = heads_mm(z, a3v, "nn", bat(m, m), bat(m, DH), (HEADS, m, DH), bat(m, DH))    # pinv (a3 v)
        out = heads_mm(a1, w2, "nn", bat(T, m), bat(m, DH), (T, INNER), (0, DH, INNER, T, DH))   # a1 (pinv a3 v) -> [T, (h d)]
        out = Add.apply(out, ResConv.apply(qkv, self.res_conv.weight))         # nystrom:135-136
        y = Linear.apply(out[pad:], self.to_out[0].weight, self.to_out[0].bias, p, seed, tick)   # last n rows (nystrom:142)
        if not return_attn:
            return y
        with torch.no_grad():                                                  # nystrom:143-150: the cls token's attention row
            if no_norm:
                b1, b2, b3 = s1 * self.scale, _pinv(s2 * self.scale), s3 * self.scale
            else:
                b1, b2, b3 = a1, z, a3
            u = heads_mm(b1[:, pad:pad + 1].contiguous(), b2, "nn", bat(1, m), bat(m, m), (HEADS, 1, m), bat(1, m))
            r = heads_mm(u, b3, "nn", bat(1, m), bat(m, T), (HEADS, 1, T), bat(1, T))
            attn = r[:, 0, pad + 1:]
            v = qkv[pad + 1:, 2 * INNER:]                                     # [n-1, (h d)] strided view of the packed rows
        return y, attn, v


def _pinv(a):
    """moore_penrose_iter_pinv (nystrom_attention.py:12-27) on [8, 256, 256]."""
    B, n, _ = a.shape
    bat = (0, n * n, n, n, n)
    mm = lambda p, q: heads_mm(p, q, "nn", bat, bat, (B, n, n), bat, B)
    z = PinvInit.apply(a)
    fused = _PREC != "f32" and n % 64 == 0 and n <= 512            # (the exact-fp32 test mode keeps the generic kernels)
    for _ in range(PINV_ITERS):
        if fused:
            az = MatmulAffine.apply(a, z, 0.0, 1.0)
            t = AffineIdent.apply(az, 7.0, -1.0)
            t = MatmulAffine.apply(az, t, 15.0, -1.0)
            t = MatmulAffine.apply(az, t, 13.0, -1.0)
            z = MatmulAffine.apply(z, t, 0.0, 0.25)
            continue
        az = mm(a, z)
        t = AffineIdent.apply(az, 7.0, -1.0)
        t = AffineIdent.apply(mm(az, t), 15.0, -1.0)
        t = AffineIdent.apply(mm(az, t), 13.0, -1.0)
        z = AffineIdent.apply(mm(z, t), 0.0, 0.25)
    return z


class TransLayer(nn.Module):
    def __init__(self, dim=512):
        super().__init__()
        self.norm = _P(weight=torch.ones(dim), bias=torch.zeros(dim))
        self.attn = NystromAttention(dim)

    def forward(self, x, need_attn=False, no_norm=False, seed=0, tick=None, training=False):
        if _PREC != "f32" and not (need_attn and no_norm):
            a = self.attn
            return TransLayerFn.apply(x, self.norm.weight, self.norm.bias, a.to_qkv.weight, a.to_out[0].weight, a.to_out[0].bias,
                                      a.res_conv.weight, a.dropout if training else 0.0, seed, tick, a.scale, bool(need_attn))
        xn = LayerNorm.apply(x, self.norm.weight, self.norm.bias)
        if need_attn:
            z, attn, v = self.attn(xn, True, no_norm, seed, tick, training)
            return Add.apply(x, z), attn, v
        return Add.apply(x, self.attn(xn, False, no_norm, seed, tick, training))


class _Conv(nn.Module):
    def __init__(self, dim, k):
        super().__init__()
        w = torch.empty(dim, 1, k, k)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(k * k)
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.empty(dim).uniform_(-bound, bound))


class _PPEG(nn.Module):
    def __init__(self, dim=512):
        super().__init__()
        self.proj, self.proj1, self.proj2 = _Conv(dim, 7), _Conv(dim, 5), _Conv(dim, 3)

    def forward(self, x, grid=0, skip=0):
        """grid = 0: emb_position.PPEG (side ceil(sqrt(N)), wrap, zero-padded to 7 x 7 below 37 tokens); grid > 0: the explicit
        grid x grid layout of modules/transmil.PPEG.forward(x, H, W).  skip: leading rows (the cls token) that pass through."""
        return PPEG.apply(x, self.proj.weight, self.proj1.weight, self.proj2.weight, self.proj.bias, self.proj1.bias, self.proj2.bias, grid, skip)


class SAttention(nn.Module):
    """mhim_modules/baseline.SAttention (pos='ppeg', pos_pos=0)."""

    def __init__(self, mlp_dim=512, head=8):
        super().__init__()
        if mlp_dim != 512:
            raise L.MhimxError("the Nystrom encoder kernels are built for mlp_dim = 512 (8 heads x 64, 256 landmarks)")
        if head != HEADS:
            # the reference builds heads=head, dim_head=dim//8 (baseline.py:202): another head count is another model (to_qkv is
            # 3*head*64 wide, res_conv has `head` channels) - refuse it instead of silently building the 8-head one
            raise L.MhimxError(f"the Nystrom encoder kernels are built for 8 heads (got head={head})")
        self.norm = _P(weight=torch.ones(mlp_dim), bias=torch.zeros(mlp_dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, mlp_dim))
        self.layer1 = TransLayer(mlp_dim)
        self.layer2 = TransLayer(mlp_dim)
        self.pos_embedding = _PPEG(mlp_dim)

    def forward(self, h, return_attn=False, no_norm=False, seeds=(0, 0), tick=None, training=False, has_cls=False):
        """h [N, 512] tokens -> cls feature [512] (+ [attn_l1, attn_l2] each [8, N], v of layer 1 [N, (8 64)]).  has_cls: h is
        [1 + N, 512] with the cls token already in row 0 (the caller assembled the matrix in place; its gradient reaches cls_token there)."""
        x = h if has_cls else torch.cat([self.cls_token.view(1, -1), h], 0)
        attn = []
        if return_attn:
            x, a, v = self.layer1(x, True, no_norm, seeds[0], tick, training)
            attn.append(a)
        else:
            x = self.layer1(x, False, no_norm, seeds[0], tick, training)
        x = self.pos_embedding(x, skip=1)                                       # baseline.py:265-266: cat([x[:1], ppeg(x[1:])])
        if return_attn:
            x, a, _ = self.layer2(x, True, no_norm, seeds[1], tick, training)
            attn.append(a)
        else:
            x = self.layer2(x, False, no_norm, seeds[1], tick, training)
        x = LayerNorm.apply(x[:1].contiguous(), self.norm.weight, self.norm.bias)   # only the cls row is used (baseline.py:276-278)
        return (x[0], attn, v) if return_attn else x[0]
