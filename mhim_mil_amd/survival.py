"""The survival task's loss on the HIP path.

``NLLSurvLoss`` is a drop-in for the reference's criterion of that name (train_utils.py:27-37; the discrete-time negative log-likelihood
of train_utils.py:8-25): same constructor, same call signature, so the reference's ``surv_train`` loop runs with it unchanged.  Called
with ``logits`` - the training form - the mean loss and its gradient come from ONE launch of mhimx_surv_nll (csrc/surv.hip): the forward
also writes ``d mean / d logits``, the backward only scales it.  Called with ``hazards`` / ``S`` - the form the reference's validation
loop uses (engines/base_engine.py:636-639) - there are no logits to hand the kernel, and the loss is the reference's formula in plain
torch; ``validate.surv_validate`` itself never takes that form: it runs the kernel on the logits.
"""
from __future__ import annotations

import torch

from . import ops

EPS = 1e-7                                   # train_utils.py:8 (nll_loss's default; the reference's class never passes another)


class _NLLSurvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, Y, c, alpha, eps):
        lg = logits.detach()
        if lg.dtype != torch.float32:
            lg = lg.float()
        if lg.stride(-1) != 1:
            lg = lg.contiguous()
        n = lg.shape[0]
        _, losses, g = ops.surv_nll(lg, Y, c, alpha=alpha, eps=eps, g_scale=1.0 / n)
        ctx.save_for_backward(g)
        ctx.in_dtype = logits.dtype
        return losses.mean()

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return (g * grad_out).to(ctx.in_dtype), None, None, None, None


def nll_loss(hazards, S, Y, c, alpha=0.4, eps=EPS):
    """train_utils.py:8-25 on given hazards and survival curve (plain torch, differentiable)."""
    n = len(Y)
    Y = Y.view(n, 1)
    c = c.view(n, 1).float()
    S_pad = torch.cat([torch.ones_like(c), S], 1)
    unc = -(1 - c) * (torch.log(torch.gather(S_pad, 1, Y).clamp(min=eps)) + torch.log(torch.gather(hazards, 1, Y).clamp(min=eps)))
    cen = -c * torch.log(torch.gather(S_pad, 1, Y + 1).clamp(min=eps))
    return ((1 - alpha) * (cen + unc) + alpha * unc).mean()


class NLLSurvLoss(object):
    """train_utils.py:27-37.  ``criterion(Y=bins, c=censorships, logits=logits)`` -> the mean loss, a tensor whose backward is the
    kernel's gradient; ``criterion(Y=, c=, hazards=, S=)`` -> the same loss from a given curve."""

    def __init__(self, alpha=0.):
        self.alpha = alpha

    def __call__(self, Y, c, logits=None, hazards=None, S=None, alpha=None):
        if alpha is None:
            alpha = self.alpha
        if hazards is not None:
            if S is None:
                S = torch.cumprod(1 - hazards, dim=1)
            return nll_loss(hazards, S, Y, c, alpha=alpha)
        if logits is None:
            raise ops.L.MhimxError("NLLSurvLoss: give logits= (or hazards= and S=)")
        logits = logits.reshape(Y.numel(), -1)
        Y = Y.reshape(-1).to(device=logits.device, dtype=torch.int64).contiguous()
        c = c.reshape(-1).to(device=logits.device, dtype=torch.float32).contiguous()
        return _NLLSurvFn.apply(logits, Y, c, float(alpha), EPS)
