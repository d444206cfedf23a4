"""CPU restatement of the survival task's loss and metric (numpy / torch), the yardstick of tests/test_surv_cpu.py and test_surv_gpu.py.

* ``nll_surv``: the discrete-time NLL survival loss and the risk score, formula by formula as the reference computes them
  (train_utils.py:8-25 before its ``.mean()``; hazards / survival curve / risk: engines/base_engine.py:636-643), in the dtype of the
  logits it is given (fp64 for the yardstick, fp32 to measure what fp32 costs) and differentiable.
* ``cindex_pairs``: the censored concordance index (engines/metrics.py:79: sksurv's concordance_index_censored with tied_tol=1e-8) from
  its definition over all ordered pairs, O(n^2).
* ``cindex_sorted``: the same index the way sksurv organises it - sort by time, walk the groups of tied times, compare each event with
  everything behind its group and with the censored members of its group.
The two C-index forms share no code beyond the tie rule on the risks and must agree in every count.
"""
import numpy as np
import torch

KEYS = ("cindex", "concordant", "discordant", "tied_risk", "tied_time")


def nll_surv(logits, Y, c, alpha=0.0, eps=1e-7):
    """-> (risk [n], losses [n]) in logits.dtype.  Y [n] int64 inside [0, K), c [n] (1 = censored)."""
    n = logits.shape[0]
    Y = Y.view(n, 1)
    c = c.view(n, 1).to(logits.dtype)
    hazards = torch.sigmoid(logits)                                          # base_engine.py:636
    S = torch.cumprod(1 - hazards, dim=1)                                    # base_engine.py:637
    risk = -torch.sum(S, dim=1)                                              # base_engine.py:643
    S_pad = torch.cat([torch.ones_like(c), S], 1)                            # train_utils.py:14
    unc = -(1 - c) * (torch.log(torch.gather(S_pad, 1, Y).clamp(min=eps)) + torch.log(torch.gather(hazards, 1, Y).clamp(min=eps)))
    cen = -c * torch.log(torch.gather(S_pad, 1, Y + 1).clamp(min=eps))       # train_utils.py:21
    losses = (1 - alpha) * (cen + unc) + alpha * unc                         # train_utils.py:22-23
    return risk, losses.view(n)


def clamp_margins(logits, Y, eps=1e-7):
    """The three clamped quantities of every row in fp64 (S_pad[Y], h[Y], S_pad[Y + 1]) relative to eps: a test's inputs keep them away
    from 1 so that fp32 and fp64 take the same side of every clamp."""
    lg = logits.double()
    n = lg.shape[0]
    h = torch.sigmoid(lg)
    S_pad = torch.cat([torch.ones(n, 1, dtype=torch.float64), torch.cumprod(1 - h, 1)], 1)
    Y = Y.view(n, 1)
    return torch.cat([torch.gather(S_pad, 1, Y), torch.gather(h, 1, Y), torch.gather(S_pad, 1, Y + 1)], 1) / eps


def _tied(rj, ri, tied_tol):
    return np.abs(rj - ri) <= np.float32(tied_tol)                           # the difference and the comparison in fp32


def _result(con, tie, cmp, tt):
    ci = (con + 0.5 * tie) / cmp if cmp else float("nan")                    # exact fp64 operands, one division
    return dict(zip(KEYS, (ci, float(con), float(cmp - con - tie), float(tie), float(tt))))


def cindex_pairs(event, time, risk, tied_tol=1e-8):
    """Pair (i, j) is comparable iff event_i and (time_j > time_i or (time_j == time_i and not event_j)); tied iff |risk_j - risk_i| <=
    tied_tol; concordant iff not tied and risk_j < risk_i; discordant otherwise.  -> dict over KEYS (counts as floats)."""
    event = np.asarray(event).astype(bool)
    time = np.asarray(time, dtype=np.float64)
    risk = np.asarray(risk, dtype=np.float32)
    cmp = con = tie = tt = 0
    rows = np.flatnonzero(event)
    for lo in range(0, rows.size, 512):
        i = rows[lo:lo + 512]
        same = (time[None, :] == time[i, None]) & ~event[None, :]
        comparable = (time[None, :] > time[i, None]) | same
        tied = _tied(risk[None, :], risk[i, None], tied_tol) & comparable
        cmp += int(comparable.sum())
        tt += int(same.sum())
        tie += int(tied.sum())
        con += int((comparable & ~tied & (risk[None, :] < risk[i, None])).sum())
    return _result(con, tie, cmp, tt)


def cindex_sorted(event, time, risk, tied_tol=1e-8):
    """The sort-and-walk form: samples in time order; inside a group of equal times every event is compared with the group's censored
    members (those pairs are ``tied_time``) and with every sample behind the group."""
    event = np.asarray(event).astype(bool)
    time = np.asarray(time, dtype=np.float64)
    risk = np.asarray(risk, dtype=np.float32)
    order = np.argsort(time, kind="stable")
    ev, tm, rk = event[order], time[order], risk[order]
    n = tm.size
    cmp = con = tie = tt = 0
    start = 0
    while start < n:
        end = start + 1
        while end < n and tm[end] == tm[start]:
            end += 1
        group_censored = np.flatnonzero(~ev[start:end]) + start
        for i in range(start, end):
            if not ev[i]:
                continue
            others = np.concatenate([group_censored, np.arange(end, n)])
            tt += group_censored.size
            cmp += others.size
            tied = _tied(rk[others], rk[i], tied_tol)
            tie += int(tied.sum())
            con += int((~tied & (rk[others] < rk[i])).sum())
        start = end
    return _result(con, tie, cmp, tt)


def as_row(d):
    return np.array([d[k] for k in KEYS], dtype=np.float64)
