"""Survival validation without a GPU: the two CPU restatements of the censored concordance index (tests/surv_oracle.py) against each
other and against hand-computed answers, and every refusal of mhimx_surv_nll / mhimx_cindex's argument checks (they run before any
device call: the pointers are made-up addresses)."""
import os
import re

import numpy as np
import pytest

from mhim_mil_amd import _lib as L
from tests import surv_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [0x7F0000000000 + (k << 36) for k in range(8)]        # never dereferenced; 256-byte aligned


# ------------------------------------------------------------------------------------------------ the restatements
def _heavy_ties(seed, n, resample):
    """Integer times from a small range (events and censored samples share times), risks on a coarse grid, and - with ``resample`` -
    duplicates of whole samples, as a bootstrap draw makes them."""
    rng = np.random.default_rng(seed)
    event = rng.random(n) < 0.5
    time = rng.integers(0, max(2, n // 4), n).astype(np.float64)
    risk = (rng.integers(-3, 4, n) * 0.25).astype(np.float32)
    if resample:
        idx = rng.integers(0, n, n)
        event, time, risk = event[idx], time[idx], risk[idx]
    return event, time, risk


@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("n", [2, 3, 17, 64, 301])
def test_the_two_restatements_agree_exactly(n, resample):
    for seed in range(6):
        event, time, risk = _heavy_ties(100 * n + seed, n, resample)
        a, b = SO.cindex_pairs(event, time, risk), SO.cindex_sorted(event, time, risk)
        assert np.array_equal(SO.as_row(a), SO.as_row(b), equal_nan=True), (n, seed, a, b)
        assert a["concordant"] + a["discordant"] + a["tied_risk"] >= a["tied_time"]


def test_heavy_tie_data_has_every_kind_of_pair():
    event, time, risk = _heavy_ties(7, 301, True)
    a = SO.cindex_pairs(event, time, risk)
    assert min(a["concordant"], a["discordant"], a["tied_risk"], a["tied_time"]) > 0 and 0.0 < a["cindex"] < 1.0


@pytest.mark.parametrize("form", [SO.cindex_pairs, SO.cindex_sorted])
def test_known_answers(form):
    ones = np.ones(5, bool)
    t = np.arange(5.0)
    # earlier event = higher risk: all 10 pairs concordant
    r = form(ones, t, -t.astype(np.float32))
    assert (r["cindex"], r["concordant"], r["discordant"], r["tied_risk"], r["tied_time"]) == (1.0, 10.0, 0.0, 0.0, 0.0)
    r = form(ones, t, t.astype(np.float32))
    assert (r["cindex"], r["concordant"], r["discordant"]) == (0.0, 0.0, 10.0)
    r = form(ones, t, np.zeros(5, np.float32))
    assert (r["cindex"], r["tied_risk"], r["concordant"], r["discordant"]) == (0.5, 10.0, 0.0, 0.0)
    # times (1, 1, 2): an event and a censored sample at time 1, an event at 2.  Comparable: (0, 1) at the same time and (0, 2);
    # risks 3 > 2 and 3 > 1: both concordant
    r = form(np.array([1, 0, 1], bool), np.array([1.0, 1.0, 2.0]), np.array([3, 2, 1], np.float32))
    assert (r["cindex"], r["concordant"], r["discordant"], r["tied_risk"], r["tied_time"]) == (1.0, 2.0, 0.0, 0.0, 1.0)
    # two events at one time are not comparable (a sample drawn twice is never compared with itself)
    r = form(np.array([1, 1], bool), np.array([4.0, 4.0]), np.array([1, 2], np.float32))
    assert np.isnan(r["cindex"]) and r["concordant"] + r["discordant"] + r["tied_risk"] == 0
    # all censored: no comparable pair
    r = form(np.zeros(5, bool), t, t.astype(np.float32))
    assert np.isnan(r["cindex"]) and SO.as_row(r)[1:].sum() == 0
    # the tie rule: 4e-9 and 8e-9 apart are ties, 1.2e-8 is not.  Pairs (0, 1): 1.2e-8 apart, concordant; (0, 2): 4e-9, (1, 2): 8e-9
    r = form(ones[:3], t[:3], np.array([1.2e-8, 0.0, 8e-9], np.float32))
    assert (r["concordant"], r["discordant"], r["tied_risk"], r["cindex"]) == (1.0, 0.0, 2.0, 2.0 / 3.0)
    r = form(ones[:3], t[:3], np.array([0.0, 1.2e-8, 2.4e-8], np.float32))
    assert (r["concordant"], r["discordant"], r["tied_risk"], r["cindex"]) == (0.0, 3.0, 0.0, 0.0)


def test_nll_surv_restatement_by_hand():
    import torch
    lg = torch.tensor([[0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)
    risk, losses = SO.nll_surv(lg, torch.tensor([1, 0]), torch.tensor([0.0, 1.0]), alpha=0.0)
    # h = 1/2, S = (1/2, 1/4): uncensored in bin 1: -(log S_0 + log h_1) = 2 log 2; censored in bin 0: -log S_0 = log 2
    np.testing.assert_allclose(risk.numpy(), [-0.75, -0.75], rtol=1e-15)
    np.testing.assert_allclose(losses.numpy(), [2 * np.log(2), np.log(2)], rtol=1e-15)
    _, l4 = SO.nll_surv(lg, torch.tensor([1, 0]), torch.tensor([0.0, 1.0]), alpha=0.4)
    np.testing.assert_allclose(l4.numpy(), [2 * np.log(2), 0.6 * np.log(2)], rtol=1e-15)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name, val in (("SURV_MAX_N", L.SURV_MAX_N), ("CINDEX_MAX_N", L.CINDEX_MAX_N), ("CINDEX_MAX_B", L.CINDEX_MAX_B),
                      ("CINDEX_MAX_BN", L.CINDEX_MAX_BN)):
        assert int(re.search(rf"#define MHIMX_{name} (\d+)", hdr).group(1)) == val
    lib = L.lib()
    for name in ("mhimx_surv_nll", "mhimx_cindex", "mhimx_cindex_ws_bytes"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    for cite in ("train_utils.py:8-37", "engines/base_engine.py:636-643", "engines/metrics.py:66-104"):
        assert cite in hdr                                     # the reference lines the calls replace
    assert lib.mhimx_version() == L.ABI_VERSION == 620         # additions do not bump the ABI version


def _nll(logits=P[0], ld=4, Y=P[1], c=P[2], n=10, K=4, alpha=0.0, eps=1e-7, risk=P[3], losses=P[4], g=P[5]):
    lib = L.lib()
    r = lib.mhimx_surv_nll(None, logits, ld, Y, c, n, K, alpha, eps, 1.0, risk, losses, g)
    return r, lib.mhimx_last_error()


NLL_REFUSED = [("null logits", dict(logits=None), b"null"), ("null Y", dict(Y=None), b"null"), ("null c", dict(c=None), b"null"),
               ("null risk", dict(risk=None), b"null"), ("null losses", dict(losses=None), b"null"),
               ("K 0", dict(K=0, ld=1), b"K=0"), ("K 17", dict(K=17, ld=17), b"K=17"), ("n 0", dict(n=0), b"n=0"),
               ("n max + 1", dict(n=L.SURV_MAX_N + 1), b"n="), ("ld < K", dict(ld=3), b"ld=3"), ("eps < 0", dict(eps=-1e-7), b"eps="),
               ("eps 0", dict(eps=0.0), b"eps="), ("alpha > 1", dict(alpha=1.5), b"alpha=")]


@pytest.mark.parametrize("what,kw,word", NLL_REFUSED, ids=[r[0] for r in NLL_REFUSED])
def test_surv_nll_refusals(what, kw, word):
    r, msg = _nll(**kw)
    assert r < 0 and msg.startswith(b"mhimx_surv_nll:") and word in msg, (what, r, msg)


def _ci(event=P[0], time=P[1], risk=P[2], n=100, idx=P[3], B=4, tol=1e-8, out=P[4], ws=P[5], ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = 1 << 40
    r = lib.mhimx_cindex(None, event, time, risk, n, idx, B, tol, out, ws, ws_bytes)
    return r, lib.mhimx_last_error()


CI_REFUSED = [("null event", dict(event=None), b"null"), ("null time", dict(time=None), b"null"), ("null risk", dict(risk=None), b"null"),
              ("null out", dict(out=None), b"null"), ("null ws", dict(ws=None), b"workspace"), ("n 0", dict(n=0), b"n=0"),
              ("n max + 1", dict(n=L.CINDEX_MAX_N + 1, B=1), b"n="), ("B 0", dict(B=0), b"B=0"), ("B max + 1", dict(B=L.CINDEX_MAX_B + 1), b"B="),
              ("B n too large", dict(n=L.CINDEX_MAX_N, B=33), b"B * n"), ("B 4 without sample_idx", dict(idx=None), b"sample_idx"),
              ("tied_tol < 0", dict(tol=-1e-8), b"tied_tol"), ("ws unaligned", dict(ws=P[5] + 8), b"256-byte aligned")]


@pytest.mark.parametrize("what,kw,word", CI_REFUSED, ids=[r[0] for r in CI_REFUSED])
def test_cindex_refusals(what, kw, word):
    r, msg = _ci(**kw)
    assert r < 0 and msg.startswith(b"mhimx_cindex:") and word in msg, (what, r, msg)


def test_cindex_workspace_one_byte_short_and_b1_without_indices():
    lib = L.lib()
    need = lib.mhimx_cindex_ws_bytes(100, 4)
    r, msg = _ci(ws_bytes=need - 1)
    assert r < 0 and msg.startswith(b"mhimx_cindex:") and b"workspace too small" in msg
    # B == 1 may go without sample_idx: with everything else in order the call gets as far as the workspace's size, its last check
    r, msg = _ci(B=1, idx=None, ws_bytes=lib.mhimx_cindex_ws_bytes(100, 1) - 1)
    assert r < 0 and b"workspace too small" in msg


def test_cindex_ws_bytes_is_positive_and_monotone():
    lib = L.lib()
    prev_n = 0
    for n in (1, 2, 255, 256, 257, 1000, 100000, L.CINDEX_MAX_N):
        prev_b = 0
        for B in (1, 2, 25, 32):
            b = lib.mhimx_cindex_ws_bytes(n, B)
            assert b > 0 and b >= prev_b and b >= 13 * n * B, (n, B, b)
            prev_b = b
        assert prev_b >= prev_n
        prev_n = prev_b
    assert lib.mhimx_cindex_ws_bytes(1000, 1000) < 16 << 20              # the documented use: 1000 patients, 1000 resamples
    for n, B in ((0, 1), (1, 0), (L.CINDEX_MAX_N + 1, 1), (1, L.CINDEX_MAX_B + 1), (L.CINDEX_MAX_N, 33)):
        assert lib.mhimx_cindex_ws_bytes(n, B) < 0 and lib.mhimx_last_error().startswith(b"mhimx_cindex_ws_bytes:")


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    from mhim_mil_amd import ops
    with pytest.raises(L.MhimxError, match="surv_nll"):
        ops.surv_nll(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64), torch.zeros(3))
    with pytest.raises(L.MhimxError, match="GPU"):
        ops.cindex(torch.ones(3, dtype=torch.uint8), torch.zeros(3, dtype=torch.float64), torch.zeros(3))
