"""The exact model of the device-drawn select (oracle/mhim_oracle.py: feistel_small, select_rows_parts, select_rows) on its own: what the
GPU routes are compared with in test_select_oracle_gpu.py has to be a draw at all - a permutation, subsets of the right sets and sizes."""
import numpy as np
import pytest

from oracle import mhim_oracle as O
from tests import select_cases as C

KEYS = [(0, 0), (1, 2), (0x9E3779B9, 0x85EBCA6B), (0xFFFFFFFF, 0xFFFFFFFF), (0x12345678, 0x0BADF00D)]


@pytest.mark.parametrize("k0,k1", KEYS)
def test_feistel_small_is_a_bijection(k0, k1):
    for n in range(1, 71):
        p = O.feistel_small(np.arange(n), n, O.small_perm_bits(n), k0, k1)
        assert p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n)), (n, k0, k1)


def test_mono32_orders_like_the_scores():
    v = np.array([-3.5, -0.25, 0.0, 1e-30, 0.375, 0.5, 1.0, 7e20], dtype=np.float32)
    up, down = O.mono32(v, True).astype(np.int64), O.mono32(v, False).astype(np.int64)
    assert (np.diff(up) > 0).all() and (np.diff(down) < 0).all()


def test_the_model_draws_subsets_of_the_right_sets():
    for (n, k, ns, R), s, seed, tick, largest, p in C.single():
        what = (n, k, ns, R)
        L = n - ns
        top = set(O.topk_indices(s, k, largest).tolist())
        assert set(p["top"].tolist()) == top and set(p["cand"].tolist()) == top and (np.diff(p["cand"]) > 0).all(), what
        masked = p["masked"]
        assert masked.shape == (ns,) and len(set(masked.tolist())) == ns and set(masked.tolist()) <= top, what
        assert p["kept"].shape == (L,) and (np.diff(p["kept"]) > 0).all() and not set(p["kept"].tolist()) & set(masked.tolist()), what
        stay, merged = p["stay"], p["merged"]
        assert merged.shape == (min(R, L),) and stay.shape == (L - min(R, L),), what
        assert (np.diff(stay) > 0).all() and (np.diff(merged) > 0).all() and not set(stay.tolist()) & set(merged.tolist()), what
        for mf in (False, True):
            rows = O.select_rows(s, k, ns, R, seed, tick, largest, mf)
            assert rows.dtype == np.int64 and np.array_equal(np.sort(rows), p["kept"]), what
            assert np.array_equal(rows, np.concatenate([merged, stay] if mf else [stay, merged])), what


def test_the_draw_depends_on_seed_and_tick():
    s = C.scores("rand", 4097, 1)
    a = O.select_rows(s, 300, 150, 395, 11, 0)
    assert not np.array_equal(a, O.select_rows(s, 300, 150, 395, 12, 0)) and not np.array_equal(a, O.select_rows(s, 300, 150, 395, 11, 1))
    assert np.array_equal(a, O.select_rows(s, 300, 150, 395, 11 + (1 << 64), 0))          # the seed is a 64-bit word
