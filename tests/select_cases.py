"""The cases of the select oracle tests (test_select_oracle_cpu.py, test_select_oracle_gpu.py): counts, scores, seeds, and the model's
answer for each (oracle/mhim_oracle.py: select_rows_parts), computed once per process and left unchanged."""
import numpy as np

from oracle import mhim_oracle as O

TICK = 0x1234567
# (N, k, n_sel, merge_R): the keys-per-thread class edges (4096 | 4097, 10240 | 10241, 16384), the partial / all / none branches of the
# Merge draw, k = 1, not a power of two, 4096 and k == N
COUNTS = [(1, 1, 0, 0), (1, 1, 0, 1), (2, 2, 1, 1), (33, 7, 3, 10), (65, 64, 64, 0), (257, 100, 50, 207), (4096, 4096, 2000, 1000),
          (4097, 300, 150, 395), (10240, 613, 307, 993), (10241, 4096, 1000, 3000), (16384, 983, 492, 1589)]
# per case: (scores, seed, tick, largest) - all-equal and four-level scores, seeds with a high word and small integers, ticks 0 and not
_KIND = ["rand", "rand", "equal", "q4", "rand", "q4", "rand", "equal", "rand", "q4", "rand"]
_SEED = [3, 0xABCDEF0123456789, 7, 0x9E3779B97F4A7C15, 12345, 0xD1B54A32D192ED03, 11, 0x0F1E2D3C4B5A6978, 0xFEDCBA9876543210, 99,
         0x8000000000000001]
_TICK = [0, 5, 0, TICK, 0, 9, TICK, 0, TICK, 1, TICK]
_LARGEST = [True, True, True, False, True, True, True, True, False, True, True]
_CACHE = {}


def scores(kind, n, seed):
    rng = np.random.RandomState(seed)
    if kind == "q4":
        return (rng.randint(0, 4, n) * 0.25).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.375, dtype=np.float32)
    return rng.random_sample(n).astype(np.float32)


def single():
    """[(counts, score, seed, tick, largest, parts)]: every case under its own seed, tick and direction (the single-bag routes)"""
    if "single" not in _CACHE:
        out = []
        for j, (n, k, ns, R) in enumerate(COUNTS):
            s = scores(_KIND[j], n, 40 + j)
            out.append(((n, k, ns, R), s, _SEED[j], _TICK[j], _LARGEST[j], O.select_rows_parts(s, k, ns, R, _SEED[j], _TICK[j], _LARGEST[j])))
        _CACHE["single"] = out
    return _CACHE["single"]


def many():
    """[(counts, score, seed, parts)] under the one tick TICK, largest scores first (what a select_rows_many call can ask for)"""
    if "many" not in _CACHE:
        out = []
        for j, (n, k, ns, R) in enumerate(COUNTS):
            s = scores(_KIND[j], n, 40 + j)
            out.append(((n, k, ns, R), s, _SEED[j], O.select_rows_parts(s, k, ns, R, _SEED[j], TICK, True)))
        _CACHE["many"] = out
    return _CACHE["many"]


def rows(parts, merge_first):
    return np.concatenate([parts["merged"], parts["stay"]] if merge_first else [parts["stay"], parts["merged"]])
