"""The device-drawn select against its exact model (oracle/mhim_oracle.py: select_rows_parts - numpy integers, nothing from the device), bit
for bit on every route that runs the production draw of csrc/select_dev.hpp: ops.select_rows (the LEAN kernel forms; n_sel == k takes
the full form), ops.select_rows with the mask-id list (the full forms), ops.select_rows_img and ops.select_rows_many.  Row ids are
integers: torch.equal only.  The cases and the model's answers: tests/select_cases.py (computed once)."""
import numpy as np
import pytest
import torch

from tests import select_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tick(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV) if v else None       # (tick 0: no device counter, the by-value seed alone)


@pytest.mark.parametrize("merge_first", [False, True])
def test_select_rows_equals_the_model(merge_first):
    from mhim_mil_amd import ops
    for (n, k, ns, R), s, seed, tick, largest, p in C.single():
        got = ops.select_rows(_dev(s), k, ns, R, seed, tick=_tick(tick), largest=largest, merge_first=merge_first)
        assert torch.equal(got, _dev(C.rows(p, merge_first))), (n, k, ns, R)


@pytest.mark.parametrize("merge_first", [False, True])
def test_select_rows_with_mask_ids_equals_the_model(merge_first):
    """The full (non-LEAN) kernel forms: the same rows, and the id list = kept rows ascending, then the masked rows in draw order
    (n_sel == k draws nothing: every candidate is masked, through the value-ordered list - value descending, then index)."""
    from mhim_mil_amd import ops
    for (n, k, ns, R), s, seed, tick, largest, p in C.single():
        rows, ids = ops.select_rows(_dev(s), k, ns, R, seed, tick=_tick(tick), largest=largest, want_mask_ids=True, merge_first=merge_first)
        assert torch.equal(rows, _dev(C.rows(p, merge_first))), (n, k, ns, R)
        assert torch.equal(ids, _dev(np.concatenate([p["kept"], p["masked"] if ns < k else p["top"]]))), (n, k, ns, R)


@pytest.mark.parametrize("merge_first", [False, True])
def test_select_rows_img_equals_the_model(merge_first):
    """rows as above; the image = [stay | 0.. | merged from the offset | 0.. to a multiple of 32] (the offset: the next multiple of 32 at
    or behind the rows that stay, and one tile further for every other case)"""
    from mhim_mil_amd import ops
    for j, ((n, k, ns, R), s, seed, tick, largest, p) in enumerate(C.single()):
        stay, merged = p["stay"], p["merged"]
        off = -(-stay.shape[0] // 32) * 32 + 32 * (j & 1)
        img = np.zeros(-(-(off + R) // 32) * 32, dtype=np.int64)
        img[:stay.shape[0]] = stay
        img[off:off + merged.shape[0]] = merged
        rows, got = ops.select_rows_img(_dev(s), k, ns, R, seed, off, tick=_tick(tick), largest=largest, merge_first=merge_first)
        assert torch.equal(rows, _dev(C.rows(p, merge_first))), (n, k, ns, R)
        assert torch.equal(got, _dev(img)), (n, k, ns, R, off)


def _many(cases, gaps, merge_first):
    from mhim_mil_amd import ops
    table, parts, r0, o0 = [], [], 0, 0
    for ((n, k, ns, R), s, seed, _), gap in zip(cases, gaps):
        parts.append(np.full(gap, 2.0, dtype=np.float32))                   # (above every score: a read outside a bag would change the top-k)
        r0, o0 = r0 + gap, o0 + gap
        table.append((r0, n, k, ns, R, o0, seed))
        parts.append(s)
        r0, o0 = r0 + n, o0 + n - ns
    return ops.select_rows_many(_dev(np.concatenate(parts)), table, tick=_tick(C.TICK), merge_first=merge_first)


@pytest.mark.parametrize("merge_first", [False, True])
def test_select_rows_many_equals_the_model(merge_first):
    """every case as one bag of ONE call (one launch on the 16-keys class, LDS sized for k = 4096), odd gaps between the bags"""
    cases = C.many()
    got = _many(cases, [2 * j + 1 for j in range(len(cases))], merge_first)
    for v, ((n, k, ns, R), _, _, p) in zip(got, cases):
        assert torch.equal(v, _dev(C.rows(p, merge_first))), (n, k, ns, R)


def test_select_rows_many_a_bag_alone_equals_the_model():
    """one bag per call: the launch's own keys-per-thread class (4 / 10 / 16) and LDS size"""
    cases = C.many()
    for j in (0, 3, 5, 6, 8, 10):
        (n, k, ns, R), _, _, p = cases[j]
        got = _many([cases[j]], [j], True)[0]
        assert torch.equal(got, _dev(C.rows(p, True))), (n, k, ns, R)
