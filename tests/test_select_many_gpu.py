"""mhimx_select_rows_many (csrc/select_many.hip) on the device: every bag of a call against the per-bag call it stands for -
ops.select_rows up to 16 384 rows, the random_perm / select_mask / random_perm sequence above - bit for bit (row ids are integers: no
tolerance anywhere in this file); MHIM.student_rows_many against a loop over student_rows; the row lists mhimx_ragged_window_run leaves
against the same per-bag calls on the window's own scores."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TICK = 0x1234567
# the v2 recipe of the window tests (HAM mask only, ABMIL with the pseudo score, Merge with 5 queries) and their trainer, kept here so that
# this file stands on its own
V2 = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999,
          merge_ratio=0.9, temp_t=0.1, dropout=0.0)
D = 256
ROUTE = "mhimx_ragged_window_run"


def _tick(v=TICK):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


# (N, k, n_sel, merge_R): the 4 / 10 / 16 keys-per-thread classes and their edges; k = 1, not a power of two, 4096 and k == N; n_sel = 0
# and n_sel == k; merge_R = 0 and merge_R == N - n_sel
CLASSES = [(1, 1, 0, 1), (2, 2, 1, 1), (33, 7, 0, 10), (257, 100, 100, 0), (1024, 1, 0, 500), (4096, 4096, 2000, 1000), (4097, 300, 150, 3947),
           (10240, 613, 307, 993), (10241, 4096, 4096, 3000), (16384, 983, 492, 1589)]
_CACHE = {}


def _scores(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "free":                        # tie-free: a permutation of n distinct values in (0, 1)
        return ((torch.randperm(n, generator=g).float() + 1.0) / (n + 1)).to(DEV)
    if kind == "q4":                          # tie-heavy: four levels
        return (torch.randint(0, 4, (n,), generator=g).float() * 0.25).to(DEV)
    if kind == "equal":
        return torch.full((n,), 0.375, device=DEV)
    return torch.rand(n, generator=g).to(DEV)


def _ref_rows(score, k, n_sel, R, seed, tick, merge_first):
    """what the per-bag calls write for one bag (computed once per (scores, counts, seed, tick, order) and shared between the tests)"""
    from mhim_mil_amd import ops
    N = score.numel()
    score = score.clone()                     # (its own allocation: nothing of a neighbour within reach)
    if N <= 16384:
        out = torch.full((max(N - n_sel, 1),), -7, dtype=torch.int64, device=DEV)
        return ops.select_rows(score, k, n_sel, R, seed, tick=tick, merge_first=merge_first, out=out[:N - n_sel]).clone()
    pm = ops.random_perm(k, seed + 0x51ED270B, tick=tick, device=score.device)
    ids, _, _ = ops.select_mask(score, k, n_sel, True, perm=pm if n_sel < k else None)
    rows = ops.random_perm(N - n_sel, seed ^ 0x3C6EF372FE94F82B, tick=tick, src=ids)
    Lk = N - n_sel - R
    return torch.cat([rows[Lk:], rows[:Lk]]) if merge_first else rows


def _class_case():
    """the ten bags of CLASSES: their scores, seeds and the per-bag reference lists for both orders of the two groups"""
    if "classes" not in _CACHE:
        tick = _tick()
        scores = [_scores("rand", n, 100 + j) for j, (n, *_) in enumerate(CLASSES)]
        seeds = [(0x9E3779B97F4A7C15 * (j + 3) + 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF for j in range(len(CLASSES))]
        ref = {mf: [_ref_rows(s, k, ns, R, sd, tick, mf) for s, (n, k, ns, R), sd in zip(scores, CLASSES, seeds)] for mf in (False, True)}
        torch.cuda.synchronize()
        _CACHE["classes"] = (scores, seeds, ref)
    return _CACHE["classes"]


def _call(scores, counts, seeds, order, gaps, tick, merge_first, poison=True):
    """one select_rows_many over the bags in ``order`` (indices into scores / counts): packed score and output vectors with ``gaps[j]``
    unused entries in front of the j-th bag of the call (odd numbers: no alignment).  Returns {bag index: rows}, and checks that nothing but
    the output ranges was written."""
    from mhim_mil_amd import ops
    table, parts, r0, o0 = [], [], 0, 0
    for j, b in enumerate(order):
        n, k, ns, R = counts[b]
        parts.append(torch.full((gaps[j],), 2.0, device=DEV))              # (above every score: a read outside a bag would change the top-k)
        r0 += gaps[j]
        o0 += gaps[j]
        table.append((r0, n, k, ns, R, o0, seeds[b]))
        parts.append(scores[b])
        r0 += n
        o0 += n - ns
    packed = torch.cat(parts)
    out = torch.full((o0 + 5,), -7, dtype=torch.int64, device=DEV)
    need = ops.select_rows_many_ws_bytes(table)
    ws = torch.full((need,), 255, dtype=torch.uint8, device=DEV) if poison else None
    views = ops.select_rows_many(packed, table, tick=tick, merge_first=merge_first, out=out, ws=ws)
    torch.cuda.synchronize()
    written = torch.zeros(out.numel(), dtype=torch.bool, device=DEV)
    for _, n, _, ns, _, o, _ in table:
        written[o:o + n - ns] = True
    assert bool((out[~written] == -7).all()), "a write outside the bags' output ranges"
    return {b: v for b, v in zip(order, views)}


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("merge_first", [False, True])
def test_one_call_over_all_kpt_classes(merge_first):
    """Ten bags, N = 1 .. 16384 over the three keys-per-thread classes and their edges, each with its own k, n_sel, merge_R and seed, a
    nonzero tick: every bag of the ONE call (one launch on the largest class, LDS sized for k = 4096) equals ops.select_rows on its slice."""
    scores, seeds, ref = _class_case()
    got = _call(scores, CLASSES, seeds, list(range(len(CLASSES))), [0] * len(CLASSES), _tick(), merge_first)
    for b, (n, k, ns, R) in enumerate(CLASSES):
        assert got[b].numel() == n - ns and torch.equal(got[b], ref[merge_first][b]), (b, n, k, ns, R)


# ------------------------------------------------------------------------------------------------------------------ 2
def test_a_bag_alone_reversed_order_gaps_and_odd_offsets():
    """The same bags each alone in a call (its own class, its own LDS size), and all of them in reversed order with gaps and odd row0 /
    out0: the same bits per bag - a bag's result depends on neither its place, its neighbours, the launch's class nor the LDS size."""
    scores, seeds, ref = _class_case()
    for b in range(len(CLASSES)):
        got = _call(scores, CLASSES, seeds, [b], [2 * b + 1], _tick(), True)
        assert torch.equal(got[b], ref[True][b]), ("alone", b, CLASSES[b])
    order = list(range(len(CLASSES)))[::-1]
    got = _call(scores, CLASSES, seeds, order, [3 + 2 * j for j in range(len(order))], _tick(), False, poison=False)
    for b in order:
        assert torch.equal(got[b], ref[False][b]), ("reversed", b, CLASSES[b])


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("kind", ["q4", "equal"])
def test_tie_heavy_scores(kind):
    """Scores quantised to four levels, and all-equal scores: the tie contract (value descending, then lowest index) of the per-bag call."""
    counts = [(33, 7, 4, 10), (257, 100, 50, 60), (4097, 300, 150, 1000), (10241, 2000, 2000, 0), (16384, 4096, 1000, 15384)]
    scores = [_scores(kind, n, 300 + j) for j, (n, *_) in enumerate(counts)]
    seeds = [7 + 1000003 * j for j in range(len(counts))]
    tick = _tick(5)
    got = _call(scores, counts, seeds, list(range(len(counts))), [1] * len(counts), tick, True)
    for b, (n, k, ns, R) in enumerate(counts):
        assert torch.equal(got[b], _ref_rows(scores[b], k, ns, R, seeds[b], tick, True)), (kind, b, n, k, ns, R)


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("merge_first", [False, True])
def test_a_large_bag_between_two_small_ones(merge_first):
    """A 16 385-row bag between two small ones: the small ones equal ops.select_rows, the large one the per-bag sequence random_perm,
    select_mask, random_perm (and the [merge | stay] swap) with the same seed."""
    counts = [(257, 16, 8, 25), (16385, 984, 492, 1590), (2100, 126, 63, 204)]
    scores = [_scores("rand", n, 400 + j) for j, (n, *_) in enumerate(counts)]
    seeds = [0xABCDEF0123456789, 0x0F1E2D3C4B5A6978, 99]
    tick = _tick(77)
    got = _call(scores, counts, seeds, [0, 1, 2], [0, 7, 1], tick, merge_first)
    for b, (n, k, ns, R) in enumerate(counts):
        assert torch.equal(got[b], _ref_rows(scores[b], k, ns, R, seeds[b], tick, merge_first)), (b, n)


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("merge_first", [False, True])
def test_set_properties_on_tie_free_scores(merge_first):
    """Without reference to another call: each list is [stay ascending | merge ascending] (merge_first: the groups swapped), the groups are
    disjoint and of the right lengths, the rows left out are n_sel of torch.topk's k."""
    counts = [(33, 7, 4, 10), (1024, 62, 31, 99), (4097, 246, 123, 397), (16384, 983, 492, 1589)]
    scores = [_scores("free", n, 500 + j) for j, (n, *_) in enumerate(counts)]
    got = _call(scores, counts, [11, 12, 13, 14], [0, 1, 2, 3], [0, 1, 0, 3], _tick(), merge_first)
    for b, (n, k, ns, R) in enumerate(counts):
        rows, Lk = got[b].cpu(), n - ns - R
        first, second = (rows[:R], rows[R:]) if merge_first else (rows[:Lk], rows[Lk:])
        assert rows.numel() == n - ns and first.numel() + second.numel() == rows.numel()
        for grp in (first, second):
            assert bool((grp[1:] > grp[:-1]).all()) and int(grp.min()) >= 0 and int(grp.max()) < n
        assert torch.unique(rows).numel() == rows.numel()
        masked = set(range(n)) - set(rows.tolist())
        assert len(masked) == ns and masked <= set(torch.topk(scores[b], k).indices.tolist())


# ------------------------------------------------------------------------------------------------------------------ 6
def test_a_captured_call_replays_the_eager_result():
    """The call inside a captured graph (the table travels by value; nothing is copied, waited for or allocated by the call), replayed
    twice: the eager result; with the device tick moved between the replays, the eager result at the new tick."""
    from mhim_mil_amd import ops
    counts = [(257, 16, 8, 25), (4097, 246, 123, 397), (16384, 983, 492, 1589), (97, 6, 3, 10)]
    scores = [_scores("rand", n, 600 + j) for j, (n, *_) in enumerate(counts)]
    seeds = [21, 22, 23, 24]
    table, r0, o0 = [], 0, 0
    for (n, k, ns, R), sd in zip(counts, seeds):
        table.append((r0, n, k, ns, R, o0, sd))
        r0, o0 = r0 + n, o0 + n - ns
    packed = torch.cat(scores)
    tick = _tick(9)
    out = torch.full((o0,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((ops.select_rows_many_ws_bytes(table),), 255, dtype=torch.uint8, device=DEV)
    eager = [v.clone() for v in ops.select_rows_many(packed, table, tick=tick, merge_first=True, out=out, ws=ws)]      # (also the warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        views = ops.select_rows_many(packed, table, tick=tick, merge_first=True, out=out, ws=ws)
    for rep in range(2):
        out.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for v, e in zip(views, eager):
            assert torch.equal(v, e), rep
    tick.add_(1)
    g.replay()
    torch.cuda.synchronize()
    for v, (n, k, ns, R), s, sd in zip(views, counts, scores, seeds):
        assert torch.equal(v, _ref_rows(s, k, ns, R, sd, tick, True))
    assert any(not torch.equal(v, e) for v, e in zip(views, eager)), "the replay did not read the device tick"


# ------------------------------------------------------------------------------------------------------------------ 7
def _twins(**cfg):
    from mhim_mil_amd.mhim import MHIM
    torch.manual_seed(31)
    ms = [MHIM(input_dim=256, n_classes=2, baseline="attn", **dict(V2, **cfg)).to(DEV).train() for _ in range(2)]
    tick = _tick(3)
    for m in ms:
        m._tick = tick
    assert ms[0]._step == ms[1]._step
    return ms


def _same_lists(a, b):
    assert len(a) == len(b)
    for (ra, *ca), (rb, *cb) in zip(a, b):
        assert ca == cb and torch.equal(ra, rb)


@pytest.mark.parametrize("merge_first", [False, True])
def test_student_rows_many_equals_the_loop(merge_first, monkeypatch):
    """MHIM.student_rows_many against a loop of student_rows on a twin model with the same seed: the same rows and counts, the same seed
    stream position afterwards - from per-bag vectors and from one packed vector with offsets, a bag above 16 384 rows among them - through
    ONE ops.select_rows_many."""
    from mhim_mil_amd import ops
    sizes = (64, 257, 16385, 2100)
    attns = [_scores("rand", n, 700 + j) for j, n in enumerate(sizes)]
    a, b = _twins()
    calls = []
    real = ops.select_rows_many
    monkeypatch.setattr(ops, "select_rows_many", lambda *x, **kw: (calls.append(1), real(*x, **kw))[1])
    many = a.student_rows_many(attns, merge_first=merge_first)
    loop = [b.student_rows(n, None, s, merge_first=merge_first) for n, s in zip(sizes, attns)]
    torch.cuda.synchronize()
    _same_lists(many, loop)
    assert a._step == b._step and a._next_seed() == b._next_seed() and len(calls) == 1
    offsets = [5]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    packed = torch.cat([torch.full((5,), 2.0, device=DEV)] + attns)
    many = a.student_rows_many(packed, offsets=offsets, merge_first=merge_first)
    loop = [b.student_rows(n, None, s, merge_first=merge_first) for n, s in zip(sizes, attns)]
    torch.cuda.synchronize()
    _same_lists(many, loop)
    assert a._step == b._step and len(calls) == 2


def test_student_rows_many_outside_the_production_condition(monkeypatch):
    """A v1 recipe (a low-attention mask ratio: the number of masked rows is data dependent) is not the production condition: the same
    rows and seed position through the per-bag fallback, and no many-select call."""
    from mhim_mil_amd import ops
    sizes = (300, 1000)
    attns = [_scores("rand", n, 800 + j) for j, n in enumerate(sizes)]
    a, b = _twins(mask_ratio_l=0.1)
    assert a.v2_counts(300) is None
    monkeypatch.setattr(ops, "select_rows_many", lambda *x, **kw: pytest.fail("the fallback must not call select_rows_many"))
    many = a.student_rows_many(attns, merge_first=True)
    loop = [b.student_rows(n, None, s, merge_first=True) for n, s in zip(sizes, attns)]
    torch.cuda.synchronize()
    _same_lists(many, loop)
    assert a._step == b._step and a._next_seed() == b._next_seed()


# ------------------------------------------------------------------------------------------------------------------ 8
def _trainer(accum):
    """student + spread teacher from the seeded synthetic state, in train mode, under FusedTrainer(accumulation_steps=accum)"""
    from mhim_mil_amd import synth
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    torch.manual_seed(5)
    base = synth.mhim_state(7, input_dim=D, merge_k=5)

    def mk(sd):
        m = MHIM(input_dim=D, n_classes=2, baseline="attn", **V2)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in dict(sd, **{"merge.global_q": sd["merge.global_q_mm"]}).items()})
        m = m.to(DEV).train()
        m.merge.dropout = 0.0
        return m
    return FusedTrainer(mk(base), mk(synth.spread_teacher(base)), aux_alpha=0.5, mm=0.9997, accumulation_steps=accum)


@pytest.mark.parametrize("sizes", [(64, 257, 2100, 97), (64, 16385, 97)], ids=["small", "with_16385"])
def test_ragged_window_rows(sizes):
    """mhimx_ragged_window_run makes every bag's row list in one many-select behind its teacher half: each bag's rows equal the per-bag
    call (ops.select_rows, or the large sequence) on that bag's own score with its seed and the call's tick, and two runs from the same
    state leave the same bits (row lists, logits, losses, the window's gradient)."""
    from mhim_mil_amd import synth
    xs = [torch.from_numpy(synth.bag(900 + j, n, D)).to(DEV)[None] for j, n in enumerate(sizes)]
    ls = [torch.tensor([j % 2], device=DEV) for j in range(len(sizes))]
    runs = []
    for _ in range(2):
        tr = _trainer(len(sizes))
        tr.window_step(xs, ls, update=False)
        torch.cuda.synchronize()
        assert tr.last["exec"] == ROUTE
        per, table = tr.last["bags"], tr.last["table"]
        runs.append(([p["rows"].clone() for p in per], [p["logits"].clone() for p in per], [p["losses"].clone() for p in per], tr.flat.grad.clone()))
    for j, n in enumerate(sizes):
        cnt, seed = table[j].cnt, int(table[j].seeds.select)
        ref = _ref_rows(per[j]["score"], cnt.k_top, cnt.n_sel, cnt.R, seed, tr.tick, True)
        torch.cuda.synchronize()
        assert per[j]["rows"].numel() == n - cnt.n_sel and torch.equal(per[j]["rows"], ref), f"rows of bag {j} ({n} rows)"
    for x, y in zip(runs[0], runs[1]):
        if torch.is_tensor(x):
            assert torch.equal(x, y)
        else:
            assert all(torch.equal(p, q) for p, q in zip(x, y))
