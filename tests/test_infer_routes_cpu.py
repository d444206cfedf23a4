"""Which route a list of bags takes through MHIM.infer_many / MHIM.infer_topk, pinned case by case without a GPU: for every model of
MODELS, every model state of STATES and every case of the grid below, the ordered list of calls the model makes (ops.infer_many /
ops.infer_dsmil_many / ops.infer_transmil_many with the configuration they got, the bags of the chunk and their dtypes, the ``want_*``
keywords and the size of the label slice; ops.topk_many with its vector, segments, k and order; forward_test with the bag's dtype and its
keywords), how far ``_step`` moved, ``self.last``'s keys with ``infer_native`` / ``infer_calls`` and the shapes of ``infer_parts``, and
the shapes and types of what came back - or the type and text of the error.  The expected outcomes were recorded from the commit before
the three inference families got their one family record and one chunk loop and sit in tests/golden/infer_routes.json, one entry per case
in the grid's order (``python -m tests.test_infer_routes_cpu --record`` writes them): an outcome that differs is a change of behaviour.

The bags are shape-only fakes (tests/test_infer_dsmil_cpu.py's _FakeBag, with what _infer_bags and _infer_run read on top); the ops
calls, the configuration builders that want device tensors and forward_test are recording stubs that return small CPU tensors of the
right shapes.  The stub of forward_test draws the seeds the real one draws (1 per bag; TransMIL 3)."""
import contextlib
import itertools
import json
import os
import types

import pytest
import torch

from mhim_mil_amd import _lib as L
from mhim_mil_amd import ops
from mhim_mil_amd.mhim import MHIM

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "infer_routes.json")
FAKE = 0x7F0000000000            # 256-byte aligned, never dereferenced
D, CC = 256, 3
ROWS = (64, 257, 97)
MODELS = {"attn": dict(baseline="attn"), "attn_gated": dict(baseline="attn", gated=True), "dsmil_cls": dict(baseline="dsmil", attn2score=True),
          "dsmil_nocls": dict(baseline="dsmil", attn2score=False), "selfattn": dict(baseline="selfattn")}
STATES = ("eval", "train", "merge_test", "f32", "hook")
# bags: how many (3/cap: three bags under a row cap that takes two of them; 3/pitch: the middle bag's pitch is below D; 3/3d: [1, N, D])
AXES = dict(bags=("0", "1", "3", "33", "3/cap", "3/pitch", "3/3d"), dtype=("f32", "f16", "bf16", "mixed", "f64"),
            labels=("none", "given", "wrong"),
            call=("many", "many:attn", "many:no_norm", "many:attn,no_norm", "topk", "topk:no_norm", "topk:smallest"))
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}
NAMES = {v: k for k, v in DTYPES.items()}
# every state but eval only switches the native route off: those models see the corners of the grid
SMALL = dict(bags=("0", "3", "33"), dtype=("f32", "f16", "mixed"), labels=AXES["labels"], call=("many", "many:attn,no_norm", "topk"))


def _cases(state):
    axes = AXES if state == "eval" else SMALL
    return [dict(zip(axes, vals)) for vals in itertools.product(*axes.values())]


class _FakeBag:
    """Shape-only stand-in for a GPU bag: what _infer_bags, _infer_ok, infer_chunks and _infer_run read."""
    is_cuda = True

    def __init__(self, n, d, dtype=torch.float32, ptr=FAKE, pitch=None, dev=torch.device("cpu"), lead=False):
        self.shape, self.dtype, self.device, self._ptr, self._pitch = ((1, n, d) if lead else (n, d)), dtype, dev, ptr, pitch or d

    def dim(self):
        return len(self.shape)

    def __getitem__(self, j):
        assert j == 0 and self.dim() == 3
        return _FakeBag(self.shape[1], self.shape[2], self.dtype, self._ptr, self._pitch, self.device)

    def stride(self, k):
        assert self.dim() == 2
        return self._pitch if k == 0 else 1

    def data_ptr(self):
        return self._ptr

    def element_size(self):
        return {torch.float32: 4, torch.float64: 8}.get(self.dtype, 2)

    def float(self):                                             # (a fresh dense fp32 matrix, as x.float() of another dtype is)
        return self if self.dtype == torch.float32 else _FakeBag(*self.shape[-2:], torch.float32, FAKE + 0x1000, None, self.device, self.dim() == 3)

    def contiguous(self):
        return self


def _runs(items):
    """Equal neighbours as one ``n x item``."""
    return [f"{n} x {k}" if n > 1 else k for k, n in ((k, len(list(g))) for k, g in itertools.groupby(items))]


def _kinds(xs):
    return "+".join(f"{len(list(g))}x{k}" for k, g in itertools.groupby(NAMES[x.dtype] for x in xs))


def _lengths(ts):
    """The lengths of the per-bag vectors; a list that repeats its head is written as the head and the count."""
    ns = [t.numel() for t in ts]
    for p in range(1, len(ns)):
        if ns == (ns[:p] * len(ns))[:len(ns)] and p < len(ns):
            return f"{len(ns)} cycling {','.join(map(str, ns[:p]))}"
    return ",".join(map(str, ns))


def _build(model, state):
    """The model with its stubs -> (model, calls, the context that replaces the ops functions)."""
    torch.manual_seed(0)
    m = MHIM(n_classes=CC, input_dim=D, merge_enable=False, **({"prec": "f32"} if state == "f32" else {}), **MODELS[model])
    m.train(state == "train")
    m.merge_test = state == "merge_test"
    calls = []
    seeds = 3 if m.baseline == "selfattn" else 1

    def forward_test(x, return_attn=False, no_norm=False, **kw):
        assert not kw
        calls.append(f"forward_test:{NAMES[x.dtype]}:attn={return_attn}:no_norm={no_norm}")
        for _ in range(seeds):
            m._next_seed()
        n, lg = x.shape[0], torch.zeros(1, CC)
        if m.baseline == "dsmil":
            return ([lg, lg], torch.zeros(1, n)) if return_attn else ([lg, lg], torch.zeros(1, CC, 4))
        if not return_attn:
            return lg
        return (lg, [torch.zeros(1, 8, 2, 2)] * 2) if m.baseline == "selfattn" else (lg, torch.zeros(1, n))
    m.forward_test = forward_test

    def native(name, fields):
        def run(cfg, xs, labels=None, **kw):
            assert labels is None or (labels.dtype == torch.int64 and labels.is_contiguous())
            cfg = cfg if isinstance(cfg, str) else "InferCfg"
            calls.append(f"{name}:{cfg};{len(xs)} bags {_kinds(xs)};{','.join(f'{k}={v}' for k, v in sorted(kw.items()))}"
                         f";labels={None if labels is None else labels.numel()}")
            n = len(xs)
            r = types.SimpleNamespace(offsets=[0] + list(itertools.accumulate(int(x.shape[0]) for x in xs)))
            r.loss = None if labels is None else torch.zeros(n)
            for f, shape in fields.items():
                setattr(r, f, torch.zeros(*(n if s == "n" else s for s in shape)))
            for f, want in (("attn", "want_attn"), ("score", "want_score")):
                setattr(r, f, torch.zeros(r.offsets[-1]) if kw.get(want) else None)
            return r
        return run

    def topk_many(score, offsets, k, largest=True):
        calls.append(f"topk_many:{score.numel()} of {NAMES[score.dtype]}:{len(offsets) - 1} segments:k={k}:largest={largest}")
        return torch.zeros(len(offsets) - 1, k, dtype=torch.int64), torch.zeros(len(offsets) - 1, k)

    stubs = dict(infer_many=native("infer_many", {"logits": ("n", CC)}),
                 infer_dsmil_many=native("infer_dsmil_many", {f: ("n", CC) for f in ("logits", "logits_bag", "logits_ins")} | {"B": ("n", CC, 4)}),
                 infer_transmil_many=native("infer_transmil_many", {"logits": ("n", CC)}),
                 topk_many=topk_many, infer_params=lambda *ts: L.StepParams(),
                 infer_dsmil_cfg=lambda D_, E, Cc, act, cls_attn, no_norm, params: f"dsmil_cfg(cls_attn={bool(cls_attn)},no_norm={bool(no_norm)})",
                 infer_transmil_cfg=lambda D_, Cc, act, params, layers: "transmil_cfg")
    if state == "hook":
        stubs["KERNEL_EVENT_HOOK"] = lambda *a: None

    @contextlib.contextmanager
    def patched():
        saved = {n: getattr(ops, n) for n in stubs}
        for n, f in stubs.items():
            setattr(ops, n, f)
        try:
            yield
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
    return m, calls, patched


def row_cap_for(m, rows):
    """The smallest ``infer_row_cap`` under which one call of ``m`` takes ``rows`` rows."""
    saved, cap = m.__dict__.get("infer_row_cap"), 1
    try:
        while True:
            m.infer_row_cap = cap
            if m.infer_rows_per_call() >= rows:
                return cap
            cap += 1
    finally:
        m.__dict__.pop("infer_row_cap")
        if saved is not None:
            m.infer_row_cap = saved


def _bags(case):
    count = int(case["bags"].split("/")[0])
    form = case["bags"].partition("/")[2]
    kinds = ["f16", "f32"] if case["dtype"] == "mixed" else [case["dtype"]]
    return [_FakeBag(ROWS[j % 3], D, DTYPES[kinds[j % len(kinds)]], FAKE + 0x10000000 * j, 128 if form == "pitch" and j == 1 else None,
                     lead=form == "3d") for j in range(count)]


def _shape(v):
    if v is None:
        return "None"
    if torch.is_tensor(v):
        return f"{NAMES.get(v.dtype, str(v.dtype).replace('torch.', ''))}{list(v.shape)}"
    if v and all(torch.is_tensor(t) and t.dim() == 1 for t in v):                  # the per-bag vectors: their lengths
        return f"{type(v).__name__}[{_kinds(v)}:{_lengths(v)}]"
    return f"{type(v).__name__}[{','.join(_shape(t) for t in v)}]"


def _outcome(m, calls, case, cap):
    del calls[:]
    m._step, m.last = 1000, {"stale": True}
    m.__dict__.pop("infer_row_cap", None)
    if case["bags"] == "3/cap":
        m.infer_row_cap = cap
    xs = _bags(case)
    n = len(xs)
    labels = None if case["labels"] == "none" else torch.arange(n + (case["labels"] == "wrong"), dtype=torch.int64) % CC
    what, _, opts = case["call"].partition(":")
    try:
        if what == "many":
            out = m.infer_many(xs, labels=labels, return_attn="attn" in opts, no_norm="no_norm" in opts)
        else:
            out = m.infer_topk(xs, 2, largest=opts != "smallest", no_norm=opts == "no_norm", labels=labels)
        end = "returned " + _shape(out)
    except (L.MhimxError, AssertionError, IndexError, RuntimeError, TypeError, AttributeError) as exc:
        end = f"{type(exc).__name__}:{exc}"
    last = ",".join(f"{k}={_shape(v) if k in ('infer_parts', 'infer_topk') else v}" for k, v in sorted(m.last.items()))
    return [q for c in _runs(calls) for q in c.split(";")] + [end, f"step+{m._step - 1000}", f"last:{last}"]   # (a call: four pieces)


def _run(model, state):
    m, calls, patched = _build(model, state)
    cap = row_cap_for(m, ROWS[0] + ROWS[1])
    with patched():
        return [_outcome(m, calls, case, cap) for case in _cases(state)]


def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["axes"] == {n: list(v) for n, v in AXES.items()} and g["small"] == {n: list(v) for n, v in SMALL.items()}, \
        "the golden file was recorded over another grid"
    g["outcomes"] = [[g["pieces"][j] for j in o] for o in g["outcomes"]]         # (an outcome: its pieces in order)
    return g


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("model", MODELS)
def test_every_case_of_the_grid_takes_the_route_it_took_before(model, state):
    g = _golden()
    want = [g["outcomes"][j] for j in g["rows"][f"{model}/{state}"]]
    got = _run(model, state)
    cases = _cases(state)
    assert len(got) == len(want) == len(cases)
    diff = [(case, w, o) for case, w, o in zip(cases, want, got) if w != o]
    assert not diff, f"{len(diff)} of {len(cases)} cases changed; the first: " + "\n".join(f"{c}\n  was: {w}\n  now: {o}" for c, w, o in diff[:5])


def test_the_grid_reaches_every_route():
    """The recorded outcomes are no vacuous table: every native call (in one chunk and in two, widened and not), the top-k on the chunk's
    buffer and on the loop's packed vectors, both loops, every refusal and every ``self.last`` form are among them."""
    text = "\n".join(" | ".join(o) for o in _golden()["outcomes"])
    for piece in ["infer_many:InferCfg | 3 bags 3xf32 | ", "infer_many:InferCfg | 32 bags 32xf16 | ", "infer_many:InferCfg | 1 bags 1xbf16 | ",
                  "infer_many:InferCfg | 2 bags 2xf32 | want_attn=False,want_score=True | labels=2",
                  "infer_dsmil_many:dsmil_cfg(cls_attn=True,no_norm=False) | 3 bags", "infer_dsmil_many:dsmil_cfg(cls_attn=False,no_norm=True) | ",
                  "want_B=True,want_attn=True", "infer_transmil_many:transmil_cfg | 2 bags 2xf16 |  | labels=None", "step+99", "step+33", "step+0",
                  "topk_many:418 of f32:3 segments:k=2:largest=False", "forward_test:f32:attn=True:no_norm=True", "forward_test:f16",
                  "infer_native=True", "infer_native=False", "infer_calls=2", "infer_parts=tuple[f32[3, 3],f32[3, 3],None]", "infer_topk=",
                  "labels for 3 bags", "MhimxError:MHIM.infer_topk: merge_test", "MhimxError:MHIM.infer_topk: TransMIL", "last:stale=True",
                  "returned tuple[f32[33, 3],list[", "returned f32[0, 3]"]:
        assert piece in text, piece


def test_the_lowered_row_cap_takes_two_of_the_three_bags():
    for model in MODELS:
        m, _, _ = _build(model, "eval")
        m.infer_row_cap = row_cap_for(m, ROWS[0] + ROWS[1])
        assert ROWS[0] + ROWS[1] <= m.infer_rows_per_call() < sum(ROWS)
        assert m.infer_chunks(_bags(dict(bags="3", dtype="f32"))) == [(0, 2), (2, 3)]


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["--record"]
    pieces, outcomes, rows = {}, {}, {}
    for model in MODELS:
        for state in STATES:
            rows[f"{model}/{state}"] = [outcomes.setdefault(tuple(pieces.setdefault(p, len(pieces)) for p in o), len(outcomes))
                                        for o in _run(model, state)]
    one = lambda v: json.dumps(v, separators=(",", ":"))
    with open(GOLDEN, "w") as f:                              # one piece and one row per line: a change shows as the lines it touches
        f.write('{"axes":%s,\n"small":%s,\n"pieces":[\n%s],\n"outcomes":%s,\n"rows":{\n%s}}\n' % (
            one({n: list(v) for n, v in AXES.items()}), one({n: list(v) for n, v in SMALL.items()}), ",\n".join(one(p) for p in pieces),
            one([list(o) for o in outcomes]), ",\n".join(f"{one(k)}:{one(r)}" for k, r in rows.items())))
    print(len(pieces), "pieces,", len(outcomes), "outcomes,", sum(len(r) for r in rows.values()), "cases")
