"""Which route a list of bags takes through MHIM.infer_cls_attn / MHIM.infer_cls_topk (the per-instance view of a TransMIL model), pinned
case by case without a GPU, the way tests/test_infer_routes_cpu.py pins infer_many / infer_topk: for every model of MODELS, every model
state of STATES and every case of the grid below, the ordered list of calls the model makes (ops.infer_transmil_many with its
configuration, the bags of the chunk and their dtypes, the sorted keywords and the size of the label slice; forward_test with the bag's
dtype and ``return_act``; _trans_score with its two shapes; ops.topk_many with its element count, segments, k and order - and, for
``by="heads"``, how many bytes its vector lies behind the first of the eight of its pack), how far ``_step`` moved, ``self.last``'s keys
with ``infer_native`` / ``infer_calls`` and the shapes of ``infer_attn`` / ``infer_topk``, whether ``infer_attn[0]`` IS the one native
call's own buffer, and the shapes, dtypes and arity of what came back - or the type and text of the error.

The expected outcomes were recorded on the parent commit - the one before the view became a family record of the one driver, where
``_infer_cls_run`` was a loop of its own - and sit in tests/golden/infer_cls_routes.json, one entry per case in the grid's order
(``python -m tests.test_infer_cls_routes_cpu --record`` writes them): 3 models x (525 cases in eval mode + 108 in each of the four states
that only switch the native route off) = 2 871 cases, 153 distinct outcomes.  An outcome that differs is a change of behaviour.

Bags, row cap and helpers are tests/test_infer_routes_cpu.py's.  The stub of forward_test draws three seeds and returns two maps of N
(merge_test: N + 5) columns, the stub of _trans_score draws one, as in tests/test_infer_transmil_attn_cpu.py."""
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
from tests import test_infer_routes_cpu as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "infer_cls_routes.json")
D, CC, ROWS, STATES, NAMES = R.D, R.CC, R.ROWS, R.STATES, R.NAMES
MODELS = {k: R.MODELS[k] for k in ("selfattn", "attn", "dsmil_cls")}               # (the last two: the refusal)
AXES = dict(bags=R.AXES["bags"], dtype=R.AXES["dtype"], labels=R.AXES["labels"],
            call=("cls", "cls:pseudo", "clstopk:pseudo", "clstopk:pseudo,smallest", "clstopk:heads,layer=1"))
# every state but eval only switches the native route off: those models see the corners of the grid
SMALL = dict(bags=R.SMALL["bags"], dtype=R.SMALL["dtype"], labels=AXES["labels"],
             call=("cls", "cls:pseudo", "clstopk:pseudo", "clstopk:heads,layer=1"))
assert AXES["bags"] == ("0", "1", "3", "33", "3/cap", "3/pitch", "3/3d") and AXES["dtype"] == ("f32", "f16", "bf16", "mixed", "f64")


def _cases(state):
    axes = AXES if state == "eval" else SMALL
    return [dict(zip(axes, vals)) for vals in itertools.product(*axes.values())]


def _build(model, state):
    """The model with its stubs -> (model, calls, the native call's buffers, the context that replaces the ops functions)."""
    torch.manual_seed(0)
    m = MHIM(n_classes=CC, input_dim=D, merge_enable=False, **({"prec": "f32"} if state == "f32" else {}), **MODELS[model])
    m.train(state == "train")
    m.merge_test = state == "merge_test"
    calls, own = [], []

    def forward_test(x, return_attn=False, no_norm=False, return_act=False, **kw):
        assert not kw and return_attn and not no_norm
        calls.append(f"forward_test:{NAMES[x.dtype]}:return_act={return_act}")
        for _ in range(3):
            m._next_seed()
        n = x.shape[0] + (5 if m.merge_test else 0)               # (merge_test scores N + k tokens)
        maps = [torch.full((1, 8, n), float(l + 1)) for l in range(2)]
        return torch.zeros(1, CC), ([maps, torch.zeros(1, 8, n, 64)] if return_act else maps)

    def trans_score(v, attn0):
        calls.append(f"_trans_score:v{list(v.shape)}:attn0{list(attn0.shape)}")
        m._next_seed()
        return torch.arange(v.shape[0], dtype=torch.float32)
    m.forward_test, m._trans_score = forward_test, trans_score

    def infer_transmil_many(cfg, xs, labels=None, **kw):
        assert labels is None or (labels.dtype == torch.int64 and labels.is_contiguous())
        calls.append(f"infer_transmil_many:{cfg};{len(xs)} bags {R._kinds(xs)};{','.join(f'{k}={v}' for k, v in sorted(kw.items()))}"
                     f";labels={None if labels is None else labels.numel()}")
        offs = [0] + list(itertools.accumulate(int(x.shape[0]) for x in xs))
        rows = offs[-1]
        r = types.SimpleNamespace(logits=torch.zeros(len(xs), CC), loss=None if labels is None else torch.zeros(len(xs)), offsets=offs,
                                  attn=torch.arange(16 * rows, dtype=torch.float32).view(2, 8, rows) if kw.get("want_attn") or kw.get("want_pscore") else None,
                                  pscore=torch.arange(rows, dtype=torch.float32) if kw.get("want_pscore") else None)
        own.append(r.attn)
        return r

    def topk_many(score, offsets, k, largest=True):
        calls.append(("topk_many", score.data_ptr(), f"topk_many:{score.numel()} of {NAMES[score.dtype]}:{len(offsets) - 1} segments:k={k}:largest={largest}"))
        return torch.zeros(len(offsets) - 1, k, dtype=torch.int64), torch.zeros(len(offsets) - 1, k)

    stubs = dict(infer_transmil_many=infer_transmil_many, topk_many=topk_many, infer_transmil_cfg=lambda D_, Cc, act, params, layers: "transmil_cfg",
                 infer_many=None, infer_dsmil_many=None, infer_params=lambda *ts: L.StepParams(), infer_dsmil_cfg=lambda *a: "dsmil_cfg")
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
    return m, calls, own, patched


def _cycle(items):
    """A list that repeats its head is written as the count and the head."""
    for p in range(1, len(items)):
        if items == (items[:p] * len(items))[:len(items)]:
            return f"{len(items)} cycling {','.join(items[:p])}"
    return ",".join(items)


def _shape(v):
    if v is None:
        return "None"
    if torch.is_tensor(v):
        return f"{NAMES.get(v.dtype, str(v.dtype).replace('torch.', ''))}{list(v.shape)}"
    if isinstance(v, list) and v and all(isinstance(t, int) for t in v):          # the offsets: how many, the first and the last
        return f"offsets[{len(v)}:{v[0]}..{v[-1]}]"
    if isinstance(v, list):
        return f"list[{_cycle([_shape(t) for t in v])}]"
    return f"{type(v).__name__}[{','.join(_shape(t) for t in v)}]"


def _written(calls, heads):
    """The recorded calls as text; the eight ops.topk_many calls of one pack of a ``by="heads"`` ranking with the bytes between their
    vector and the first of the eight."""
    out, first, seen = [], None, 0
    for c in calls:
        if isinstance(c, tuple):
            _, ptr, text = c
            if heads:
                first = ptr if seen % 8 == 0 else first
                text += f":+{ptr - first} bytes"
                seen += 1
            c = text
        out.append(c)
    return out


def _outcome(m, calls, own, case, cap):
    del calls[:], own[:]
    m._step, m.last = 1000, {"stale": True}
    m.__dict__.pop("infer_row_cap", None)
    if case["bags"] == "3/cap":
        m.infer_row_cap = cap
    xs = R._bags(case)
    n = len(xs)
    labels = None if case["labels"] == "none" else torch.arange(n + (case["labels"] == "wrong"), dtype=torch.int64) % CC
    what, _, opts = case["call"].partition(":")
    try:
        if what == "cls":
            out = m.infer_cls_attn(xs, labels=labels, pseudo=opts == "pseudo")
        elif opts.startswith("heads"):
            out = m.infer_cls_topk(xs, 2, by="heads", layer=1, labels=labels)
        else:
            out = m.infer_cls_topk(xs, 2, largest="smallest" not in opts, by="pseudo", labels=labels)
        end = "returned " + _shape(out)
    except (L.MhimxError, AssertionError, IndexError, RuntimeError, TypeError, AttributeError) as exc:
        end = f"{type(exc).__name__}:{exc}"
    last = ",".join(f"{k}={_shape(v) if k in ('infer_attn', 'infer_topk') else v}" for k, v in sorted(m.last.items()))
    packed = m.last.get("infer_attn")
    mine = "attn is the call's buffer:" + (str(packed[0].data_ptr() == own[0].data_ptr()) if packed is not None and len(own) == 1 else "n/a")
    text = _written(calls, opts.startswith("heads"))
    return [q for c in R._runs(text) for q in c.split(";")] + [end, f"step+{m._step - 1000}", f"last:{last}", mine]


def _run(model, state):
    m, calls, own, patched = _build(model, state)
    cap = R.row_cap_for(m, ROWS[0] + ROWS[1])
    with patched():
        return [_outcome(m, calls, own, case, cap) for case in _cases(state)]


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
    """The recorded outcomes are no vacuous table: the native call in one chunk and in two, with and without the pseudo-score, on half bags
    as they are; both loops; the three rankings on the call's buffers and on the loop's packs; the call's own buffer handed out; every
    refusal and every ``self.last`` form are among them."""
    text = "\n".join(" | ".join(o) for o in _golden()["outcomes"])
    for piece in ["infer_transmil_many:transmil_cfg | 3 bags 3xf16 | want_attn=True,want_pscore=False | labels=None",
                  "infer_transmil_many:transmil_cfg | 32 bags 32xbf16 | want_attn=True,want_pscore=True | labels=32",
                  "infer_transmil_many:transmil_cfg | 2 bags 2xf32 | ", "infer_transmil_many:transmil_cfg | 1 bags 1xf32 | ",
                  "forward_test:f32:return_act=True | _trans_score:v[64, 512]:attn0[8, 64]", "33 x forward_test:f32:return_act=False",
                  "topk_many:418 of f32:3 segments:k=2:largest=False", "topk_many:418 of f32:3 segments:k=2:largest=True:+11704 bytes",
                  "segments:k=2:largest=True:+0 bytes", "32 segments", "step+99", "step+9", "step+3", "step+0", "infer_native=True", "infer_native=False",
                  "infer_calls=2", "infer_attn=tuple[f32[2, 8, 418],f32[418],offsets[4:0..418]]", "infer_attn=tuple[f32[2, 8, 0],None,offsets[1:0..0]]",
                  "infer_topk=tuple[int64[3, 8, 2],f32[3, 8, 2]]", "infer_topk=tuple[int64[0, 2],f32[0, 2]]", "attn is the call's buffer:True",
                  "attn is the call's buffer:n/a", "4 labels for 3 bags", "infer_many(return_attn=True)",
                  "last:stale=True", "returned tuple[f32[33, 3],list[33 cycling f32[2, 8, 64],f32[2, 8, 257],f32[2, 8, 97]],None]",
                  "returned tuple[f32[0, 3],list[],list[]]"]:
        assert piece in text, piece


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
