"""Which route a single bag takes, pinned case by case without a GPU: for every trainer (both kinds, the plain and the gated ABMIL, the
TransMIL and the DSMIL student, cross entropy and - where the constructor takes it - the survival loss, accumulation_steps 1 and 3), every
entry point of ENTRIES and every case of the grid below, the ordered list of the calls that ran with their keywords - a family's run,
_exec_step, _forward_backward_nat, _forward_backward_py, update, ops.step_run_many, the train_step calls of run_steps' fallback, the
warm-up of shape_cached - and how the entry point ended, or the exception's type and message.  The expected outcomes were recorded from
the commit before FusedTrainer got _step_route and sit in tests/golden/step_routes.json, deduplicated and run-length encoded, one row per
(entry point, trainer) in the grid's order (``python -m tests.test_step_routes_cpu --record`` writes them): an outcome that differs is a
change of behaviour, with the exceptions that _became() states.

The models are real CPU models and _nat_ok, _exec_ok and _step_counts_ok the real ones; the bags are fakes that expose what the routing
reads.  The four family checks are stubs with the real checks' front (False for a trainer of another family's model), else they take the
bag in the form ``take``; they decide and are not recorded - a check draws no seed and touches no counter, so asking one more often is no
change of behaviour, and what a check was offered shows in what its run received.  A single bag is only ever offered widened, so
``take="half"`` is a refusal like ``"nothing"``."""
import itertools
import json
import os
import types

import pytest
import torch

from mhim_mil_amd import _lib as L
from mhim_mil_amd import ops
from tests.test_window_families_cpu import FAMILIES, V2

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "step_routes.json")
D = 256
STUDENTS = {"abmil": ("attn", False), "gated": ("attn", True), "transmil": ("selfattn", False), "dsmil": ("dsmil", False)}
TRAINERS = [(kind, student, loss, accum) for kind in ("mhim", "mhim_pure") for student in STUDENTS for loss in ("ce", "nll_surv")
            for accum in (1, 3) if loss == "ce" or student == "abmil"]          # (the constructor: the plain ABMIL student only)
ENTRIES = ("forward_backward", "train_step", "run_steps_1", "run_steps_3", "shape_cached/forward_backward", "shape_cached/train_step",
           "_exec_ok")
# (shape_cached has no survival form - its key reads the shape of ONE label tensor, and the parent raised on a pair's or answered "not
# cached" -, so the survival trainers are not taken through the recording: test_shape_cached_does_not_cache_a_survival_trainer)
ROWS = [(entry,) + tr for entry in ENTRIES for tr in TRAINERS if not (entry.startswith("shape_cached") and tr[2] == "nll_surv")]
# two grids, each a full product over its own axes with the other's at their first value.  The switches: the trainer's state, the mask
# ratio (v1: v2_counts is None), injected draws.  The bag: its rows, row pitch (D or D + 2 elements), address (16-byte aligned or off by
# 4), element type (fp32, or half as handed over), the label (an int64 tensor or a Python int) and the form the family's check takes.
SWITCHES = dict(micro=(0, 1), injected=(False, True), world=(1, 2), clip=(False, True), single_pass=(True, False), v1=(False, True),
                use_executor=(True, False), hook=(False, True))
BAG = dict(rows=(512, 63, 64, 16384, 16385), half=(False, True), int_label=(False, True), pitch=(D, D + 2),
           take=("wide", "half", "nothing"), off=(0, 4))
CASES = [dict(zip(list(SWITCHES) + list(BAG), vals)) for vals in
         list(itertools.product(*SWITCHES.values(), *[v[:1] for v in BAG.values()]))
         + list(itertools.product(*[v[:1] for v in SWITCHES.values()], *BAG.values()))]


class _Bag:
    """What the routing reads of a bag.  ``form``: "wide" (contiguous fp32: MHIM._check_x hands it back as it is), "f32" (fp32 with a
    padded pitch) or "raw" (half precision as the caller hands it over)."""
    is_cuda = True
    device = types.SimpleNamespace(index=0, type="cuda")

    def __init__(self, n, pitch=D, off=0, half=False):
        self.shape, self.pitch, self.ptr = (n, D), pitch, 0x7F0000000000 + off
        self.dtype = torch.float16 if half else torch.float32
        self.form = "raw" if half else "wide" if pitch == D else "f32"

    def stride(self, j=None):
        return (self.pitch, 1) if j is None else (self.pitch, 1)[j]

    def dim(self):
        return 2

    def data_ptr(self):
        return self.ptr

    def element_size(self):
        return 2 if self.dtype == torch.float16 else 4

    def numel(self):
        return self.shape[0] * D

    def widened(self):
        """MHIM._check_x: the bag itself when it is contiguous fp32, else a contiguous fp32 copy (at an aligned address of its own)."""
        return self if self.form == "wide" else _Bag(self.shape[0])


class _Hook:
    pass


def _build(kind, student, loss, accum):
    """A trainer of real CPU models; the routes' ends are recording stubs on the instance that keep the host's bookkeeping (_micro, last)."""
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    baseline, gated = STUDENTS[student]
    if kind == "mhim":
        s, t = [MHIM(input_dim=D, n_classes=2, baseline=baseline, gated=gated, **V2).train() for _ in range(2)]
    else:
        s, t = MHIM(input_dim=D, n_classes=2, baseline=baseline, gated=gated, act="gelu", da_act="relu", merge_enable=False, dropout=0.25).train(), None
    tr = FusedTrainer(s, t, model=kind, accumulation_steps=accum, **({"loss": loss} if loss != "ce" else {}))
    calls, cfg = [], {}
    s._check_x = lambda b: b.widened()
    tr._half_bags = lambda bags: None                                  # (a widened bag is no half bag)
    tr._surv_label = lambda label, dev: label

    def done(updated):
        tr._micro = 0 if updated else tr._micro + 1

    def last(x, name):
        tr.last = {"patch_num": x.shape[0], "keep_num": x.shape[0], "exec": name}
        return "logits", "losses"
    for fam, (fkind, fbase, takes_i) in FAMILIES.items():
        mine = (fkind, fbase) == (kind, baseline)

        def ok(xs, labels, i=None, mine=mine):
            return bool(xs) and mine and xs[0].form == cfg["take"]

        def run(xs, labels, *a, fam=fam, takes_i=takes_i, **kw):
            assert len(a) == 1 + takes_i                               # ([i,] update)
            pairs = "pairs" if isinstance(labels[0], tuple) else "labels"
            calls.append(f"run:{fam}:{','.join(x.form for x in xs)}:{pairs}:update={a[-1]}:{','.join(f'{n}={bool(v)}' for n, v in sorted(kw.items()))}")
            done(a[-1] and not tr.clip_grad)
            last(xs[0], fam)
            return [["logits"] * len(xs), ["losses"] * len(xs)]
        setattr(tr, f"_{fam}_window_ok", ok)
        setattr(tr, f"_exec_{fam}_window", run)

    def exec_step(x, label, i):
        calls.append(f"exec:{x.form}:update={bool(tr._fold_now)}")
        done(bool(tr._fold_now))
        return last(x, True)

    def orchestration(name):
        def step(x, label, perm, ids_shuffle, i):
            calls.append(f"{name}:{x.form}:fold={bool(tr._fold_now)}:draws={perm},{ids_shuffle}")
            done(False)
            return last(x, False)
        return step
    tr._exec_step, tr._forward_backward_nat, tr._forward_backward_py = exec_step, orchestration("nat"), orchestration("py")
    tr.update = lambda: calls.append("update") or done(True)
    # behind run_steps' decision: the label check passes tensors on, the plan and the workspace are names, the chunk call is recorded
    tr._exec_cfg = lambda: {"cfg": "cfg"}
    tr._exec_plan = lambda ex, N, i: (None if kind == "mhim_pure" else "cnt", types.SimpleNamespace(total=N))
    tr._step_seeds = lambda: "seeds"
    tr._last_step = lambda ws, lay, N, cnt: {"logits": "logits", "losses": "losses"}
    tr._capture_stream = lambda: "capture stream"
    tr._warm_up = lambda cs, fn, n=1: calls.append("warm_up") or fn()
    tr._record = lambda cs, fn, **kw: calls.append("record") or ("graph", fn())
    return tr, calls, cfg


def _check_label(label, dev, message, nonempty=False):
    if not torch.is_tensor(label):
        raise L.MhimxError(message)


def _outcome(tr, calls, cfg, entry, case, monkeypatch):
    del calls[:]
    cfg.update(case)
    s, t = tr.s, tr.t
    monkeypatch.setattr(ops, "KERNEL_EVENT_HOOK", _Hook() if case["hook"] else None)
    tr.use_executor, tr.single_pass, tr.clip_grad = case["use_executor"], case["single_pass"], 1.0 if case["clip"] else None
    tr._micro, tr.world, tr.last, tr._capturing, tr._fold_now = case["micro"], case["world"], {}, False, False
    tr.flat.step, tr._shape_graphs = 0, None
    for m in (s, t):
        if m is not None:
            m.mask_ratio = 0.3 if case["v1"] else 0
    surv = tr.loss == "nll_surv"
    bag = _Bag(case["rows"], case["pitch"], case["off"], case["half"])
    label = ("Y", "c") if surv else 1 if case["int_label"] else torch.ones(1, dtype=torch.int64)
    draws = {"perm": "perm", "ids_shuffle": "shuffle"} if case["injected"] else {}
    try:
        if entry in ("forward_backward", "train_step"):
            end = f"returned:{getattr(tr, entry)(bag, label, i=5, **draws)}"
        elif entry.startswith("run_steps"):
            # (three bags: the middle one has too few rows for the executor, whatever the case's bag is)
            bags = [bag] if entry == "run_steps_1" else [bag, _Bag(32), bag]
            tr.train_step = lambda b, l, i=None: calls.append(f"train_step:{b.form}:{b.shape[0]}:i={i}") or ("logits", "losses")
            try:
                end = f"returned:{tr.run_steps(bags, [label] * len(bags), i=5)}"
            finally:
                del tr.train_step
        elif entry.startswith("shape_cached"):
            out = tr.shape_cached(entry.split("/")[1], bag, label, i=5)
            end = "not cached" if out is None else f"returned:{out}"
        else:
            end = str(tr._exec_ok(bag, 5, draws.get("perm"), draws.get("ids_shuffle")))
    except (AssertionError, AttributeError, TypeError, KeyError, L.MhimxError) as exc:
        end = f"{type(exc).__name__}:{exc}"
    assert tr._capturing is False
    return " | ".join(calls + [end, f"micro={tr._micro}"])


def _run(entry, kind, student, loss, accum, monkeypatch):
    tr, calls, cfg = _build(kind, student, loss, accum)
    monkeypatch.setattr(ops, "check_label", _check_label)
    monkeypatch.setattr(ops, "workspace", lambda *a, **kw: "ws")
    monkeypatch.setattr(ops, "step_run_many", lambda c, xs, labels, cnts, seeds, host_step, ws: calls.append(
        f"step_run_many:{','.join(x.form for x in xs)}:cnts={cnts}:seeds={len(seeds)}:host_step={host_step}"))
    out = []
    for case in CASES:
        with monkeypatch.context() as mp:
            out.append(_outcome(tr, calls, cfg, entry, case, mp))
    return out


ATTRIBUTE_ERRORS = ("AttributeError:'_Attention' object has no attribute 'attention'", "AttributeError:'DSMIL' object has no attribute 'attention'")


def _became(entry, student, case, was):
    """What a recorded outcome is now, where it is not what it was.  _exec_ok used to read the plain ABMIL scorer of whatever student the
    'mhim' trainer had and raised for a gated ABMIL and a DSMIL one; it now answers False for them, and run_steps - which asked it before
    _nat_ok - takes the documented bag-by-bag train_step fallback.  It also asks _nat_ok itself now, so that no caller has to ask both in
    the right order: asked directly with single_pass off it used to say yes to a bag that no route would then hand to the executor."""
    if was.split(" | ")[0] in ATTRIBUTE_ERRORS:
        if entry == "_exec_ok":
            return f"False | micro={case['micro']}"
        form = "raw" if case["half"] else "wide" if case["pitch"] == D else "f32"
        bags = [(form, case["rows"], 5)] if entry == "run_steps_1" else [(form, case["rows"], 5), ("wide", 32, 6), (form, case["rows"], 7)]
        return " | ".join([f"train_step:{f}:{n}:i={i}" for f, n, i in bags] + ["returned:('logits', 'losses')", f"micro={case['micro']}"])
    if entry == "_exec_ok" and not case["single_pass"] and was.startswith("True"):
        return "False" + was[4:]
    return was


def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["switches"] == {n: list(v) for n, v in SWITCHES.items()} and g["bag"] == {n: list(v) for n, v in BAG.items()}, \
        "the golden file was recorded over another grid"
    return g


def _row(g, key):
    runs = g["rows"][key]
    return [g["outcomes"][o] for o, n in zip(runs[::2], runs[1::2]) for _ in range(n)]


@pytest.mark.parametrize("entry, kind, student, loss, accum", ROWS)
def test_every_bag_of_the_grid_takes_the_route_it_took_before(entry, kind, student, loss, accum, monkeypatch):
    was = _row(_golden(), f"{entry}/{kind}/{student}/{loss}/{accum}")
    want = [_became(entry, student, case, w) for case, w in zip(CASES, was)]
    got = _run(entry, kind, student, loss, accum, monkeypatch)
    assert len(got) == len(want) == len(CASES)
    diff = [(case, w, o) for case, w, o in zip(CASES, want, got) if w != o]
    assert not diff, f"{len(diff)} of {len(CASES)} cases changed; the first: " + "\n".join(f"{c}\n  want: {w}\n  now: {o}" for c, w, o in diff[:5])
    # the stated exceptions are the AttributeErrors of run_steps and _exec_ok under a gated ABMIL or a DSMIL student of the 'mhim'
    # trainer, and _exec_ok's own answer with single_pass off: nothing else differs from the recording
    changed = [(case, w) for case, w, o in zip(CASES, was, got) if w != o]
    for case, w in changed:
        raised = w.split(" | ")[0] in ATTRIBUTE_ERRORS
        assert raised and entry in ("run_steps_1", "run_steps_3", "_exec_ok") and kind == "mhim" and student in ("gated", "dsmil") or \
            entry == "_exec_ok" and not case["single_pass"] and w.startswith("True"), (case, w)
    assert not any("AttributeError" in o for o in got if "'attention'" in o)


def test_the_recorded_attribute_errors_are_where_the_issue_found_them():
    """The recording holds the parent's AttributeErrors: under run_steps and _exec_ok, a gated ABMIL or a DSMIL student, model='mhim'."""
    g = _golden()
    hit = {tuple(key.rsplit("/", 4)[:3]) for key in g["rows"] if any(o.split(" | ")[0] in ATTRIBUTE_ERRORS for o in set(_row(g, key)))}
    assert hit == {(entry, "mhim", student) for entry in ("run_steps_1", "run_steps_3", "_exec_ok") for student in ("gated", "dsmil")}, hit


def test_the_grid_reaches_every_route():
    """The recorded outcomes are no vacuous table: every family's run, the executor, both orchestrations, the chunk call, run_steps'
    fallback, shape_cached's nat form (the step runs as it is), its auto form (the step runs in a warm-up on the capture stream) and its
    "not cached" answer are among them."""
    g = _golden()
    text = "\n".join(g["outcomes"])
    for piece in [f"run:{fam}:" for fam in FAMILIES] + ["exec:", "nat:", "py:", "step_run_many:", "train_step:", "update", "not cached",
                                                         "surv=True", "draws=perm,shuffle", "MhimxError:run_steps"]:
        assert piece in text, piece
    cached = "\n".join(o for key in g["rows"] if key.startswith("shape_cached") for o in set(_row(g, key)))
    for piece in ["warm_up | py:", "warm_up | run:dsmil:", "run:dsmil_mhim:", "exec:", "nat:", "not cached"]:
        assert piece in cached, piece
    assert any(o.startswith(("exec:", "nat:", "run:dsmil_mhim:")) for o in cached.split("\n"))          # (the nat form: no warm-up in front)


@pytest.mark.parametrize("kind", ["mhim", "mhim_pure"])
@pytest.mark.parametrize("what", ["forward_backward", "train_step"])
def test_shape_cached_does_not_cache_a_survival_trainer(what, kind, monkeypatch):
    """Every case of the grid: "not cached" (run it eagerly), nothing called, no error from the label pair."""
    tr, calls, cfg = _build(kind, "abmil", "nll_surv", 1)
    for case in CASES:
        with monkeypatch.context() as mp:
            assert _outcome(tr, calls, cfg, f"shape_cached/{what}", case, mp) == f"not cached | micro={case['micro']}", case


@pytest.mark.parametrize("kind, student, loss, accum", TRAINERS)
def test_exec_ok_answers_for_itself(kind, student, loss, accum, monkeypatch):
    """_exec_ok never raises and never says yes to a bag _nat_ok refuses, for every model the constructor accepts."""
    tr, calls, cfg = _build(kind, student, loss, accum)
    for case in CASES:
        with monkeypatch.context() as mp:
            _outcome(tr, calls, cfg, "_exec_ok", case, mp)               # (sets the trainer up for the case)
            bag = _Bag(case["rows"], case["pitch"], case["off"], case["half"])
            for window in (False, True):
                assert not tr._exec_ok(bag, 5, window=window) or tr._nat_ok(bag, 5), case


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["--record"]
    mp = pytest.MonkeyPatch()
    outcomes, rows = {}, {}
    for entry, kind, student, loss, accum in ROWS:
        ids = [outcomes.setdefault(o, len(outcomes)) for o in _run(entry, kind, student, loss, accum, mp)]
        rows[f"{entry}/{kind}/{student}/{loss}/{accum}"] = [v for o, grp in itertools.groupby(ids) for v in (o, len(list(grp)))]
    mp.undo()
    with open(GOLDEN, "w") as f:
        json.dump({"switches": {n: list(v) for n, v in SWITCHES.items()}, "bag": {n: list(v) for n, v in BAG.items()},
                   "outcomes": list(outcomes), "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(len(outcomes), "outcomes,", len(CASES) * len(rows), "cases,", sum(len(r) for r in rows.values()) // 2, "runs")
