"""Which route a window takes, pinned case by case without a GPU: for every trainer (the four families' models, cross entropy and - where
the constructor takes it - the survival loss, accumulation_steps 1 and 3) and every window of the grid below, the ordered list of family
checks window_step offers the bags to (with the bags' form), the run that took the window with its keywords, or the assertion that fired;
and whether capture_window refuses the same window (and with which message) or goes on to capture.  The expected outcomes were recorded
from the commit before FusedTrainer got its one route decision and sit in tests/golden/window_routes.json, one entry per case in the
grid's order (``python -m tests.test_window_routes_cpu --record`` writes them): an outcome that differs is a change of behaviour.

The fakes and the trainer with recording stubs are tests/test_window_families_cpu.py's.  The family checks here are stubs with the real
checks' front (_family_ok): False for an empty window and for a trainer of another family's model; else they take the bags in the form
``take`` ("half", "wide" or neither)."""
import itertools
import json
import os

import pytest
import torch

from mhim_mil_amd import _lib as L
from tests.test_window_families_cpu import FAMILIES, _FakeBag, _trainer

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "window_routes.json")
TRAINERS = [(name, loss, accum) for name in FAMILIES for loss in ("ce", "nll_surv") for accum in (1, 3)
            if loss == "ce" or FAMILIES[name][1] == "attn"]                    # (the constructor: the ABMIL student only)
# short: one bag fewer than accumulation_steps; same: bags of one shape; half: fp16 / bf16 bags as handed over (else fp32); world 2: set on
# the trainer (no process group; a survival trainer is one process by its constructor)
AXES = dict(short=(False, True), same=(False, True), half=(False, True), injected=(False, True), world=(1, 2), window_ok=(False, True),
            exec_window_ok=(False, True), take=("half", "wide", "nothing"), update=(True, False))


class _StreamForm(Exception):
    """Raised by the stub of _nat_prep: the window reached the stream form."""


class _WentOn(Exception):
    """Raised by the stub of torch.cuda.Stream: capture_window accepted the window."""


def _cases(loss, capture):
    axes = dict(AXES)
    if loss == "nll_surv":
        axes["world"] = (1,)
    if capture:
        axes["update"] = (True,)
    return [dict(zip(axes, vals)) for vals in itertools.product(*axes.values())]


def _build(name, loss, accum):
    """The families test's trainer; its stubs replaced by ones that read the case in ``cfg`` and write to ``calls``."""
    tr, calls = _trainer(name, accum, **({"loss": loss} if loss != "ce" else {}))
    cfg = {}
    for fam, (kind, baseline, takes_i) in FAMILIES.items():
        mine = (kind, baseline) == FAMILIES[name][:2]

        def ok(xs, labels, i=None, fam=fam, mine=mine):
            calls.append(f"ok:{fam}:{','.join(x.form for x in xs)}:{'pairs' if labels and isinstance(labels[0], tuple) else 'labels'}")
            return bool(xs) and mine and xs[0].form == cfg["take"]

        def run(xs, labels, *a, fam=fam, takes_i=takes_i, **kw):
            assert len(a) == 1 + takes_i                               # ([i,] update)
            calls.append(f"run:{fam}:{','.join(x.form for x in xs)}:update={a[-1]}:{','.join(sorted(kw))}")
            return [["logits"] * len(xs), ["losses"] * len(xs)]
        setattr(tr, f"_{fam}_window_ok", ok)
        setattr(tr, f"_exec_{fam}_window", run)

    def bag(what):
        def step(b, l, i=None, **kw):
            calls.append(f"{what}:{b.form}:{','.join(sorted(kw))}")
            tr.last = {"risk": torch.zeros(1)}
            return "logits", "losses"
        return step
    tr.train_step, tr.forward_backward = bag("train_step"), bag("forward_backward")
    tr.window_ok = lambda xs, i=None: cfg["window_ok"]
    tr._exec_window_ok = lambda xs, labels, i=None: cfg["exec_window_ok"]
    tr._exec_window = lambda xs, labels, i, update: calls.append(f"window_run:{','.join(x.form for x in xs)}:update={update}") or "window_run"

    def nat_prep(xs, i, **kw):
        calls.append(f"stream:{','.join(x.form for x in xs)}")
        raise _StreamForm()
    tr._nat_prep = nat_prep
    return tr, calls, cfg


def _window(case, accum, surv):
    k = accum - int(case["short"])
    form = "raw" if case["half"] else "f32"
    bags = [_FakeBag(n, form) for n in ((300, 300, 300) if case["same"] else (64, 257, 97))[:k]]
    labels = [("Y", "c") if surv else "label"] * k
    draws = {"perms": [None] * k, "shuffles": [None] * k} if case["injected"] else {}
    return bags, labels, draws


def _outcome(tr, calls, cfg, case, accum, surv, capture):
    del calls[:]
    cfg.update(case)
    tr.world, tr._micro, tr.last, tr._capturing = case["world"], 0, {}, False
    bags, labels, draws = _window(case, accum, surv)
    try:
        if capture:
            tr.capture_window(bags, labels, **draws)
            end = "returned"
        else:
            out = tr.window_step(bags, labels, update=case["update"], **draws)
            end = "returned:" + ("window_run" if out == "window_run" else f"{len(out[0])}")
    except _StreamForm:
        end = "stream form"
    except _WentOn:
        end = "went on to capture"
    except (AssertionError, IndexError, L.MhimxError) as exc:
        end = f"{type(exc).__name__}:{exc}"
    last = ",".join(n for n in ("bags", "risk") if n in tr.last)
    assert tr._capturing is False
    return end if capture else " | ".join(calls + [end, f"last={last}"])


def _run(name, loss, accum, capture, monkeypatch=None):
    tr, calls, cfg = _build(name, loss, accum)
    if capture:
        def stream(*a, **kw):
            raise _WentOn()
        if monkeypatch is not None:
            monkeypatch.setattr(torch.cuda, "Stream", stream)
        else:
            torch.cuda.Stream = stream
    return [_outcome(tr, calls, cfg, case, accum, loss == "nll_surv", capture) for case in _cases(loss, capture)]


def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["axes"] == {n: list(v) for n, v in AXES.items()}, "the golden file was recorded over another grid"
    return g


@pytest.mark.parametrize("capture", [False, True], ids=["window_step", "capture_window"])
@pytest.mark.parametrize("name, loss, accum", TRAINERS)
def test_every_window_of_the_grid_takes_the_route_it_took_before(name, loss, accum, capture, monkeypatch):
    g = _golden()
    want = [g["outcomes"][j] for j in g["rows"][f"{'capture_window' if capture else 'window_step'}/{name}/{loss}/{accum}"]]
    got = _run(name, loss, accum, capture, monkeypatch)
    cases = _cases(loss, capture)
    assert len(got) == len(want) == len(cases)
    diff = [(case, w, o) for case, w, o in zip(cases, want, got) if w != o]
    assert not diff, f"{len(diff)} of {len(cases)} cases changed; the first: " + "\n".join(f"{c}\n  was: {w}\n  now: {o}" for c, w, o in diff[:5])


def test_the_grid_reaches_every_route():
    """The recorded outcomes are no vacuous table: every family's run, mhimx_window_run, the stream form, all three bag-after-bag forms,
    both assertions and both of capture_window's ends are among them."""
    text = "\n".join(_golden()["outcomes"])
    for piece in [f"run:{fam}:" for fam in FAMILIES] + ["window_run:", "stream form", "train_step:", "forward_backward:", "last=bags,risk",
                                                          "at most accumulation_steps", "exactly accumulation_steps", ":surv", ":pairs",
                                                          "went on to capture", "MhimxError:capture_window"]:
        assert piece in text, piece


if __name__ == "__main__":
    import sys
    assert sys.argv[1:] == ["--record"]
    outcomes, rows = {}, {}
    for capture in (False, True):
        for name, loss, accum in TRAINERS:
            rows[f"{'capture_window' if capture else 'window_step'}/{name}/{loss}/{accum}"] = [
                outcomes.setdefault(o, len(outcomes)) for o in _run(name, loss, accum, capture)]
    with open(GOLDEN, "w") as f:
        json.dump({"axes": {n: list(v) for n, v in AXES.items()}, "outcomes": list(outcomes), "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    print(len(outcomes), "outcomes,", sum(len(r) for r in rows.values()), "cases")
