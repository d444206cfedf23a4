"""The one dispatcher and the one runner behind the four ragged native train calls (pure, dsmil, dsmil_mhim, ragged) without a GPU:
forward_backward (accumulation_steps == 1), window_step with a full window and with a shorter last window reach the family's own
_<name>_window_ok / _exec_<name>_window - the ones set on the instance -, offer the bags as they are first (fp16 / bf16) and widened second,
and leave all four alone under injected draws; a window the layout call refuses leaves every seed stream and counter where it was.  The
checks and runs are stubs and the bags fakes: no device."""
import pytest
import torch

from mhim_mil_amd import _lib as L

V2 = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999,
          merge_ratio=0.9, temp_t=0.1, dropout=0.25)
# family -> (FusedTrainer's model, the student's baseline, its calls take ``i``)
FAMILIES = {"pure": ("mhim_pure", "attn", False), "dsmil": ("mhim_pure", "dsmil", False), "dsmil_mhim": ("mhim", "dsmil", True),
            "ragged": ("mhim", "attn", True)}


class _FakeBag:
    """What the routing reads of a bag: shape, strides, device; ``form``: "raw" (a half-precision bag as the caller hands it over), "half"
    (what _half_bags makes of it) or "wide" (what _check_x makes of it)."""
    device = "fake"

    def __init__(self, n, form="raw", d=256):
        self.shape, self._stride, self.form = (n, d), (d, 1), form

    def stride(self, j=None):
        return self._stride if j is None else self._stride[j]

    def dim(self):
        return 2

    def to(self, form):
        return _FakeBag(self.shape[0], form)


def _models(name):
    from mhim_mil_amd.mhim import MHIM
    kind, baseline, _ = FAMILIES[name]
    if kind == "mhim":
        return kind, [MHIM(input_dim=256, n_classes=2, baseline=baseline, **V2).train() for _ in range(2)]
    return kind, [MHIM(input_dim=256, n_classes=2, baseline=baseline, act="gelu", da_act="relu", merge_enable=False, dropout=0.25).train(), None]


def _trainer(name, accum, take="wide", **kw):
    """A trainer of the family's model whose four checks and four runs are recording stubs on the instance; the family's check takes the
    bags in the form ``take``."""
    from mhim_mil_amd.engine import FusedTrainer
    kind, (s, t) = _models(name)
    tr = FusedTrainer(s, t, model=kind, accumulation_steps=accum, **kw)
    s._check_x = lambda b: b.to("wide")
    tr._half_bags = lambda bags: [b.to("half") for b in bags] if all(b.form == "raw" for b in bags) else None
    tr._surv_label = lambda label, dev: label
    calls = []
    for fam, (_, _, takes_i) in FAMILIES.items():
        def ok(xs, labels, i=None, fam=fam):
            calls.append(("ok", fam, [x.form for x in xs]))
            return xs[0].form == take
        def run(xs, labels, *a, fam=fam, takes_i=takes_i, **kw):
            assert len(a) == 1 + takes_i                               # ([i,] update)
            calls.append(("run", fam, [x.form for x in xs], sorted(kw)))
            return [["logits"] * len(xs), ["losses"] * len(xs)]
        setattr(tr, f"_{fam}_window_ok", ok)
        setattr(tr, f"_exec_{fam}_window", run)
    tr.train_step = lambda b, l, i=None, **kw: calls.append(("bag", sorted(kw))) or (None, None)
    tr.window_ok = lambda xs, i=None: False
    tr._nat_ok = lambda x, i=None: True
    tr._exec_ok = lambda *a, **kw: False
    tr._forward_backward_nat = lambda x, label, perm, ids_shuffle, i: calls.append(("nat", x.form)) or (None, None)
    return tr, calls


@pytest.mark.parametrize("name", list(FAMILIES))
def test_forward_backward_offers_its_widened_bag_to_the_family_on_the_instance(name):
    """accumulation_steps == 1: the ABMIL families are reached by a survival bag (a cross-entropy bag keeps the step calls), the DSMIL
    families by every bag.  forward_backward widens its bag first, so the call sees the widened form alone; ``single=True`` asks for the
    single-bag bookkeeping."""
    surv = FAMILIES[name][1] == "attn"
    tr, calls = _trainer(name, 1, **({"loss": "nll_surv"} if surv else {}))
    label = ("Y", "c") if surv else "label"
    assert tr.forward_backward(_FakeBag(97), label) == ("logits", "losses")
    assert calls == [("ok", name, ["wide"]), ("run", name, ["wide"], ["single", "surv"] if surv else ["single"])], calls
    del calls[:]
    tr.forward_backward(_FakeBag(97), label, perm="perm", ids_shuffle="shuffle")             # injected draws: none of the four
    assert calls == [("nat", "wide")], calls


@pytest.mark.parametrize("k", [3, 2])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_window_step_offers_half_bags_first_and_widened_second_to_the_family_on_the_instance(name, k):
    """A full window (3 of accumulation_steps == 3 bags, of different sizes) and a shorter last window (2)."""
    bags, labels = [_FakeBag(n) for n in (64, 257, 97)][:k], [0, 1, 0][:k]
    tr, calls = _trainer(name, 3, take="wide")
    assert tr.window_step(bags, labels) == [["logits"] * k, ["losses"] * k]
    assert calls == [("ok", name, ["half"] * k), ("ok", name, ["wide"] * k), ("run", name, ["wide"] * k, [])], calls
    tr, calls = _trainer(name, 3, take="half")
    tr.window_step(bags, labels)
    assert calls == [("ok", name, ["half"] * k), ("run", name, ["half"] * k, [])], calls


@pytest.mark.parametrize("name", ["dsmil_mhim", "ragged"])
@pytest.mark.parametrize("sizes, perms", [((300, 300, 300), None), ((64, 257, 97), None), ((64, 257, 97), [None] * 3)])
def test_window_step_widens_every_bag_once_whatever_route_takes_the_window(name, sizes, perms):
    """A full window of same-shaped bags (not offered to the ragged call), a window the checks refuse and one with injected draws all fall
    through to the routes behind the native calls, which read the widened bags: _check_x ran once per bag."""
    tr, calls = _trainer(name, 3, take="nothing")
    widened, check_x = [], tr.s._check_x
    tr.s._check_x = lambda b: widened.append(b) or check_x(b)
    bags = [_FakeBag(n) for n in sizes]
    tr.window_step(bags, [0, 1, 0], perms=perms, shuffles=perms)
    assert widened == bags and calls[-3:] == [("bag", ["ids_shuffle", "perm"] if perms else [])] * 3, (widened, calls)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_injected_draws_bypass_all_four_families(name):
    tr, calls = _trainer(name, 3)
    tr.window_step([_FakeBag(n) for n in (64, 257, 97)], [0, 1, 0], perms=[None] * 3, shuffles=[None] * 3)
    assert calls == [("bag", ["ids_shuffle", "perm"])] * 3, calls


@pytest.mark.parametrize("name", list(FAMILIES))
def test_a_window_the_layout_call_refuses_leaves_seed_streams_and_counters_alone(name, monkeypatch):
    from mhim_mil_amd import engine as EN
    from mhim_mil_amd.engine import FusedTrainer
    kind, (s, t) = _models(name)
    tr = FusedTrainer(s, t, model=kind, accumulation_steps=3)
    seen = []

    def refuse(syms, cfg, bags, n, layout_only=True, *a, **kw):
        seen.append((syms.layout_of, layout_only))
        raise L.MhimxError(f"{syms.layout_of}: refused")
    monkeypatch.setattr(EN.ops, "_window_call", refuse)
    xs, labels = [torch.zeros(n, 256) for n in (64, 257)], [torch.zeros(1, dtype=torch.int64) for _ in range(2)]
    before = (s._step, None if t is None else t._step, tr.flat.step, tr._micro, int(tr.tick), int(tr.opt_step), dict(tr.last))
    with pytest.raises(L.MhimxError, match="layout_of: refused"):
        getattr(tr, f"_exec_{name}_window")(xs, labels, *((None,) if FAMILIES[name][2] else ()), True)
    assert seen == [(f"mhimx_{name}_window_layout_of", True)], seen
    assert (s._step, None if t is None else t._step, tr.flat.step, tr._micro, int(tr.tick), int(tr.opt_step), dict(tr.last)) == before
