"""run_steps on students the step executor does not take (FusedTrainer._step_route): the documented bag-by-bag fallback, on the device."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(mask_ratio_h=0.03, mask_ratio_hr=0.5, merge_enable=True, merge_k=5, merge_mm=0.9999, merge_ratio=0.9, act="gelu", da_act="relu",
           attn2score=True, temp_t=0.1, dropout=0.25)


def _trainer(student):
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    torch.manual_seed(11)
    kw = {"baseline": "attn", "gated": True} if student == "gated" else {"baseline": "dsmil"}
    s = MHIM(input_dim=256, n_classes=2, **kw, **CFG).cuda().train()
    t = copy.deepcopy(s).train()
    return FusedTrainer(s, t, lr=1e-3, mm=0.999, aux_alpha=0.5, model="mhim")


@pytest.mark.parametrize("student", ["gated", "dsmil"])
def test_run_steps_goes_bag_by_bag_where_the_executor_does_not_take_the_student(student):
    """ADVICE r6, first finding: run_steps asked _exec_ok before _nat_ok, and _exec_ok read the plain ABMIL scorer of whatever student it
    was given - AttributeError for a gated ABMIL and for a DSMIL student.  Every bag's route is now asked of _step_route, and a chunk
    with a bag that is not the executor's is three train_step calls: the same logits, losses, parameters and moments bit for bit, and
    self.last["exec"] names the route those steps took (the Python orchestration; mhimx_dsmil_mhim_window_run)."""
    tr_m, tr_1 = _trainer(student), _trainer(student)
    g = torch.Generator(device="cuda").manual_seed(4)
    bags = [torch.randn(n, 256, device="cuda", generator=g).abs_() for n in (64, 97, 300)]
    labels = [torch.tensor([j % 2], device="cuda") for j in range(len(bags))]
    assert not any(tr_m._exec_ok(b, j) for j, b in enumerate(bags))
    lm, sm = tr_m.run_steps(bags, labels, i=0)
    for j, (b, l) in enumerate(zip(bags, labels)):
        l1, s1 = tr_1.train_step(b, l, i=j)
    assert torch.equal(lm, l1) and torch.equal(sm, s1)
    assert tr_m.last["exec"] == tr_1.last["exec"] == (False if student == "gated" else "mhimx_dsmil_mhim_window_run")
    assert tr_m.flat.step == tr_1.flat.step == 3
    for tr in (tr_m, tr_1):
        assert int(tr.opt_step) == 3
    for a, b in ((tr_m.flat.student, tr_1.flat.student), (tr_m.flat.teacher, tr_1.flat.teacher), (tr_m.flat.m, tr_1.flat.m),
                 (tr_m.flat.v, tr_1.flat.v), (tr_m.tick, tr_1.tick)):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(tr_m.flat.student).all()) and float(tr_m.flat.m.abs().max()) > 0.0
