"""The weight gradient's two-workgroups-per-CU form (csrc/wgrad.hip: bag_wgrad_ws2_kernel, mhimx_bag_wgrad_args.form = 2) against the
one-per-CU form (form = 1) on the same inputs: the same slabs, k order and term order, so every slab float and the reduced dW1 are equal
BIT FOR BIT (torch.equal).

Where D is a multiple of 128 but not of 256 the one-per-CU form cannot take the shape itself: it then runs over the same rows widened to
the next multiple of 256 (the columns of a product are independent and the slab plan of such a D is that of the widened one), and its
first D columns are the reference."""
import copy
import ctypes as C

import pytest
import torch

from mhim_mil_amd import _lib as L
from mhim_mil_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _inputs(N, n_rows, E, pitch, seed, rows="sorted"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((N, pitch), generator=g).abs().to(DEV)
    dH = (torch.randn((N, E), generator=g) * 1e-3).to(DEV)
    if rows == "sorted":
        r = torch.randperm(N, generator=g)[:n_rows].sort().values.to(DEV)
    elif rows == "repeats":                                         # any order, some rows more than once
        r = torch.randint(0, N, (n_rows,), generator=g).to(DEV)
    else:
        r = None
    return x, dH, r


def _image(dH, rows, n_rows, E):
    lib = L.lib()
    img = torch.zeros(lib.mhimx_wgrad_image_bytes(n_rows, E) // 4, device=DEV)
    L.check(lib.mhimx_rows_dpre_image(ops._stream(), ops._p(dH), None, ops._p(rows), n_rows, E, ops._p(img), None, 0, None, 0, None), "image")
    return img


def _product(x, img, rows, n_rows, E, D, form):
    """(slabs [splits, E, D], dW [E, D]) of one launch + its slab sum; x [N, pitch >= D]"""
    lib = L.lib()
    ws = torch.full((lib.mhimx_wgrad_ws_floats(n_rows, E, D),), float("nan"), device=DEV)
    out = torch.full((E, D), float("nan"), device=DEV)
    g = L.BagWgrad(img=ops._p(img), X=ops._p(x), ldx=x.stride(0), n_bag_rows=x.shape[0], rows=ops._p(rows), L=n_rows, E=E, D=D, C=ops._p(out),
                   ldc=D, accumulate=0, ws=ops._p(ws), ws_floats=ws.numel(), defer=None, form=form)
    L.check(lib.mhimx_bag_wgrad(ops._stream(), C.byref(g)), "mhimx_bag_wgrad")
    torch.cuda.synchronize()
    return ws.view(-1, E, D), out


def _both(N, n_rows, E, D, seed, rows="sorted", pitch=None):
    Dw = -(-D // 256) * 256
    x, dH, r = _inputs(N, n_rows, E, pitch or Dw, seed, rows)
    img = _image(dH, r, n_rows, E)
    s1, w1 = _product(x, img, r, n_rows, E, Dw, 1)
    s2, w2 = _product(x, img, r, n_rows, E, D, 2)
    assert s1.shape[0] == s2.shape[0], "the two forms must plan the same slabs"
    assert torch.equal(s2, s1[:, :, :D]) and torch.equal(w2, w1[:, :D])
    assert bool(torch.isfinite(w2).all())
    return s2.shape[0], x, dH, r, w2


@pytest.mark.parametrize("n_rows", [32, 33, 95])
def test_one_tile_one_slab_and_clamped_tail_rows(n_rows):
    """E = 128, D = 128: one tile, one slab; L = 32: one full k-step; 33 / 95: rows past L inside the last k-step (clamped, times zero)"""
    assert _both(120, n_rows, 128, 128, seed=n_rows)[0] == 1


@pytest.mark.parametrize("nk,E,D", [(1, 128, 128), (2, 128, 128), (3, 128, 128), (4, 128, 128), (7, 2048, 4096)])
def test_ring_fill_wrap_and_drain(nk, E, D):
    """nk k-steps in ONE slab (seven need the 256 tiles of E = 2048, D = 4096: fewer tiles split seven k-steps over two slabs)"""
    assert _both(nk * 32 + 9, nk * 32 - 5 if nk > 1 else 27, E, D, seed=100 + nk)[0] == 1


@pytest.mark.parametrize("splits,n_rows", [(1, 128), (3, 345), (8, 1024), (16, 2045)])
def test_tile_grid_and_slabs(splits, n_rows):
    """E = 256, D = 384 (2 x 3 tiles, bag rows wider than D): fewer than 8 slabs, workgroups past the last slab, a shorter last slab"""
    assert _both(2100, n_rows, 256, 384, seed=splits)[0] == splits


@pytest.mark.parametrize("rows", [None, "repeats"])
def test_row_lists_and_pitch(rows):
    """rows null (the bag's first L rows) and a row list in any order with repeats; ldx > D"""
    _both(500, 200 if rows else 333, 128, 128, seed=7, rows=rows, pitch=264)
    _both(500, 200 if rows else 333, 256, 256, seed=8, rows=rows, pitch=260)


def test_against_fp64():
    """the tolerance of tests/test_wgrad_gpu.py::test_bag_wgrad_vs_fp64: 2e-5 of the largest element (three-term bf16, ~2^-16)"""
    N, n_rows, E, D = 700, 333, 256, 384
    x, dH, r = _inputs(N, n_rows, E, 512, seed=21)
    dact = (torch.randn((N, E), generator=torch.Generator().manual_seed(3)) * 0.7).to(torch.float16).to(DEV)
    dW, db = ops.bag_wgrad(dH, dact, x[:, :D], r, n_rows, form=2)
    dpre = dH[r].double() * dact[r].double()
    rW, rb = dpre.t() @ x[r, :D].double(), dpre.sum(0)
    assert float((dW.double() - rW).abs().max()) <= 2e-5 * float(rW.abs().max()) + 1e-12
    assert float((db.double() - rb).abs().max()) <= 1e-5 * float(rb.abs().max()) + 1e-12


def test_automatic_is_one_of_the_two_and_form_is_checked():
    x, dH, r = _inputs(300, 100, 128, 256, seed=2)
    img = _image(dH, r, 100, 128)
    s0, w0 = _product(x, img, r, 100, 128, 256, 0)
    s1, w1 = _product(x, img, r, 100, 128, 256, 1)
    assert torch.equal(s0, s1) and torch.equal(w0, w1)
    with pytest.raises(L.MhimxError):
        _product(x, img, r, 100, 128, 256, 3)
    with pytest.raises(L.MhimxError):
        _product(x, img, r, 100, 128, 128, 1)                      # D = 128 is the two-per-CU form's alone


def test_step_with_riders_is_the_same_step():
    """One mhimx_step_run (the Merge tail's stages and the queued reductions ride in the weight-gradient launch, with its smaller LDS):
    logits, losses, and weights, moments and teacher after the update, then every gradient of a forward + backward, bit for bit with
    either form."""
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    cfg = dict(mask_ratio_h=0.03, mask_ratio_hr=0.5, merge_enable=True, merge_k=5, merge_mm=0.9999, merge_ratio=0.9, act="gelu",
               da_act="relu", attn2score=True, temp_t=0.1)
    res = []
    for form in (1, 2):
        torch.manual_seed(11)
        s = MHIM(input_dim=256, n_classes=2, baseline="attn", dropout=0.25, **cfg).cuda().train()
        t = copy.deepcopy(s).train()
        t.merge_test = False
        tr = FusedTrainer(s, t, lr=1e-3, mm=0.999, aux_alpha=0.5)
        tr.wgrad_form = form
        x = torch.randn(1500, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)).abs_()
        logits, losses = tr.train_step(x, torch.tensor([1], device=DEV))
        torch.cuda.synchronize()
        assert tr._exec is not None and tr.last.get("ws") is not None, "the executor did not run"
        fl = tr.flat
        state = [logits.clone(), losses.clone(), fl.student.clone(), fl.teacher.clone(), fl.m.clone(), fl.v.clone()]
        tr.forward_backward(x, torch.tensor([0], device=DEV))         # (update = 0: the complete gradient stays in the flat buffer)
        torch.cuda.synchronize()
        res.append(state + [fl.grad.clone()])
    assert float(res[0][-1].abs().max()) > 0
    for a, b in zip(*res):
        assert torch.equal(a, b)
