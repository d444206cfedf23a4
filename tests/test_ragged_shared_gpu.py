"""The shared merge of a bag's pool partials (rg_merge_stats, csrc/infer_tab.hpp, and the pooled-row loops beside its callers) past its
first 512 partials.  A kernel merges a bag's partials 512 at a time; no other test has a bag of more than 512 partials, so the second
trip of those loops ran nowhere.  One partial is 256 rows: 512 * 256 + 1 = 131 073 rows make 513.  One ragged call each of the ABMIL and
the DSMIL inference (the DSMIL finalize is the strided instance of the helper), D = 256, C = 2, fp32, bags of 131 073, 1 and 257 rows:

  (a) the large bag's outputs have the bits of a call of its own - the position independence the file headers promise;
  (b) they agree with an fp64 softmax-pool of the returned scores over the feature rows (ABMIL; tolerances of tests/test_infer_gpu.py:
      the maximum exact, sum e^{s - max} to 1e-5 relative - its "attention sums to 1" bound -, z atol 2e-4 rtol 1e-3), and with the
      module's bag-after-bag forward_test (DSMIL; LOGIT_TOL / B_TOL of tests/test_infer_dsmil_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import mhim_oracle as O
from tests import test_infer_dsmil_gpu as DD
from tests import test_infer_gpu as TI
from tests.test_mhim_gpu import V2

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 256
SIZES = (512 * 256 + 1, 1, 257)


@functools.lru_cache(maxsize=None)
def _bags():
    """The three bags, made once on the device (seeded; |N(0, 1)| like the timing drivers' bags), shared by both tests, never modified."""
    g = torch.Generator(device=DEV)
    g.manual_seed(700)
    return tuple(torch.randn(n, D, device=DEV, generator=g).abs_() for n in SIZES)


def test_abmil_bag_of_513_partials():
    st = TI._state(21, D, merge_k=5)
    m = TI.build(st, "auto", input_dim=D, **V2).eval()
    xs = list(_bags())
    assert (SIZES[0] + 255) // 256 == 513
    r = TI._call(m, xs)
    alone = TI._call(m, xs[:1])
    torch.cuda.synchronize()
    n = SIZES[0]
    assert r.offsets[:2] == [0, n]
    for f in ("logits", "stats", "z"):                                          # (a)
        assert torch.equal(getattr(r, f)[0], getattr(alone, f)[0]), f
    assert torch.equal(r.score[:n], alone.score) and torch.equal(r.attn[:n], alone.attn)
    # (b)
    po, cfg = O.as_torch(st), O.Cfg(**V2)
    torch.set_num_threads(16)
    with torch.no_grad():
        h = O.feature(xs[0].cpu(), po, cfg.act).double()
    s = r.score[:n].double().cpu()
    mx = s.max()
    e = torch.exp(s - mx)
    stats, z = r.stats[0].cpu(), r.z[0].cpu().numpy()
    print(f"[ragged shared] max {float(stats[0])} vs {float(mx)}, sum {float(stats[1])} vs {float(e.sum())}, "
          f"z max abs diff {float(np.abs(z - ((e / e.sum()) @ h).numpy()).max()):.3e}")
    assert float(stats[0]) == float(mx)
    np.testing.assert_allclose(float(stats[1]), float(e.sum()), rtol=1e-5)
    np.testing.assert_allclose(z, ((e / e.sum()) @ h).numpy(), atol=2e-4, rtol=1e-3)
    assert abs(float(r.attn[:n].double().sum()) - 1.0) < 1e-5


def test_dsmil_bag_of_513_partials():
    cc = 2
    sseed, _ = DD.SEEDS[cc]
    m = DD.build(DD.state(sseed, cc), cc)
    xs = list(_bags())
    r = DD._call(m, xs)
    alone = DD._call(m, xs[:1])
    torch.cuda.synchronize()
    for f in ("logits_bag", "logits_ins", "logits", "B", "crit"):              # (a)
        assert torch.equal(getattr(r, f)[0], getattr(alone, f)[0]), f
    assert torch.equal(r.attn[:SIZES[0]], alone.attn)
    (flb, _), fB = m.forward_test(xs[0])                                        # (b)
    lb, B = r.logits_bag[0].cpu().numpy(), r.B[0].cpu().numpy()
    print(f"[ragged shared] dsmil logits_bag diff {float(np.abs(lb - flb.reshape(-1).cpu().numpy()).max()):.3e}, "
          f"B diff {float(np.abs(B - fB[0].cpu().numpy()).max()):.3e}")
    np.testing.assert_allclose(lb, flb.reshape(-1).cpu().numpy(), atol=DD.LOGIT_TOL, rtol=0)
    np.testing.assert_allclose(B, fB[0].cpu().numpy(), **DD.B_TOL)
