"""The token block of the gated scorer backward (scorer_fused_bwd_kernel, block 0 of a launch in which a Merge backward's first stage
rides): it alone produces the riders' dz - the k merged tokens' gradient rows at the end of the student's list [rows that stay | tokens] -
with the tile's arithmetic, and the tile blocks leave those rows to it.

Every case runs the same backward twice through the public ops: GATED (the Merge stage parked before abmil_pool_bwd, so the launch has the
token block and the riders) and UNGATED (nothing parked: tile blocks only, the Merge stage runs after the launch).  The ungated launch has
no token block, so bit-identical results check the new block against the tile path: dT on every row, the pool workspace (du, the d_wc /
d_bc partials), the dPRE image and its column sums, d_wa / d_wc / d_bc after the flush and every gradient of the Merge backward.  A rider
that took its give-up path poisons the Merge gradients with NaN: they are checked finite."""
import numpy as np
import pytest
import torch

from mhim_mil_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, A, N, R = 512, 128, 256, 40            # E, A: fixed by the kernel; N rows in the bag, R of them merged into the k tokens
MERGE_KEYS = ("d_ln_w", "d_ln_b", "d_wkv", "d_wq", "d_wo", "d_bo")


def rnd(seed, shape, std=1.0):
    return torch.from_numpy((synth.normal(seed, shape) * std).astype(np.float32))


def _pool_ws_written(ws, M):
    """The parts of a PoolState's workspace that the one-pass backward writes: du [M, A] and the first ceil(M / 32) rows of the d_wc
    and d_bc partials, as int32.  The rest of the workspace (spare partial rows, slabs of paths these shapes do not take) is never
    written and holds whatever the allocator left there, so the workspace cannot be compared whole.  The offsets restate
    pool_ws_layout (csrc/rows.hip: every array rounded up to 256 bytes, G = 2 MAX_PART = 1024 partial rows); the total is checked
    against the library's own figure so that a change of that layout fails here and is not compared past."""
    from mhim_mil_amd import _lib as L
    G, TN_SLABS, off, at = 1024, 128, 0, {}
    for name, floats in (("pm", G), ("pl", G), ("pz", G * E), ("attn", M), ("du", M * A), ("dwc_part", G * A), ("dbc_part", G),
                         ("u_pre", M * A), ("tn_ws", TN_SLABS * A * E), ("nt_ws", 4 * M * A)):
        at[name] = off
        off += -(-floats * 4 // 256) * 256
    assert off == L.lib().mhimx_abmil_pool_ws_bytes(M, E, A, 0) and ws.numel() >= off, "pool_ws_layout changed: restate it here"
    tiles = -(-M // 32)
    take = lambda name, floats: ws[at[name]:at[name] + 4 * floats].clone().view(torch.int32)
    return take("du", M * A), take("dwc_part", tiles * A), take("dbc_part", tiles)


def _run_case(Lk, k, with_img, drop_p):
    from mhim_mil_amd import _lib as L
    from mhim_mil_amd import ops
    assert R + Lk <= N
    Hbuf = torch.zeros(N + k, E, device=DEV)
    Hbuf[:N] = rnd(1, (N, E)).to(DEV)
    perm = torch.from_numpy(synth.permutation(2, N).copy()).to(DEV)
    merge_rows, stay = perm[:R].contiguous(), perm[R:R + Lk]
    rows1 = torch.cat([stay, N + torch.arange(k, device=DEV)]).contiguous()            # [Lk stay rows | the k tokens behind the bag]
    M = Lk + k
    wa, wc = rnd(3, (A, E), std=0.05).to(DEV), rnd(4, (1, A), std=0.3).to(DEV)
    sc = ops.ScorerW(wa, wc, L.ACT["relu"], prec="bf16x3")
    wa_t = ops.transpose(wa)
    wa_t_frag = torch.empty_like(wa_t)
    ops.prep_batch([(ops.PREP_FRAG_T, wa, wa_t_frag)])
    q = rnd(13, (k, E), std=0.05).to(DEV)
    lnw, lnb = (1 + rnd(14, (E,), std=0.1)).to(DEV), rnd(15, (E,), std=0.1).to(DEV)
    wkv, wq = rnd(16, (1024, E), std=0.04).to(DEV), rnd(17, (512, E), std=0.04).to(DEV)
    wo, bo = rnd(18, (E, 512), std=0.04).to(DEV), rnd(19, (E,), std=0.1).to(DEV)
    tr = (ops.transpose(wkv), ops.transpose(wq), ops.transpose(wo))
    tick = torch.zeros(1, dtype=torch.int64, device=DEV)
    mw = ops.MergeW(q, lnw, lnb, wkv, wq, wo, bo, 0.999, prec="bf16x3", transposes=tr, x_rows=merge_rows, drop_p=drop_p, drop_seed=77,
                    drop_tick=tick if drop_p > 0 else None)
    g_z = rnd(5, (E,)).to(DEV)
    dact = (rnd(6, (N, E)).to(DEV) * 0.7).half()                 # [N, E]: the tokens (source rows N + j) have no row in it
    tiles = -(-M // 32)
    img_floats = L.lib().mhimx_wgrad_image_bytes(tiles * 32, E) // 4

    def run(gated):
        # (the Merge forward makes the tokens Hbuf[N:], its workspace, and resets the gate the riders wait on)
        _, _, mws = ops.merge_fwd(mw, Hbuf, z_out=Hbuf[N:], update_q=False)
        st = ops.abmil_pool_fwd(sc, Hbuf, None, rows1=rows1)
        dH = torch.zeros(N + k, E, device=DEV)
        lst = ops.ReduceList()
        mgr = {"dX": dH}
        for key, shape in zip(MERGE_KEYS, ((E,), (E,), (1024, E), (512, E), (E, 512), (E,))):
            mgr[key] = torch.zeros(shape, device=DEV)
        pool_g = {"dT1": dH, "d_wa": torch.zeros(A, E, device=DEV), "d_wc": torch.zeros(1, A, device=DEV)}
        img = torch.full((img_floats,), float("nan"), device=DEV) if with_img else None
        part = torch.full((tiles, E), float("nan"), device=DEV) if with_img else None
        if gated:
            ops.merge_bwd_park(mw, Hbuf, dH[N:], mws, mgr, defer=lst)
            assert lst.c.pre.pending == 1, "the Merge stage was not parked"
        g = ops.abmil_pool_bwd(sc, st, g_z, wa_t, need_bias=True, grads=pool_g, defer=lst, wa_t_frag=wa_t_frag, img=img,
                               img_dact=dact if with_img else None, img_part=part, img_rows=Lk if with_img else 0)
        assert lst.c.pre.pending == (2 if gated else 0), "the gated launch did not take the parked stage"
        mg = ops.merge_bwd(mw, Hbuf, dH[N:], mws, grads=mgr, defer=lst)
        ops.reduce_flush(lst)
        torch.cuda.synchronize()
        out = {"dT": dH, "d_wa": g["d_wa"], "d_wc": g["d_wc"], "d_bc": g["d_bc"]}
        out["du"], out["d_wc partials"], out["d_bc partials"] = _pool_ws_written(st.ws, M)
        if with_img:
            out["image"], out["img_part"] = img.view(torch.int32), part.view(torch.int32)
        for key in MERGE_KEYS:
            out["merge " + key] = mg[key]
        return out, st

    got, st = run(True)
    ref, _ = run(False)
    for name in ref:
        assert torch.equal(got[name], ref[name]), f"{name} differs between the gated and the ungated launch"
    for key in MERGE_KEYS:
        assert torch.isfinite(got["merge " + key]).all(), f"merge {key}: a rider gave up"
    # the rows of dT that took part are written (tokens always; the rows that stay unless they left as image rows), no other row is
    dT = got["dT"]
    assert (dT[N:].abs().sum(1) > 0).all()
    touched = torch.zeros(N + k, dtype=torch.bool, device=DEV)
    touched[N:] = True
    touched[merge_rows] = True                                   # (the Merge backward scatters dX there)
    if not with_img:
        touched[stay] = True
        assert (dT[stay].abs().sum(1) > 0).all()
    assert (dT[~touched] == 0).all()
    return got


CASES = [(96, 5),      # the tokens open a fresh tile (Lk % 32 == 0)
         (125, 5),     # the tokens straddle two tiles (3 + 2)
         (127, 1),     # a single token in the last slot of a tile
         (90, 6),      # the largest k the step allows, mid-tile
         (20, 5)]      # the whole list shorter than one tile (M < 32)


@pytest.mark.parametrize("with_img", [False, True], ids=["rows", "image"])
@pytest.mark.parametrize("Lk,k", CASES)
def test_token_block_equals_the_tile_path(Lk, k, with_img):
    _run_case(Lk, k, with_img, 0.0)


def test_token_block_with_dropout_in_the_merge():
    _run_case(125, 5, True, 0.25)


def test_token_block_in_every_plane_of_a_bag_batched_launch():
    """Two bags whose student lists are the 125 / 5 case (N = 160: 5 rows masked, 30 merged, 125 stay, 5 tokens) as ONE window through the
    bag-batched launches (mhimx_window_run: blockIdx.z = bag, every plane with its own token block, gate and riders) against the same
    two bags as single-bag launches with the same seeds.  Bit for bit: draws, tokens, logits, losses and the accumulated gradient of every
    parameter that the scorer backward launch and its riders feed (the scorer's and the Merge's).  The projection's and the predictor's
    gradients are summed over the bags in another order by the batched window (one multi-bag weight-gradient launch, its slab count
    following the launch's size), with or without a token block: they get test_window_gpu's bound for this same comparison."""
    from mhim_mil_amd import engine as EN
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    n, d, acc = 160, 256, 2
    cfg = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5,
               merge_mm=0.9999, merge_ratio=0.81, temp_t=0.1, dropout=0.0)
    base = synth.mhim_state(7, input_dim=d, merge_k=5)

    def mk(sd):
        m = MHIM(input_dim=d, n_classes=2, baseline="attn", **cfg)
        sd = dict(sd)
        sd["merge.global_q"] = sd["merge.global_q_mm"]
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        m = m.to(DEV).train()
        m.merge.dropout = 0.0
        return m

    xs = [torch.from_numpy(synth.bag(900 + j, n, d)).to(DEV)[None] for j in range(acc)]
    ls = [torch.tensor([j % 2], device=DEV) for j in range(acc)]
    old = EN._WINDOW_PROJECT, EN._WINDOW_BATCHED
    res = []
    try:
        for batched in (False, True):
            EN._WINDOW_PROJECT, EN._WINDOW_BATCHED = True, batched
            torch.manual_seed(5)
            s, t = mk(base), mk(synth.spread_teacher(base))
            tr = FusedTrainer(s, t, aux_alpha=0.5, mm=0.9997, accumulation_steps=acc)
            assert tr._exec_window_ok([x[0] for x in xs], ls) == batched
            logits, losses = tr.window_step(xs, ls, n_streams=1, update=False)
            torch.cuda.synchronize()
            per = tr.last["bags"]
            for b in per:
                assert b["R"] == 30 and b["rows"].numel() == 30 + 125, "not the 125 / 5 list"
            res.append(dict(logits=torch.stack([l.reshape(-1) for l in logits]).cpu(), losses=torch.stack([l.reshape(-1)[:3] for l in losses]).cpu(),
                            rows=torch.stack([b["rows"] for b in per]).cpu(), tokens=torch.stack([b["tokens"] for b in per]).cpu()))
            res[-1].update({"grad " + name: g.detach().cpu().clone() for name, g in tr.flat.grad_views.items()})
    finally:
        EN._WINDOW_PROJECT, EN._WINDOW_BATCHED = old
    a, b = res
    other_order = ("grad feature.0.weight", "grad feature.0.bias", "grad predictor.weight")     # (summed over the bags in another order)
    assert sum(name.startswith("grad merge.") for name in a) == 6 and sum(name.startswith("grad online_encoder.attention.") for name in a) == 2
    for name in a:
        assert torch.isfinite(b[name].float()).all(), f"{name}: not finite (a rider gave up)"
        if name in other_order:
            g0, g1 = a[name].numpy(), b[name].numpy()
            np.testing.assert_allclose(g0, g1, atol=3e-6 * np.abs(g0).max(), rtol=1e-4, err_msg=name)
        else:
            assert torch.equal(a[name], b[name]), f"{name} differs between the bag-batched window and the single-bag launches"
