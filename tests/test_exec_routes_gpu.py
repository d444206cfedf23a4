"""What each native route of FusedTrainer (and the two inference wrappers of ops) leaves behind ON THE HOST - GPU box only, because the
routes run their calls, but nothing a kernel computes is looked at (the routes' own test files do that): the route that ran, the counters
(_micro, flat.step), the seed streams (how many draws, for the two windows of the full model also their order), the exact keys of
``tr.last`` and of every ``tr.last["bags"][j]`` with each tensor's shape, dtype and place in the workspace, and the workspace itself - the
slot of ``tr._exec`` it is cached in, its size, when it is kept and when replaced, and that a captured call owns a fresh one.

Shapes are the smallest the routes take (D = 256; 64 rows is the single-bag step's minimum).  Every expected value was taken from the
commit before the routes' host pieces were shared; the file passes there unchanged."""
import pytest
import torch

from mhim_mil_amd import synth
from tests.test_window_gpu import V2, _mk

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, E, CC, KM = 256, 512, 2, 5
F32, F16, I64 = torch.float32, torch.float16, torch.int64
PURE_KEYS = {"logits", "losses", "patch_num", "keep_num", "rows", "score", "R", "tokens", "H_student", "H_teacher"}
STEP_KEYS = PURE_KEYS | {"ws", "exec"}


def _full(accum=1, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    torch.manual_seed(5)
    base = synth.mhim_state(7, input_dim=D, merge_k=KM)
    return FusedTrainer(_mk(base, D, **V2), _mk(synth.spread_teacher(base), D, **V2), aux_alpha=0.5, mm=0.9997, accumulation_steps=accum, **kw)


def _pure(accum=1, **kw):
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    torch.manual_seed(5)
    m = MHIM(input_dim=D, n_classes=CC, baseline="attn", dropout=0.25, act="gelu", da_act="relu", merge_enable=False)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in synth.mhim_state(7, input_dim=D, merge_enable=False).items()})
    return FusedTrainer(m.to(DEV).train(), None, model="mhim_pure", accumulation_steps=accum, **kw)


def _bags(sizes, batch_dim=False, seed=300):
    xs = [torch.from_numpy(synth.bag(seed + j, n, D)).to(DEV) for j, n in enumerate(sizes)]
    return [x[None] for x in xs] if batch_dim else xs, [torch.tensor([j % 2], device=DEV) for j in range(len(sizes))]


def _watch(tr):
    """Records every seed draw as (model, teacher flag) and counts the calls of tr.update()."""
    seen = {"draws": [], "updates": 0}
    for name, m in (("s", tr.s), ("t", tr.t)):
        if m is not None:
            def draw(teacher=False, _m=m, _name=name, _orig=m._next_seed):
                seen["draws"].append((_name, bool(teacher)))
                return _orig(teacher=teacher)
            m._next_seed = draw
    orig = tr.update

    def update():
        seen["updates"] += 1
        return orig()
    tr.update = update
    return seen


def _at(t, ws, off, shape, dtype=F32):
    """t is the view of the workspace at byte ``off`` with this shape and dtype."""
    assert torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape), (t.dtype, tuple(t.shape), shape)
    assert t.data_ptr() - ws.data_ptr() == off, (t.data_ptr() - ws.data_ptr(), off)


def _counters(tr, micro, step, s_draws, t_draws=None):
    assert (tr._micro, tr.flat.step, tr.s._step) == (micro, step, s_draws), (tr._micro, tr.flat.step, tr.s._step)
    assert t_draws is None or tr.t._step == t_draws, tr.t._step


FULL_DRAWS = [("t", True), ("s", False), ("s", False), ("s", False)]       # drop_teacher, drop_student, select, mca


def _check_full_bag(p, ws, lay, base, N, cnt, r0=0):
    """The nine keys every full route keeps per bag (logits / losses are the caller's: their pitch differs by route)."""
    assert (p["patch_num"], p["keep_num"], p["R"]) == (N, cnt.Lk + KM, cnt.R)
    _at(p["rows"], ws, base + lay.rows_all + 8 * r0, (cnt.len_keep,), I64)
    _at(p["score"], ws, base + lay.score + 4 * r0, (N,))
    _at(p["H_student"], ws, base + lay.H_student + 4 * E * r0, (N, E))
    _at(p["tokens"], ws, base + lay.H_student + 4 * E * (r0 + N), (KM, E))
    _at(p["H_teacher"], ws, base + lay.H_teacher + 4 * E * r0, (N, E))


def _check_pure_last(last, ws, lay, N):
    assert set(last) == STEP_KEYS and last["exec"] is True and last["ws"] is ws
    assert (last["patch_num"], last["keep_num"], last["R"]) == (N, N, 0)
    assert last["rows"] is None and last["score"] is None and last["tokens"] is None and last["H_teacher"] is None
    _at(last["logits"], ws, lay.logits, (CC,)); _at(last["losses"], ws, lay.losses, (3,))
    _at(last["H_student"], ws, lay.H_student, (N, E))


# ------------------------------------------------------------------------------------------------------------------ the single-bag step
@pytest.mark.parametrize("inside", [True, False])
def test_exec_step_full(inside):
    tr = _full(clip_grad=None if inside else 1.0)           # (clipping keeps the update outside the call)
    seen = _watch(tr)
    (x,), (y,) = _bags([64], batch_dim=True)
    logits, losses = tr.train_step(x, y)
    assert tr.last["exec"] is True
    _counters(tr, 0, 1, 3, 1)
    assert seen["draws"] == FULL_DRAWS and seen["updates"] == (0 if inside else 1)
    (key, (cnt, lay)), = tr._exec["layouts"].items()
    assert key == (64, cnt.k_top, cnt.n_sel, cnt.Lk)
    ws = tr._exec["ws"]
    assert ws.numel() == int(lay.total * 1.25) and tr.last["ws"] is ws and set(tr.last) == STEP_KEYS
    _at(tr.last["logits"], ws, lay.logits, (CC,)); _at(tr.last["losses"], ws, lay.losses, (3,))
    assert logits is tr.last["logits"] and losses is tr.last["losses"]
    _check_full_bag(tr.last, ws, lay, 0, 64, cnt)
    torch.cuda.synchronize()


@pytest.mark.parametrize("inside", [True, False])
def test_exec_step_pure(inside):
    """(the pure step leaves clipping to the Python orchestration: its update stays outside when forward_backward is called on its own)"""
    tr = _pure()
    seen = _watch(tr)
    (x,), (y,) = _bags([64])
    if inside:
        tr.train_step(x, y)
        _counters(tr, 0, 1, 1)
    else:
        tr.forward_backward(x, y)
        _counters(tr, 1, 0, 1)
    assert tr.last["exec"] is True and seen["draws"] == [("s", False)] and seen["updates"] == 0
    assert list(tr._exec["layouts"]) == [("pure", 64)]
    lay = tr._exec["layouts"][("pure", 64)][1]
    ws = tr._exec["ws"]
    assert ws.numel() == int(lay.total * 1.25)
    _check_pure_last(tr.last, ws, lay, 64)
    if not inside:
        tr.update()
        _counters(tr, 0, 1, 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ run_steps
def test_run_steps_full():
    tr = _full()
    seen = _watch(tr)
    xs, ys = _bags([64, 97], batch_dim=True)
    logits, losses = tr.run_steps(xs, ys)
    _counters(tr, 0, 2, 6, 2)
    assert seen["draws"] == FULL_DRAWS * 2 and seen["updates"] == 0
    assert tr.last == {}                                    # (the full model's run_steps leaves tr.last alone)
    lays = {k[0]: v[1] for k, v in tr._exec["layouts"].items()}
    ws = tr._exec["ws"]
    assert sorted(lays) == [64, 97] and ws.numel() == int(max(l.total for l in lays.values()) * 1.25)
    _at(logits, ws, lays[97].logits, (CC,)); _at(losses, ws, lays[97].losses, (3,))
    torch.cuda.synchronize()


def test_run_steps_full_with_clipping_goes_bag_by_bag_through_the_step():
    tr = _full(clip_grad=1.0)
    seen = _watch(tr)
    xs, ys = _bags([64, 97], batch_dim=True)
    tr.run_steps(xs, ys)
    assert tr.last["exec"] is True and set(tr.last) == STEP_KEYS and tr.last["patch_num"] == 97
    _counters(tr, 0, 2, 6, 2)
    assert seen["draws"] == FULL_DRAWS * 2 and seen["updates"] == 2
    torch.cuda.synchronize()


def test_run_steps_pure():
    tr = _pure()
    seen = _watch(tr)
    xs, ys = _bags([64, 97])
    logits, losses = tr.run_steps(xs, ys)
    _counters(tr, 0, 2, 2)
    assert seen["draws"] == [("s", False)] * 2 and seen["updates"] == 0
    lays = tr._exec["layouts"]
    ws = tr._exec["ws"]
    assert sorted(lays) == [("pure", 64), ("pure", 97)] and ws.numel() == int(lays[("pure", 97)][1].total * 1.25)
    _check_pure_last(tr.last, ws, lays[("pure", 97)][1], 97)
    assert logits is tr.last["logits"] and losses is tr.last["losses"]
    torch.cuda.synchronize()


def test_run_steps_pure_with_clipping_takes_the_python_orchestration():
    tr = _pure(clip_grad=1.0)
    seen = _watch(tr)
    xs, ys = _bags([64, 97])
    tr.run_steps(xs, ys)
    assert tr.last["exec"] is False
    _counters(tr, 0, 2, 2)
    assert seen["updates"] == 2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the three windows
WAYS = [("inside", None, True), ("outside", 1.0, True), ("no update", None, False)]


def _window_counters(tr, seen, way, n, s_draws, t_draws=None):
    if way == "no update":
        _counters(tr, n, 0, s_draws, t_draws)
    else:
        _counters(tr, 0, 1, s_draws, t_draws)
    assert seen["updates"] == (1 if way == "outside" else 0)


@pytest.mark.parametrize("way, clip, update", WAYS)
def test_exec_window(way, clip, update):
    tr = _full(accum=2, clip_grad=clip)
    seen = _watch(tr)
    xs, ys = _bags([64, 64], batch_dim=True)
    logits, losses = tr.window_step(xs, ys, update=update)
    assert tr.last["exec"] == "mhimx_window_run"
    _window_counters(tr, seen, way, 2, 6, 2)
    # every bag's two dropout seeds first, then bag after bag the select's and Merge's
    assert seen["draws"] == [("t", True), ("s", False)] * 2 + [("s", False)] * 4
    (key, (cnt, lay)), = tr._exec["layouts"].items()
    assert key == ("window", 2, 64, cnt.k_top, cnt.n_sel, cnt.Lk)
    ws = tr._exec["ws_win"]
    assert ws.numel() == lay.total and tr.last["ws"] is ws and tr._exec["ws"] is None
    assert set(tr.last) == PURE_KEYS | {"bags", "ws", "exec"} and len(tr.last["bags"]) == 2
    for j, p in enumerate(tr.last["bags"]):
        base = j * lay.bag_stride
        assert set(p) == PURE_KEYS
        _at(p["logits"], ws, base + lay.bag.logits, (CC,)); _at(p["losses"], ws, base + lay.bag.losses, (3,))
        _check_full_bag(p, ws, lay.bag, base, 64, cnt)
        assert logits[j] is p["logits"] and losses[j] is p["losses"] and tr.last["logits"][j] is p["logits"] and tr.last["losses"][j] is p["losses"]
    assert all(tr.last[k] is tr.last["bags"][-1][k] for k in PURE_KEYS - {"logits", "losses"})
    torch.cuda.synchronize()


SIZES = (64, 97, 257)


@pytest.mark.parametrize("way, clip, update", WAYS)
def test_exec_pure_window(way, clip, update):
    tr = _pure(accum=3, clip_grad=clip)
    seen = _watch(tr)
    xs, ys = _bags(SIZES)
    logits, losses = tr.window_step(xs, ys, update=update)
    assert tr.last["exec"] is True and "layout" in tr.last
    _window_counters(tr, seen, way, 3, 3)
    assert seen["draws"] == [("s", False)] * 3
    lay, ws = tr.last["layout"], tr._exec["ws_pw"]
    assert ws.numel() == int(lay.total * 1.25) and tr.last["ws"] is ws and tr._exec["ws"] is None
    assert set(tr.last) == PURE_KEYS | {"bags", "layout", "ws", "exec", "x_dtype"} and tr.last["x_dtype"] == F32
    assert tr.last["rows"] is None and tr.last["score"] is None and tr.last["tokens"] is None and tr.last["H_teacher"] is None and tr.last["R"] == 0
    for j, (p, N) in enumerate(zip(tr.last["bags"], SIZES)):
        r0 = int(lay.row0[j])
        assert set(p) == {"logits", "losses", "patch_num", "keep_num", "row0", "H_student", "dact"}
        assert (p["patch_num"], p["keep_num"], p["row0"]) == (N, N, r0)
        _at(p["logits"], ws, lay.logits + 4 * CC * j, (CC,)); _at(p["losses"], ws, lay.losses + 12 * j, (3,))
        _at(p["H_student"], ws, lay.H + 4 * E * r0, (N, E)); _at(p["dact"], ws, lay.dact + 2 * E * r0, (N, E), F16)
        assert logits[j] is p["logits"] and losses[j] is p["losses"] and tr.last["logits"][j] is p["logits"] and tr.last["losses"][j] is p["losses"]
    assert tr.last["H_student"] is tr.last["bags"][-1]["H_student"] and tr.last["patch_num"] == tr.last["keep_num"] == 257
    torch.cuda.synchronize()


RAGGED_KEYS = PURE_KEYS | {"dact", "z_teacher", "z_student", "row0"}


@pytest.mark.parametrize("way, clip, update", WAYS)
def test_exec_ragged_window(way, clip, update):
    tr = _full(accum=3, clip_grad=clip)
    seen = _watch(tr)
    xs, ys = _bags(SIZES, batch_dim=True)
    logits, losses = tr.window_step(xs, ys, update=update)
    assert tr.last["exec"] == "mhimx_ragged_window_run"
    _window_counters(tr, seen, way, 3, 9, 3)
    assert seen["draws"] == FULL_DRAWS * 3                  # bag after bag
    lay, table, ws = tr.last["layout"], tr.last["table"], tr._exec["ws_rw"]
    assert ws.numel() == int(lay.total * 1.25) and tr.last["ws"] is ws and tr._exec["ws"] is None
    assert set(tr.last) == RAGGED_KEYS | {"bags", "layout", "table", "ws", "exec", "x_dtype"} and tr.last["x_dtype"] == F32
    for j, (p, N) in enumerate(zip(tr.last["bags"], SIZES)):
        r0 = int(lay.row0[j])
        assert set(p) == RAGGED_KEYS and p["row0"] == r0
        _at(p["logits"], ws, lay.logits + 64 * j, (CC,)); _at(p["losses"], ws, lay.losses + 16 * j, (3,))
        _check_full_bag(p, ws, lay, 0, N, table[j].cnt, r0)
        _at(p["dact"], ws, lay.dact + 2 * E * r0, (N, E), F16)
        _at(p["z_teacher"], ws, lay.z_teacher + 4 * E * j, (E,)); _at(p["z_student"], ws, lay.z_student + 4 * E * j, (E,))
        assert logits[j] is p["logits"] and losses[j] is p["losses"] and tr.last["logits"][j] is p["logits"] and tr.last["losses"][j] is p["losses"]
    assert all(tr.last[k] is tr.last["bags"][-1][k] for k in RAGGED_KEYS - {"logits", "losses", "patch_num", "keep_num", "R", "row0"})
    assert all(tr.last[k] == tr.last["bags"][-1][k] for k in ("patch_num", "keep_num", "R", "row0"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the workspace
def _step_total(tr, N):
    return max(v[1].total for k, v in tr._exec["layouts"].items() if (k[1] if k[0] == "pure" else k[0]) == N)


@pytest.mark.parametrize("route", ["step", "pure step", "run_steps", "pure run_steps", "window", "pure window", "ragged window"])
def test_the_workspace_is_kept_for_smaller_bags_and_replaced_for_larger_ones(route):
    pure = route.startswith("pure")
    windowed = route.endswith("window")
    tr = (_pure if pure else _full)(accum={"window": 2, "pure window": 3, "ragged window": 3}.get(route, 1))
    slot = {"window": "ws_win", "pure window": "ws_pw", "ragged window": "ws_rw"}.get(route, "ws")
    slack = 1.0 if route == "window" else 1.25
    sizes = {"step": ([128], [64], [4096]), "run_steps": ([128, 97], [64, 64], [4096, 64]), "window": ([128] * 2, [64] * 2, [4096] * 2)}.get(
        route[5:] if pure and not windowed else route, (list(SIZES), [64, 65, 66], [1100, 2100, 4100]))      # (different sizes: a same-shaped full window is mhimx_window_run's)
    # (the larger call must need more than 1.25 x the first: at D = 256 the parts of a layout that do not grow with N weigh ~95 MB in the
    # full step (38 MB pure, 60 MB ragged window) and a row 24 KB (14 KB, 7 KB) - mhimx_step_layout_of: 98.2 MB at 128 rows, 119.8 MB at
    # 1 024, 193.0 MB at 4 096; the ragged window: 65.1 MB for SIZES, 147.2 MB for the larger list)

    def run(ns):
        xs, ys = _bags(ns, batch_dim=not pure)
        if windowed:
            tr.window_step(xs, ys)
            assert tr.last["exec"] == {"window": "mhimx_window_run", "ragged window": "mhimx_ragged_window_run"}.get(route, True)
            return tr.last["layout"].total if "layout" in tr.last else next(
                v[1].total for k, v in tr._exec["layouts"].items() if k[:3] == ("window", 2, ns[0]))
        if route.endswith("run_steps"):
            tr.run_steps(xs, ys)
        else:
            tr.train_step(xs[0], ys[0])
            assert tr.last["exec"] is True
        return max(_step_total(tr, n) for n in ns)

    total = run(sizes[0])
    ws0 = tr._exec[slot]
    assert ws0.numel() == int(total * slack)
    assert run(sizes[1]) < total and tr._exec[slot] is ws0
    if route != "run_steps":
        assert tr.last["ws"] is ws0
    larger = run(sizes[2])
    assert larger > ws0.numel() and tr._exec[slot] is not ws0 and tr._exec[slot].numel() == int(larger * slack)
    assert {k for k, v in tr._exec.items() if k.startswith("ws") and v is not None} == {slot}
    torch.cuda.synchronize()


def test_a_captured_step_and_a_captured_window_own_a_fresh_workspace():
    tr = _full()
    (x,), (y,) = _bags([64], batch_dim=True)
    g = tr.capture(x, y, warmup=1)
    cached = tr._exec["ws"]
    lay = next(iter(tr._exec["layouts"].values()))[1]
    assert tr.last["exec"] is True and tr.last["ws"] is not cached and tr.last["ws"].numel() == lay.total
    assert cached is not None and cached.numel() == int(lay.total * 1.25)
    tr = _full(accum=3)
    xs, ys = _bags(SIZES, batch_dim=True)
    gw = tr.capture_window(xs, ys, warmup=1)
    cached = tr._exec["ws_rw"]
    total = tr.last["layout"].total
    assert tr.last["exec"] == "mhimx_ragged_window_run" and tr.last["ws"] is not cached and tr.last["ws"].numel() == total
    assert cached is not None and cached.numel() == int(total * 1.25)
    torch.cuda.synchronize()
    del g, gw


def test_the_inference_wrappers_share_one_workspace_per_device():
    """ops.infer_many / ops.infer_dsmil_many: ops._INFER_WS[device index], exactly the bytes the first call needs, kept for smaller
    calls - of either wrapper -, replaced for a larger one."""
    from mhim_mil_amd import ops
    from tests.test_infer_dsmil_gpu import build, state
    idx = torch.cuda.current_device()
    ops._INFER_WS.pop(idx, None)                            # (whatever an earlier test file left there)
    ab = _pure().s.eval()
    ds = build(state(151, CC), CC)
    cfg, dcfg = ab._infer_cfg(), ds._infer_dsmil_cfg()
    mid, small, large = _bags([64, 97, 257])[0], _bags([1, 33])[0], _bags([257, 600, 1100])[0]
    ops.infer_many(cfg, mid)
    ws0 = ops._INFER_WS[idx]
    assert ws0.numel() == ops.infer_ws_bytes(cfg, mid)
    ops.infer_many(cfg, small)
    assert ops._INFER_WS[idx] is ws0
    need = ops.infer_dsmil_ws_bytes(dcfg, large)
    assert need > ws0.numel()
    ops.infer_dsmil_many(dcfg, large)
    ws1 = ops._INFER_WS[idx]
    assert ws1 is not ws0 and ws1.numel() == need
    ops.infer_dsmil_many(dcfg, small)
    assert ops._INFER_WS[idx] is ws1
    assert ops.infer_ws_bytes(cfg, large) <= need
    ops.infer_many(cfg, large)
    assert ops._INFER_WS[idx] is ws1
    mine = torch.full((ops.infer_ws_bytes(cfg, small),), 255, dtype=torch.uint8, device=DEV)
    ops.infer_many(cfg, small, ws=mine)                     # (a caller's own workspace leaves the cache alone)
    assert ops._INFER_WS[idx] is ws1
    torch.cuda.synchronize()
