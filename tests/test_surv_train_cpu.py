"""Survival training in the native train calls (mhimx_head_surv_fwd_bwd, mhimx_pure_window_run_surv, mhimx_ragged_window_run_surv) without
a GPU: the entry points are declared, exported and bound, mhimx_surv_spec has its size and offsets, no pinned struct changed, every new
refusal is an error status raised before any device call and names the bag, ops.surv_spec_ok mirrors the C checks, and
FusedTrainer(loss="nll_surv") refuses the models the calls do not serve.  Pointers handed over here are made-up addresses: a refused call
never touches them; a 1-byte workspace is the probe that every check before the workspace's passed (tests/test_exec_mirror_cpu.py)."""
import ctypes as C
import os
import re

import pytest

from mhim_mil_amd import _lib as L
from tests import test_half_input_cpu as H
from tests import test_pure_window_cpu as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSED = b"workspace too small"
CENS = PW.FAKE + (1 << 43)
NEW = ("mhimx_head_surv_fwd_bwd", "mhimx_pure_window_run_surv", "mhimx_ragged_window_run_surv")


def _spec(n, alpha=0.4, eps=1e-7, null_at=None, risk=True):
    sp = L.SurvSpec(alpha=alpha, eps=eps, risk=(PW.FAKE + (1 << 44)) if risk else None)
    for b in range(n):
        sp.censor_dev[b] = None if b == null_at else CENS + 64 * b
    return sp


def _rbags(ns):
    bags = (L.RaggedWindowBag * len(ns))()
    for b, N in enumerate(ns):
        bags[b].X, bags[b].ldx, bags[b].N, bags[b].label_dev = H.X0 + (b << 33), 256, N, H.LAB0 + 64 * b
        bags[b].cnt = H._counts(N)
        bags[b].seeds = L.StepSeeds(1 + b, 2 + b, 3 + b, 4 + b)
    return bags


def _pure(ns, sp):
    lib = L.lib()
    r = lib.mhimx_pure_window_run_surv(None, C.byref(PW._cfg()), len(ns), PW._bags(ns), 1, PW.WS, 1, 1, L.X_F32, C.byref(sp) if sp is not None else None)
    return r, lib.mhimx_last_error()


def _ragged(ns, sp):
    lib = L.lib()
    r = lib.mhimx_ragged_window_run_surv(None, C.byref(H._rcfg(256)), len(ns), _rbags(ns), 1, H.WS, 1, 1, L.X_F32,
                                         C.byref(sp) if sp is not None else None)
    return r, lib.mhimx_last_error()


# ------------------------------------------------------------------------------------------------------------------ 1
def test_entry_points_are_declared_exported_and_bound():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.SYMBOLS
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mhimx_[a-z0-9_]+)\s*\(", code))
    assert declared == set(L.SYMBOLS) and all(hasattr(lib, n) for n in declared)
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == lib.mhimx_version() == 620
    # every entry point cites the reference lines it replaces
    tail = hdr[hdr.index("Survival training in the native train calls"):]
    for cite in ("engines/base_engine.py:395-441", "common_mil.py:14-48", "train_utils.py:8-37"):
        assert tail.count(cite) >= 3, cite


def test_the_spec_struct_and_the_pinned_structs():
    assert C.sizeof(L.SurvSpec) == 8 + 8 * 32 + 8
    assert (L.SurvSpec.alpha.offset, L.SurvSpec.eps.offset, L.SurvSpec.censor_dev.offset, L.SurvSpec.risk.offset) == (0, 4, 8, 264)
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mhimx_surv_spec;", hdr).group(1)
    assert re.findall(r"(\w+)(?:\[MHIMX_INFER_MAX\])?;", body) == ["eps", "censor_dev", "risk"] and "float alpha, eps;" in body
    assert L.INFER_MAX == 32
    # nothing that existing bindings pin moved
    assert C.sizeof(L.PureWindowBag) == 40 and C.sizeof(L.PureWindowLayout) == 8 * (10 + L.PURE_WINDOW_MAX)
    assert C.sizeof(L.RaggedWindowBag) == 32 + C.sizeof(L.StepCounts) + C.sizeof(L.StepSeeds) == 104
    assert C.sizeof(L.RaggedWindowLayout) == 8 * (12 + L.RAGGED_WINDOW_MAX)
    assert C.sizeof(L.StepLayout) == 96 and C.sizeof(L.WindowLayout) == 32 + 96
    # the C side pins the same numbers at compile time (csrc/surv_dev.hpp); where a C compiler is at hand the header is also compiled as C
    dev = open(os.path.join(ROOT, "mhim_mil_amd", "csrc", "surv_dev.hpp")).read()
    assert "static_assert(sizeof(mhimx_surv_spec) == 8 + 8 * MHIMX_INFER_MAX + 8" in dev
    import shutil
    import subprocess
    import tempfile
    if shutil.which("cc") is None:
        return
    src = '#include "mhimx.h"\n#include <stdio.h>\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(mhimx_step_cfg), sizeof(mhimx_surv_spec), ' \
          'sizeof(mhimx_pure_window_bag), sizeof(mhimx_ragged_window_bag));return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        cc = subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")], capture_output=True)
        if cc.returncode != 0:
            pytest.fail("the header does not compile as C: " + cc.stderr.decode()[-400:])
        got = [int(v) for v in subprocess.run([os.path.join(td, "s")], capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(L.StepCfg), 272, 40, 104], got


# ------------------------------------------------------------------------------------------------------------------ 2
CASES = [
    # (alpha, eps, null censor at, taken, word in the message)
    (0.0, 1e-7, None, True, PASSED), (1.0, 0.5, None, True, PASSED), (0.4, 1e-7, None, True, PASSED),
    (-0.01, 1e-7, None, False, b"alpha"), (1.01, 1e-7, None, False, b"alpha"), (float("nan"), 1e-7, None, False, b"alpha"),
    (0.4, 0.0, None, False, b"eps"), (0.4, 1.0, None, False, b"eps"), (0.4, -1e-7, None, False, b"eps"),
    (0.4, 1e-7, 0, False, b"bag 0: null censorship"), (0.4, 1e-7, 2, False, b"bag 2: null censorship"),
]


@pytest.mark.parametrize("alpha,eps,null_at,taken,word", CASES)
def test_new_refusals_before_any_device_call_and_their_mirror(alpha, eps, null_at, taken, word):
    from mhim_mil_amd import ops
    ns_p, ns_r = [700, 1, 33], [64, 97, 130]
    for who, run, ns in ((b"pure_window", _pure, ns_p), (b"ragged_window", _ragged, ns_r)):
        sp = _spec(len(ns), alpha, eps, null_at)
        r, msg = run(ns, sp)
        assert r < 0 and msg.startswith(who + b":") and word in msg, (who, r, msg)
        assert (PASSED in msg) == taken
        got = ops.surv_spec_ok(alpha, eps, [sp.censor_dev[b] for b in range(len(ns))], len(ns))
        assert got == taken, (who, alpha, eps, null_at, got)
    # a risk buffer is optional
    r, msg = _pure(ns_p, _spec(3, 0.4, 1e-7, None, risk=False))
    assert r < 0 and PASSED in msg


def test_null_spec_the_siblings_checks_and_the_head():
    lib = L.lib()
    r, msg = _pure([64], None)
    assert r < 0 and msg.startswith(b"pure_window:") and b"null survival description" in msg
    r, msg = _ragged([64], None)
    assert r < 0 and msg.startswith(b"ragged_window:") and b"null survival description" in msg
    # the siblings' own checks come first and keep their words
    bags = PW._bags([64, 0, 64])
    assert lib.mhimx_pure_window_run_surv(None, C.byref(PW._cfg()), 3, bags, 1, PW.WS, 1, 1, L.X_F32, C.byref(_spec(3))) < 0
    assert b"bag 1: N must be" in lib.mhimx_last_error()
    bags = PW._bags([64, 64])
    bags[1].label_dev = None
    assert lib.mhimx_pure_window_run_surv(None, C.byref(PW._cfg()), 2, bags, 1, PW.WS, 1, 1, L.X_F32, C.byref(_spec(2))) < 0
    assert b"bag 1: null label" in lib.mhimx_last_error()
    assert lib.mhimx_pure_window_run_surv(None, C.byref(PW._cfg()), 2, PW._bags([64, 64]), 1, PW.WS, 1, 1, 3, C.byref(_spec(2))) < 0      # x_dtype
    # the head building block: every refusal before the launch
    F = PW.FAKE
    base = dict(z=F, t=None, wp=F + 4096, bp=F + 8192, label=F + 12288, censor=F + 16384, E=512, C=4, alpha=0.4, eps=1e-7)
    for kw, word in [(dict(censor=None), b"censor"), (dict(label=None), b"null label"), (dict(alpha=1.5), b"alpha"), (dict(alpha=-0.5), b"alpha"),
                     (dict(eps=0.0), b"eps"), (dict(eps=1.0), b"eps"), (dict(C=17), b"bad dims"), (dict(C=0), b"bad dims"), (dict(z=None), b"null args")]:
        a = dict(base)
        a.update(kw)
        r = lib.mhimx_head_surv_fwd_bwd(None, a["z"], a["t"], a["wp"], a["bp"], a["label"], a["censor"], a["E"], a["C"], 1.0, 1.0, 0.0, 1.0,
                                        a["alpha"], a["eps"], F + 20480, F + 24576, None, F + 28672, None, None, 0)
        msg = lib.mhimx_last_error()
        assert r < 0 and msg.startswith(b"head_surv:") and word in msg, (kw, r, msg)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_the_trainer_refuses_what_the_calls_do_not_serve():
    from mhim_mil_amd.engine import FusedTrainer
    from mhim_mil_amd.mhim import MHIM
    # (the refusals are the first thing the constructor does: no flat buffer is made, no device needed)
    kw = dict(input_dim=256, n_classes=4, dropout=0.25, merge_enable=False, act="gelu", da_act="relu")
    for bad in (dict(baseline="dsmil"), dict(baseline="selfattn"), dict(baseline="attn", gated=True)):
        with pytest.raises(L.MhimxError, match="nll_surv"):
            FusedTrainer(MHIM(**kw, **bad), None, model="mhim_pure", loss="nll_surv")
    with pytest.raises(L.MhimxError, match="loss="):
        FusedTrainer(MHIM(**kw, baseline="attn"), None, model="mhim_pure", loss="cox")
    for a, e in ((1.5, 1e-7), (0.4, 0.0)):
        with pytest.raises(L.MhimxError, match="surv_alpha"):
            FusedTrainer(MHIM(**kw, baseline="attn"), None, model="mhim_pure", loss="nll_surv", surv_alpha=a, surv_eps=e)
