"""Host refusals of the step's tail (csrc/optim.hip: mhimx_optim_step, mhimx_head_fwd_bwd, mhimx_dsmil_head) - no GPU: a null stream and
fake, 16-byte aligned addresses; every refused call returns before anything is dereferenced or launched, and leaves its message in
mhimx_last_error."""
import ctypes as C

import pytest

from mhim_mil_amd import _lib as L

BASE = dict(p=4096, g=8192, m=12288, v=16384, n_train=1024, n_all=1024, step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
SLABS = dict(g_extra=20480, n_extra=2, extra_pitch=1024)

OPTIM_REFUSALS = {
    "empty mm_table": (dict(mm_table=32768, mm_len=0), b"momentum schedule"),
    "empty lr_table": (dict(lr_table=32768, lr_len=0), b"learning-rate schedule"),
    "n_all < n_train": (dict(n_all=1023), b"bad args"),
    "step 0 without step_dev": (dict(step=0), b"bad args"),
    "null p": (dict(p=None), b"bad args"),
    "null g": (dict(g=None), b"bad args"),
    "null m": (dict(m=None), b"bad args"),
    "null v": (dict(v=None), b"bad args"),
    "slab pitch below n_train": (dict(SLABS, extra_pitch=1020), b"gradient slabs"),
    "slab pitch not a multiple of 4": (dict(SLABS, extra_pitch=1026), b"gradient slabs"),
    "slab base unaligned": (dict(SLABS, g_extra=20484), b"gradient slabs"),
    "slabs without a base": (dict(SLABS, g_extra=None), b"gradient slabs"),
    "clipping without ws": (dict(clip_norm=1.0), b"workspace of 1024"),
    "clipping with a short ws": (dict(clip_norm=1.0, ws=32768, ws_floats=1023), b"workspace of 1024"),
}


def _refused(rc, text, what):
    msg = L.lib().mhimx_last_error()
    assert rc != 0, what
    assert msg and text in msg, (what, msg)


@pytest.mark.parametrize("what", sorted(OPTIM_REFUSALS))
def test_optim_step_refuses(what):
    bad, text = OPTIM_REFUSALS[what]
    a = L.OptimArgs(**dict(BASE, **bad))
    _refused(L.lib().mhimx_optim_step(None, C.byref(a)), text, what)


def test_optim_step_refuses_null_args():
    _refused(L.lib().mhimx_optim_step(None, None), b"null args", "null args")


def test_optim_step_refuses_an_overfull_fold_list():
    """mhimx_reduce_list.n > MHIMX_REDUCE_MAX: refused before a job is read (the 17th would lie outside the array), with and without
    clipping, and n < 0 as well."""
    assert L.REDUCE_MAX == 16
    for n in (L.REDUCE_MAX + 1, -1):
        for extra in (dict(), dict(clip_norm=1.0, ws=32768, ws_floats=1024)):
            lst = L.ReduceListC()
            lst.n = n
            a = L.OptimArgs(**dict(BASE, **extra), fold=C.addressof(lst))
            _refused(L.lib().mhimx_optim_step(None, C.byref(a)), b"bad reduction list", (n, extra))
            assert lst.n == n


def test_optim_step_of_nothing_is_a_no_op():
    """n_all = 0 returns 0 without a launch (this machine has no GPU: a launch would fail); with the step on the device too."""
    lib = L.lib()
    a = L.OptimArgs(**dict(BASE, n_train=0, n_all=0))
    assert lib.mhimx_optim_step(None, C.byref(a)) == 0
    a = L.OptimArgs(**dict(BASE, n_train=0, n_all=0, step=0, step_dev=32768))
    assert lib.mhimx_optim_step(None, C.byref(a)) == 0
    assert lib.mhimx_adam_ema(None, 4096, 8192, 12288, 16384, None, 0, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.9997, 1, None, None, 0) == 0


def _head(E=512, Cc=2, logits=4096 * 6, losses=4096 * 7, g_z=4096 * 8, z=4096, wp=4096 * 3):
    return L.lib().mhimx_head_fwd_bwd(None, z, None, wp, None, None, E, Cc, 1.0, 1.0, 0.0, 1.0, logits, losses, g_z, None, None, 0, None, None)


@pytest.mark.parametrize("what,kw,text", [
    ("C = 0", dict(Cc=0), b"bad dims"), ("C = 17", dict(Cc=17), b"bad dims"), ("C < 0", dict(Cc=-1), b"bad dims"),
    ("E = 0", dict(E=0), b"bad dims"), ("E < 0", dict(E=-4), b"bad dims"),
    ("null logits", dict(logits=None), b"null args"), ("null losses", dict(losses=None), b"null args"), ("null g_z", dict(g_z=None), b"null args"),
    ("null z", dict(z=None), b"null args"), ("null wp", dict(wp=None), b"null args")])
def test_head_refuses(what, kw, text):
    _refused(_head(**kw), text, what)


def _dsmil(lb=4096, li=8192, label=12288, Bs=16384, Cc=2, V=512, losses=20480, g_lb=24576, g_li=28672):
    return L.lib().mhimx_dsmil_head(None, lb, li, label, Bs, None, Cc, V, 1.0, 1.0, 0.0, 1.0, losses, g_lb, g_li, None, None)


@pytest.mark.parametrize("what,kw,text", [
    ("label without bag logits", dict(lb=None), b"label needs"), ("label without instance logits", dict(li=None), b"label needs"),
    ("label without g_logits_bag", dict(g_lb=None), b"label needs"), ("label without g_logits_ins", dict(g_li=None), b"label needs"),
    ("null losses", dict(losses=None), b"bad args"), ("null Bs", dict(Bs=None), b"bad args"), ("C = 0", dict(Cc=0), b"bad args"),
    ("C = 17", dict(Cc=17), b"bad args"), ("V = 0", dict(V=0), b"bad args")])
def test_dsmil_head_refuses(what, kw, text):
    _refused(_dsmil(**kw), text, what)
