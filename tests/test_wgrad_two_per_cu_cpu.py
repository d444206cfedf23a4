"""Host side of the weight gradient's kernel choice (csrc/wgrad.hip: mhimx_bag_wgrad_args.form, mhimx_bag_wgrad_form): which product kernel
a launch takes, which shapes fall back to the one-workgroup-per-CU kernel, and the argument checks - nothing here touches a GPU."""
import ctypes as C
import os
import re

import pytest

from mhim_mil_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                                                      # an aligned non-null address: the host-side checks never follow it


def _args(L_=9705, E=512, D=1024, ldx=None, N=10000, form=0, ximg=None, rows=FAKE):
    return L.BagWgrad(img=FAKE, X=FAKE, ldx=ldx or D, n_bag_rows=N, rows=rows, L=L_, E=E, D=D, C=FAKE, ldc=D, accumulate=0, ws=FAKE,
                      ws_floats=1 << 40, defer=None, ride_tail=0, ximg=ximg, form=form)


def _form(n_bags=1, **kw):
    return L.lib().mhimx_bag_wgrad_form(C.byref(_args(**kw)), n_bags)


def test_the_field_is_declared_last_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mhimx.h")).read()
    body = hdr[:hdr.index("} mhimx_bag_wgrad_args;")]
    assert re.search(r"\bint32_t form;", body[body.rindex("typedef struct"):])
    assert body.rindex("int32_t form;") > body.rindex("const void* ximg;")             # trailing: zero-initialised callers stay automatic
    assert L.BagWgrad._fields_[-1][0] == "form" and L.BagWgrad._fields_[-2][0] == "ximg"
    assert L.StepCfg._fields_[-1][0] == "wgrad_form"
    assert re.search(r"\bmhimx_bag_wgrad_form\s*\(", hdr) and "mhimx_bag_wgrad_form" in L.SYMBOLS
    assert int(re.search(r"#define MHIMX_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.lib().mhimx_version()   # additions only


def test_automatic_takes_two_per_cu_for_one_bag_of_whole_tiles():
    assert _form() == 2                                             # the benchmarked step: E = 512, D = 1024, 32 tiles x 16 slabs = 512 workgroups
    assert _form(E=128, D=128, L_=1, N=1) == 2
    assert _form(E=256, D=384, ldx=512) == 2                        # D % 256 == 128: this form alone
    assert _form(rows=None, L_=10000) == 2
    assert _form(form=2) == 2 and _form(form=1) == 1
    assert _form(L_=194000, N=200000, D=1536, form=2) == 2          # forced: any shape the kernel takes
    assert _form(L_=2000, N=2000, E=512, D=256) == 2 and _form(L_=600, N=600, E=512, D=512) == 2   # a single round of a smaller grid


@pytest.mark.parametrize("kw, n_bags", [
    (dict(), 2), (dict(), 8),                                       # the launch of an accumulation window's bags
    (dict(ximg=FAKE, rows=None, L_=10000), 1),                      # both operands as images
    (dict(form=1), 1),
    (dict(L_=194000, N=200000, D=1536), 1),                         # more workgroups than are resident at once: 48 tiles x 64 slabs
    (dict(L_=50000, N=50000, E=1536, D=512), 1),                    # 48 tiles x 17 slabs
    (dict(L_=9705, E=512, D=1536), 1),                              # 48 tiles x 11 slabs
])
def test_what_stays_on_the_one_per_cu_kernel(kw, n_bags):
    assert _form(n_bags, **kw) == 1


@pytest.mark.parametrize("kw", [
    dict(D=192), dict(D=1000), dict(D=64), dict(E=96), dict(E=64), dict(L_=0), dict(ldx=1022), dict(D=1024, ldx=512),
    dict(N=1 << 21, D=1024),                                        # 2^21 rows x 4 KiB: row offsets no longer fit 32 bits
    dict(form=3), dict(form=-1),
    dict(form=1, D=384, ldx=512),                                   # forced forms do not fall back
    dict(form=2, ximg=FAKE, rows=None, L_=10000),
])
def test_shapes_no_kernel_takes(kw):
    assert _form(**kw) < 0


def test_forced_form_two_is_refused_for_a_window():
    assert _form(2, form=2) < 0
    assert _form(2, D=384, ldx=512) < 0                             # automatic: the window's kernel needs D % 256 == 0
    assert _form(0) < 0 and _form(9) < 0


@pytest.mark.parametrize("kw, word", [
    (dict(form=3), b"form"), (dict(form=2, ximg=FAKE, rows=None, L_=10000), b"form 2"), (dict(form=1, D=384, ldx=512), b"D %"),
    (dict(D=192), b"D %"),
])
def test_the_launch_refuses_them_before_it_touches_the_device(kw, word):
    lib = L.lib()
    assert lib.mhimx_bag_wgrad(None, C.byref(_args(**kw))) < 0
    assert word in lib.mhimx_last_error(), lib.mhimx_last_error()


def test_workspace_plan_of_a_half_tile_width_is_that_of_the_widened_one():
    lib = L.lib()
    for L_, E, D in ((9705, 512, 1024), (345, 256, 384), (2045, 256, 384), (32, 128, 128), (219, 2048, 4096)):
        Dw = -(-D // 256) * 256
        assert lib.mhimx_wgrad_ws_floats(L_, E, D) * Dw == lib.mhimx_wgrad_ws_floats(L_, E, Dw) * D
    assert lib.mhimx_wgrad_ws_floats(9705, 512, 1024) == 16 * 512 * 1024          # the benchmarked step keeps its 16 slabs
