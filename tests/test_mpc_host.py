"""CPU-side checks of the receding-horizon control step (isls_mpc_step_*, include/isls_hip.h): the exported symbols, the ctypes
mirror of the argument block, the argument errors (all returned before anything touches a device), the scratch table of its
kernels and the numpy restatement's shift."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from isls import _capi as capi
from mpc_reference import shift_hold, shift_naive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_version():
    lib = capi.load_hip_library()
    for s in ("isls_mpc_step_f64", "isls_mpc_step_f32"):
        assert hasattr(lib, s), s
        assert s in capi.EXPORTED
    assert lib.isls_version() == 107
    assert hasattr(capi.Kernels, "mpc_step")


def test_struct_layout_matches_header():
    """size and every offset of isls_mpc_step_args as gcc lays the header out == the ctypes mirror"""
    fields = [f[0] for f in capi.MpcStepArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "isls_hip.h"\nint main(){printf("%zu\\n", sizeof(isls_mpc_step_args));' + \
          "".join(f'printf("%zu\\n", offsetof(isls_mpc_step_args, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == ctypes.sizeof(capi.MpcStepArgs)
    assert got[1:] == [getattr(capi.MpcStepArgs, f).offset for f in fields]


def _valid():
    """an argument block that passes every check (the pointers are never followed: the errors come first)"""
    p = 0x1000
    return dict(B=3, N=4, n=2, m=1, model=capi.MODEL_LTI, model_par=p, xhat=p, uhat=p)


@pytest.mark.parametrize("change", [
    dict(xhat=None), dict(uhat=None), dict(model_par=None),                            # a NULL required pointer
    dict(N=0), dict(N=-3), dict(B=-1),
    dict(n=0), dict(n=17), dict(m=0), dict(m=9),                                       # dimensions outside the limits
    dict(par_sb=-1), dict(plant_sb=-1), dict(tab_sb=-1), dict(tab_next_sb=-1),         # a negative stride
    dict(x_meas_sb=-1), dict(u_out_sb=-1), dict(x_next_sb=-1),
    dict(tab=0x1000, W=0), dict(tab=0x1000, W=17), dict(tab=0x1000, W=-1),             # a table with a width outside [1, 16]
    dict(w=0x1000, noise_std=0x1000),                                                  # explicit and drawn noise together
])
def test_argument_errors_without_a_device(change):
    lib = capi.load_hip_library()
    for sfx in ("f64", "f32"):
        fn = getattr(lib, f"isls_mpc_step_{sfx}")
        fn.restype = ctypes.c_int
        a = capi.MpcStepArgs(**{**_valid(), **change})
        assert fn(ctypes.byref(a), None) == capi.ERR_ARG, (sfx, change)
        assert fn(None, None) == capi.ERR_ARG
    # an empty batch is no error and launches nothing
    a = capi.MpcStepArgs(**{**_valid(), "B": 0})
    assert lib.isls_mpc_step_f64(ctypes.byref(a), None) == capi.OK


def test_kernels_use_no_scratch():
    """tools/scan_kernels.py on the built library: every mpc_step instantiation (the families, the run-time-dimension LTI, fp64
    and fp32) keeps its state and its ring of rows in registers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from scan_kernels import kernel_table
    tab = {k: v for k, v in kernel_table().items() if "mpc_step" in k}
    assert len(tab) >= 2 * 15, sorted(tab)                                             # 14 families + the run-time LTI, two precisions
    bad = {k: v["scratch"] for k, v in tab.items() if v["scratch"] or v["spill"]}
    assert not bad, bad


@pytest.mark.parametrize("N", [1, 2, 3, 17])
def test_reference_shift_equals_roll_and_fix(N):
    rng = np.random.default_rng(N)
    for shape in ((4, N, 3), (2, N, 3, 5), (1, N, 1)):
        a = rng.standard_normal(shape)
        got = shift_hold(a)
        assert np.array_equal(got, shift_naive(a))
        assert np.array_equal(got[:, -1], a[:, -1]) and (N == 1 or np.array_equal(got[:, :-1], a[:, 1:]))
        assert N > 1 or np.array_equal(got, a)
