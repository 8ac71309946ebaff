"""CPU-side checks of the regularised gain pass's boundary: the two new argument structs mirror the header, the four entry
points are exported at an unchanged ISLS_VERSION, `isls.Regularization` validates its settings, and every REG instantiation of
the gain kernel holds no more scratch than its plain twin (tools/scan_kernels.py reads the code objects; no GPU)."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from isls import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_struct_layouts_match_header():
    src = ('#include <stdio.h>\n#include "isls_hip.h"\nint main(){printf("%zu %zu\\n", sizeof(isls_reg_args), '
           'sizeof(isls_reg_update_args)); return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert sizes == [ctypes.sizeof(capi.RegArgs), ctypes.sizeof(capi.RegUpdateArgs)]


def test_new_symbols_exported_at_the_same_version():
    lib = capi.load_hip_library()
    for name in ("isls_riccati_gain_reg_f64", "isls_riccati_gain_reg_f32", "isls_reg_update_f64", "isls_reg_update_f32"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED
    lib.isls_version.restype = ctypes.c_int
    assert lib.isls_version() == capi.ABI_VERSION == 107
    assert capi.ST_REG_MAX == 8


def test_argument_validation_without_gpu():
    lib = capi.load_hip_library()
    lib.isls_riccati_gain_reg_f64.restype = lib.isls_reg_update_f64.restype = ctypes.c_int
    g, r = capi.GainArgs(B=4, N=5, n=6, m=3), capi.RegArgs()
    assert lib.isls_riccati_gain_reg_f64(None, None, ctypes.byref(r), None) == capi.ERR_ARG
    assert lib.isls_riccati_gain_reg_f64(ctypes.byref(g), None, None, None) == capi.ERR_ARG
    assert lib.isls_riccati_gain_reg_f64(ctypes.byref(g), None, ctypes.byref(r), None) == capi.ERR_ARG      # null pointers
    assert lib.isls_reg_update_f64(None, None) == capi.ERR_ARG
    u = capi.RegUpdateArgs(B=4, mode=0, factor=1.6, mu_min=1e-6, mu_max=1e10)
    assert lib.isls_reg_update_f64(ctypes.byref(u), None) == capi.ERR_ARG                                   # null pointers


def test_regularization_validation():
    import isls
    r = isls.Regularization()
    assert (r.mu_init, r.mu_min, r.mu_max, r.factor, r.on, r.on_x) == (0.0, 1e-6, 1e10, 1.6, 'u', False)
    assert isls.Regularization(on='xu').on_x
    for kw in (dict(mu_init=-1.0), dict(mu_min=0.0), dict(mu_min=-1e-6), dict(mu_max=1e-9), dict(factor=1.0), dict(factor=0.5),
               dict(on='x'), dict(on=None), dict(mu_init=float("nan")), dict(mu_max=float("inf")), dict(factor="2"),
               dict(mu_init=1e11)):
        with pytest.raises(ValueError):
            isls.Regularization(**kw)


def test_schedule_reference_ladder():
    """reg_reference.Schedule: iLQG.m's ladder from mu = 0 and back."""
    from reg_reference import Schedule
    s = Schedule(1, np.float64)
    assert s.raise_(0) and s.mu[0] == 1e-6 and s.delta[0] == 1.6
    assert s.raise_(0) and s.delta[0] == 1.6 * 1.6 and s.mu[0] == 1e-6 * (1.6 * 1.6)
    s.lower(0)
    assert s.delta[0] == 1 / 1.6 and s.mu[0] == 1e-6 * (1.6 * 1.6) * (1 / 1.6)
    s.lower(0)
    assert s.mu[0] == 0.0                                       # below mu_min: zero
    s.mu[0], s.delta[0] = 9e9, 1.0
    assert not s.raise_(0) and s.mu[0] == 9e9 and s.delta[0] == 1.0


def test_reg_gain_kernels_use_no_more_scratch_than_their_twins():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import scan_kernels
    finally:
        sys.path.pop(0)
    tab = scan_kernels.kernel_table(scan_kernels.DEFAULT_LIB)
    # riccati_gain_kernel<T, NX, NU, D, MODE, FF, REC, ARR, LIN, RL, SH, REG>: the REG forms are dense with a record per trajectory
    reg_tail, plain_tail = "Li0ELb0ELb0ELb1EEEvNS_5GainPIT_EE", "Li0ELb0ELb0ELb0EEEvNS_5GainPIT_EE"
    reg = {k: v for k, v in tab.items() if k.startswith("_ZN4isls19riccati_gain_kernelI") and k.endswith(reg_tail)}
    assert len(reg) == 8 * 2 * 2 * 3 - 2 * 2, len(reg)         # 8 pairs x 2 dtypes x 2 modes x 3 forms, less the FF form of (9, 3)
    for k, v in reg.items():
        twin = tab[k[:-len(reg_tail)] + plain_tail]
        assert v["scratch"] <= twin["scratch"] and v["lds"] == twin["lds"], (k, v, twin)
    gen = {k: v for k, v in tab.items() if "gain_generic_kernel" in k}
    assert len(gen) == 4
    for k, v in gen.items():
        if "Lb1E" in k:
            assert v["scratch"] <= tab[k.replace("Lb1E", "Lb0E")]["scratch"], (k, v)
