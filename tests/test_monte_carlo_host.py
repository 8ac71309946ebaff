"""CPU-side checks of the Monte-Carlo closed loop (isls_mc_closed_loop_*, include/isls_hip.h): the generator's known answers,
the ctypes mirror of the argument block, the exported symbols, the argument errors (all raised before anything touches a device)
and the register / scratch table of its kernels."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from isls import _capi as capi
from mc_reference import normals, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    """Philox4x32-10 of Random123: the published known-answer vectors, from the numpy restatement the GPU tests compare with"""
    got = philox4x32_10(*(np.array([c], dtype=np.uint32) for c in ctr), *key)
    assert tuple(int(g[0]) for g in got) == out


def test_normals_are_vectorised_consistently():
    """the restatement gives the same numbers for one counter and for an array of them, and the tails stop below 6.8 sigma"""
    z = normals(seed=11, problem=np.arange(3)[:, None, None], sample=np.arange(5)[None, :, None],
                step=np.arange(4)[None, None, :], n=6)
    assert z.shape == (3, 5, 4, 6)
    one = normals(seed=11, problem=2, sample=4, step=3, n=6)
    assert np.array_equal(one.reshape(6), z[2, 4, 3])
    assert np.all(np.abs(z) < 6.8)


def test_struct_layout_matches_header():
    """size and every offset of isls_mc_loop_args as gcc lays the header out == the ctypes mirror"""
    fields = [f[0] for f in capi.McLoopArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "isls_hip.h"\nint main(){printf("%zu\\n", sizeof(isls_mc_loop_args));' + \
          "".join(f'printf("%zu\\n", offsetof(isls_mc_loop_args, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == ctypes.sizeof(capi.McLoopArgs)
    assert got[1:] == [getattr(capi.McLoopArgs, f).offset for f in fields]


def test_symbols_and_version():
    lib = capi.load_hip_library()
    for s in ("isls_mc_closed_loop_f64", "isls_mc_closed_loop_f32", "isls_mc_work_elems"):
        assert hasattr(lib, s), s
        assert s in capi.EXPORTED
    assert lib.isls_version() == 107


def test_work_elems():
    lib = capi.load_hip_library()
    we = lambda *a: lib.isls_mc_work_elems(*a)                                        # noqa: E731
    assert we(3, 65, 7, 9, 3, 0) == 0                                                 # stage-local gains keep no history
    for bad in ((3, 65, 0, 9, 3, 1), (3, 65, 7, 17, 3, 1), (3, 65, 7, 9, 9, 1), (3, 65, 7, 0, 3, 1), (-1, 65, 7, 9, 3, 1), (3, 65, 7, 9, 3, 2)):
        assert we(*bad) == 0, bad
    for P, M, N, n, m in ((3, 65, 7, 9, 3), (1, 1, 1, 2, 1), (16, 4096, 50, 6, 3)):
        got = we(P, M, N, n, m, 1)
        assert got == capi.mc_work_elems(P, M, N, n, m, 1) >= P * M * N * n


def _valid():
    """an argument block that passes every check (the pointers are never followed: the errors come first)"""
    p = 0x1000
    return dict(P=2, M=5, N=4, n=2, m=1, model=capi.MODEL_LTI, K_form=0, model_par=p, K=p, k=p, x0=p)


@pytest.mark.parametrize("change", [
    dict(model_par=None), dict(K=None), dict(k=None),                                  # a NULL required pointer
    dict(x0=None),                                                                     # neither source of initial states
    dict(x0s=0x1000),                                                                  # both
    dict(w=0x1000, noise_std=0x1000),                                                  # explicit and drawn noise together
    dict(n=0), dict(n=17), dict(m=0), dict(m=9), dict(N=0), dict(P=-1), dict(M=-1), dict(K_form=2),   # dimensions outside the limits
    dict(K_form=1), dict(K_form=1, work=0x1000, work_elems=2 * 128 * 4 * 2 - 1),       # no / too small a work buffer
    dict(K_sb=-1),
])
def test_argument_errors_without_a_device(change):
    lib = capi.load_hip_library()
    for sfx in ("f64", "f32"):
        fn = getattr(lib, f"isls_mc_closed_loop_{sfx}")
        fn.restype = ctypes.c_int
        a = capi.McLoopArgs(**{**_valid(), **change})
        assert fn(ctypes.byref(a), None) == capi.ERR_ARG, (sfx, change)
        assert fn(None, None) == capi.ERR_ARG
    # an empty batch is no error and launches nothing
    a = capi.McLoopArgs(**{**_valid(), "P": 0})
    assert lib.isls_mc_closed_loop_f64(ctypes.byref(a), None) == capi.OK


def test_kernels_use_no_scratch():
    """tools/scan_kernels.py on the built library: every mc_closed_loop instantiation (the families, the run-time-dimension
    LTI, fp64 and fp32) keeps its state in registers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from scan_kernels import kernel_table
    tab = {k: v for k, v in kernel_table().items() if "mc_closed_loop" in k}
    assert len(tab) >= 2 * 15, sorted(tab)                                             # 14 families + the run-time LTI, two precisions
    bad = {k: v["scratch"] for k, v in tab.items() if v["scratch"] or v["spill"]}
    assert not bad, bad
