"""CPU-side checks of the closed-loop covariance (isls_cov_closed_loop_*, include/isls_hip.h; isls/covariance.py): the ctypes
mirror of the argument block, the exported symbols, the argument errors of the library and of the Python layer (all raised before
anything touches a device), the scratch table of the kernels, and the numpy restatement against plain matrix algebra."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from cov_reference import closed_loop, prob_outside
from isls import _capi as capi
from isls import covariance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_header():
    """size and every offset of isls_cov_args as gcc lays the header out == the ctypes mirror"""
    fields = [f[0] for f in capi.CovArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "isls_hip.h"\nint main(){printf("%zu\\n", sizeof(isls_cov_args));' + \
          "".join(f'printf("%zu\\n", offsetof(isls_cov_args, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == ctypes.sizeof(capi.CovArgs)
    assert got[1:] == [getattr(capi.CovArgs, f).offset for f in fields]


def test_symbols_and_version():
    lib = capi.load_hip_library()
    for s in ("isls_cov_closed_loop_f64", "isls_cov_closed_loop_f32"):
        assert hasattr(lib, s), s
        assert s in capi.EXPORTED
    assert lib.isls_version() == 107


def _valid():
    """an argument block that passes every check (the pointers are never followed: the errors come first)"""
    p = 0x1000
    return dict(P=2, N=4, n=2, m=1, A=capi.View(p, 0, 0), Bm=capi.View(p, 0, 0), K=p, S0=p)


@pytest.mark.parametrize("change,code", [
    (dict(A=capi.View(None, 0, 0)), capi.ERR_ARG), (dict(Bm=capi.View(None, 0, 0)), capi.ERR_ARG), (dict(K=None), capi.ERR_ARG),
    (dict(S0=None), capi.ERR_ARG), (dict(N=0), capi.ERR_ARG), (dict(P=-1), capi.ERR_ARG), (dict(K_sb=-1), capi.ERR_ARG),
    (dict(W=capi.View(0x1000, -1, 0)), capi.ERR_ARG),
    (dict(n=5, m=1), capi.ERR_UNSUPPORTED), (dict(n=2, m=3), capi.ERR_UNSUPPORTED), (dict(n=16, m=8), capi.ERR_UNSUPPORTED),
    (dict(P=0), capi.OK),                                                              # an empty batch launches nothing
])
def test_argument_errors_without_a_device(change, code):
    lib = capi.load_hip_library()
    for sfx in ("f64", "f32"):
        fn = getattr(lib, f"isls_cov_closed_loop_{sfx}")
        fn.restype = ctypes.c_int
        a = capi.CovArgs(**{**_valid(), **change})
        assert fn(ctypes.byref(a), None) == code, (sfx, change)
        assert fn(None, None) == capi.ERR_ARG


def test_kernels_use_no_scratch():
    """tools/scan_kernels.py on the built library: every cov_closed_loop instantiation (the pairs of families.def, with and
    without the full covariances and the probabilities, fp64 and fp32) keeps its state in registers"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from scan_kernels import kernel_table
    tab = {k: v for k, v in kernel_table().items() if "cov_closed_loop" in k}
    pairs = capi.supported_dims()
    assert len(tab) == 2 * 4 * len(pairs), sorted(tab)
    bad = {k: v["scratch"] for k, v in tab.items() if v["scratch"] or v["spill"]}
    assert not bad, bad
    assert all(v["wg"] == 64 for v in tab.values())


def test_python_argument_validation_without_a_device():
    N, n, m = 5, 6, 3
    assert covariance.stage_local(np.zeros((N, m, n)), N, n, m) is False
    assert covariance.stage_local(np.zeros((7, N, m, n)), N, n, m) is True
    for K in (np.zeros((N * m, N * n)), np.zeros((4, N * m, N * n))):
        with pytest.raises(ValueError, match=r"stage-local gains.*phi_u S0 phi_u'"):
            covariance.stage_local(K, N, n, m)
        with pytest.raises(ValueError, match=r"stage-local gains.*phi_u S0 phi_u'"):
            covariance.run(None, np.eye(n), np.zeros((n, m)), K, None, N, n, m)
    with pytest.raises(ValueError, match="expected stage-local gains"):
        covariance.stage_local(np.zeros((N, n, m)), N, n, m)
    # the two forms of a spread
    assert covariance.second_moment(None, None, n, "x") is None and covariance.second_moment(0.0, None, n, "x") is None
    assert np.array_equal(covariance.second_moment(0.5, None, n, "x"), 0.25 * np.eye(n))
    sd = np.arange(n) / 4.0
    assert np.array_equal(covariance.second_moment(sd, None, n, "x"), np.diag(sd ** 2))
    S = covariance.second_moment(np.stack([sd, 2 * sd]), None, n, "x")
    assert S.shape == (2, n, n) and np.array_equal(S[1], np.diag(4 * sd ** 2))
    C = np.arange(n * n, dtype=float).reshape(n, n)
    assert np.array_equal(covariance.second_moment(None, C, n, "x"), C)
    assert covariance.second_moment(0.0, np.zeros((3, N, n, n)), n, "w", N=N).shape == (3, N, n, n)
    with pytest.raises(ValueError, match="not both"):
        covariance.second_moment(0.1, C, n, "x")
    with pytest.raises(ValueError, match="not both"):
        covariance.run(None, np.eye(n), np.zeros((n, m)), np.zeros((N, m, n)), None, N, n, m, noise_scale=[0.1] * n, noise_cov=C)
    with pytest.raises(ValueError, match=r"expected \[n,n\], \[P,n,n\] with"):
        covariance.second_moment(None, np.zeros((3, N, n, n)), n, "x")                 # the initial spread has no time axis
    with pytest.raises(ValueError, match="standard deviations are"):
        covariance.second_moment(np.ones(n + 1), None, n, "x")
    with pytest.raises(ValueError, match="does not go with K"):
        covariance.run(None, np.eye(n), np.zeros((n, m)), np.zeros((N, m, n)), np.zeros((2, N, m)), N, n, m)
    # an (n, m) without a kernel names the pairs of families.def
    with pytest.raises(capi.IslsError, match=r"families\.def.*\(6, 3\)"):
        covariance.run(None, np.eye(5), np.zeros((5, 1)), np.zeros((N, 1, 5)), None, N, 5, 1)
    with pytest.raises(ValueError, match="disagree on the number of problems"):
        covariance.run(None, np.eye(n), np.zeros((n, m)), np.zeros((4, N, m, n)), None, N, n, m, x0_cov=np.zeros((3, n, n)))


def test_tightened():
    rng = np.random.default_rng(0)
    r = covariance.CovarianceResult(u_var=rng.uniform(0.0, 0.04, (3, 5, 2)))
    lo, hi = r.tightened(-1.0, [1.0, 2.0], 2.0)
    assert lo.shape == hi.shape == (3, 5, 2)
    assert np.array_equal(lo, -1.0 + 2.0 * np.sqrt(r.u_var)) and np.array_equal(hi, np.array([1.0, 2.0]) - 2.0 * np.sqrt(r.u_var))
    with pytest.raises(ValueError, match="cross"):
        r.tightened(-1.0, 1.0, 1.001 / np.sqrt(r.u_var.max()))


def test_restatement_against_matrix_algebra():
    """the restatement's ordered sums against numpy's matrix products, its W convention (W_t behind step t) and its sigma == 0 rule"""
    rng = np.random.default_rng(1)
    P_, N, n, m = 3, 7, 4, 2
    A, B = 0.4 * rng.standard_normal((P_, N, n, n)), rng.uniform(-0.5, 0.5, (P_, N, n, m))
    K, k = rng.uniform(-0.5, 0.5, (P_, N, m, n)), rng.standard_normal((P_, N, m))
    L = rng.standard_normal((P_, n, n))
    S0, W = L @ np.swapaxes(L, -1, -2), 0.1 * np.eye(n)
    xh, uh, d0 = rng.standard_normal((P_, N, n)), rng.standard_normal((P_, N, m)), rng.standard_normal((P_, n))
    r = closed_loop(A, B, K, S0, k=k, W=W, xhat=xh, uhat=uh, dx0=d0)
    for b in range(P_):
        Sig, d = S0[b], d0[b]
        for t in range(N):
            Phi = A[b, t] + B[b, t] @ K[b, t]
            assert np.allclose(r["x_cov"][b, t], Sig, atol=1e-12) and np.allclose(r["u_cov"][b, t], K[b, t] @ Sig @ K[b, t].T, atol=1e-12)
            assert np.allclose(r["x_mean"][b, t], xh[b, t] + d) and np.allclose(r["u_mean"][b, t], uh[b, t] + k[b, t] + K[b, t] @ d)
            Sig, d = Phi @ Sig @ Phi.T + W, Phi @ d + B[b, t] @ k[b, t]
    assert np.array_equal(r["x_cov"], np.swapaxes(r["x_cov"], -1, -2)) and r["p_x"] is None
    mu, var = np.array([0.0, 0.0, 0.0, 2.0, 1.0, 0.0]), np.array([1.0, 1.0, 4.0, 0.0, 0.0, 0.0])
    lo, hi = np.array([-np.inf, -1.0, -2.0, 0.0, 1.0, 0.5]), np.array([0.0, 1.0, np.inf, 1.0, 3.0, 2.0])
    p = prob_outside(mu, var, lo, hi)
    assert np.allclose(p[:3], [0.5, 0.31731050786291415, 0.15865525393145707], rtol=1e-14) and list(p[3:]) == [1.0, 0.0, 1.0]
