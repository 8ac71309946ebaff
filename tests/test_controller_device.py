"""SLS controller synthesis on the device (isls_sls_controller; SLS.controller / iSLS.controller): K = PHI_U Phi_x^-1 and
k = (I - K Su) du from block recursions through the dynamics instead of the dense transfer matrices and inverse.

CPU: a numpy restatement of the recursions against the reference's own controllers (g7) and the dense host path, and the
resource check of the new kernels.  GPU: the kernel against the dense host path (sls_dense.controller) over dimensions,
horizons, precisions and LTI / LTV dynamics, the class surfaces against the reference's outputs (g7, g9), full-size batches and
the routing rules (torch in / out, fp32 solvers, non-causal PHI_U)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, float(np.max(np.abs(b)))))


def lower_mask(N, n, m):
    """[N m, N n] True on and below the block diagonal."""
    t = np.arange(N * m) // m
    s = np.arange(N * n) // n
    return s[None, :] <= t[:, None]


def random_problem(rng, B, N, n, m, ltv, dtype=np.float64):
    """Causal PHI_U [B, N m, N n], du [B, N m] and dynamics A [Ba, Na, n, n], Bm [Ba, Na, n, m] close to a stable
    discretisation (spectral radius about 1, so that Phi_x stays moderate over N = 100 steps)."""
    Ba, Na = (B, N) if ltv else (1, 1)
    A = np.eye(n) + 0.1 / np.sqrt(n) * rng.standard_normal((Ba, Na, n, n))
    if not ltv:                                                 # one matrix for all steps: its powers must not grow
        A /= max(1.0, float(np.max(np.abs(np.linalg.eigvals(A[0, 0])))))
    Bm = 0.1 * rng.standard_normal((Ba, Na, n, m))
    PHI_U = 0.1 * rng.standard_normal((B, N * m, N * n)) * lower_mask(N, n, m)
    du = rng.standard_normal((B, N * m))
    return [x.astype(dtype) for x in (A, Bm, PHI_U, du)]


def dense_reference(A, Bm, PHI_U, du, b):
    from isls import sls_dense as dense
    N = PHI_U.shape[-2] // Bm.shape[-1]
    Ab, Bb = A[min(b, A.shape[0] - 1)].astype(np.float64), Bm[min(b, Bm.shape[0] - 1)].astype(np.float64)
    Sw, Su = dense.transfer_matrices_ltv(np.broadcast_to(Ab, (N,) + Ab.shape[-2:]), np.broadcast_to(Bb, (N,) + Bb.shape[-2:]))
    return dense.controller(Sw, Su, PHI_U[b].astype(np.float64), du[b].astype(np.float64))


def recursions(A, Bm, PHI_U, du):
    """numpy restatement of the kernel's algorithm for one problem (A [N or 1, n, n], Bm [N or 1, n, m])."""
    n, m = Bm.shape[-2], Bm.shape[-1]
    N = PHI_U.shape[0] // m
    At = lambda l: A[min(l, A.shape[0] - 1)]                                     # noqa: E731
    Bt = lambda l: Bm[min(l, Bm.shape[0] - 1)]                                   # noqa: E731
    P = lambda t, s: PHI_U[t * m:(t + 1) * m, s * n:(s + 1) * n]                 # noqa: E731
    X = {}
    for s in range(N):
        X[s, s] = np.eye(n, dtype=PHI_U.dtype)
        for l in range(s, N - 1):
            X[l + 1, s] = At(l) @ X[l, s] + Bt(l) @ P(l, s)
    K = np.zeros_like(PHI_U)
    for t in range(N):
        for s in range(t, -1, -1):
            acc = np.zeros((m, n), dtype=PHI_U.dtype)
            for l in range(s + 1, t + 1):
                acc += K[t * m:(t + 1) * m, l * n:(l + 1) * n] @ X[l, s]
            K[t * m:(t + 1) * m, s * n:(s + 1) * n] = P(t, s) - acc
    xd = np.zeros((N, n), dtype=PHI_U.dtype)
    for t in range(N - 1):
        xd[t + 1] = At(t) @ xd[t] + Bt(t) @ du[t * m:(t + 1) * m]
    return K, du - K @ xd.reshape(-1)


def fp32_tolerance(A, Bm, PHI_U, b):
    """Relative tolerance of an fp32 controller: an entry of K or k is a sum of at most N n products, each factor carrying
    the rounding of up to N steps of the recursions; bounded here by 4 N n eps32 times the growth max|Phi_x| of the problem
    (Phi_x from the fp64 dense path).  Measured errors of the numpy restatement in fp32 stay 100x or more below it."""
    from isls import sls_dense as dense
    N, n = PHI_U.shape[-1] // Bm.shape[-2], Bm.shape[-2]
    Ab, Bb = A[min(b, A.shape[0] - 1)].astype(np.float64), Bm[min(b, Bm.shape[0] - 1)].astype(np.float64)
    Sw, Su = dense.transfer_matrices_ltv(np.broadcast_to(Ab, (N,) + Ab.shape[-2:]), np.broadcast_to(Bb, (N,) + Bb.shape[-2:]))
    growth = max(1.0, float(np.max(np.abs(Sw + Su @ PHI_U[b].astype(np.float64)))))
    return 4.0 * N * n * float(np.finfo(np.float32).eps) * growth


# ---------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------
def test_recursions_reproduce_reference_controllers(golden):
    """The algorithm the kernel implements, in numpy, against the reference's K, k (g7: dense inverse in the reference) and
    against the dense host path on random LTV problems; the blocks above the diagonal are exactly 0."""
    for name in ("g7_sls_d1.npz", "g7_sls_d3.npz"):
        g = golden(name)
        for b in range(g["du"].shape[0]):
            K, k = recursions(g["A"][None], g["B"][None], g["phi_u"][b], g["du"][b])
            mask = lower_mask(int(g["N"]), g["A"].shape[0], g["B"].shape[1])
            assert rel(K * mask, g["K"][b] * mask) < 1e-12 and rel(k, g["k"][b]) < 1e-12
            assert not K[~mask].any()
    rng = np.random.default_rng(1)
    for (n, m, N) in ((2, 1, 7), (5, 2, 6), (9, 3, 5)):
        A, Bm, PHI_U, du = random_problem(rng, 2, N, n, m, ltv=True)
        K, k = recursions(A[1], Bm[1], PHI_U[1], du[1])
        Kd, kd = dense_reference(A, Bm, PHI_U, du, 1)
        assert rel(K, Kd * lower_mask(N, n, m)) < 1e-12 and rel(k, kd) < 1e-12


def test_controller_kernels_use_no_scratch():
    """Both phases of isls_sls_controller, every (n, dtype) instance, hold their state in registers (tools/scan_kernels.py)."""
    from isls import _capi as capi
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import scan_kernels
    finally:
        sys.path.pop(0)
    tab = scan_kernels.kernel_table(scan_kernels.DEFAULT_LIB)
    for fam in ("ctl_columns_kernel", "ctl_rows_kernel"):
        hit = {k: v for k, v in tab.items() if fam in k}
        assert len(hit) == 32, (fam, sorted(hit))                            # n = 1 .. 16, fp64 and fp32
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
    lib = capi.load_hip_library()
    import ctypes
    lib.isls_sls_controller_work_elems.restype = ctypes.c_int64
    for B, N, n in ((1, 1, 2), (3, 50, 6), (1024, 100, 9)):
        got = lib.isls_sls_controller_work_elems(ctypes.c_int32(B), ctypes.c_int32(N), ctypes.c_int32(n))
        assert got == capi.sls_controller_work_elems(B, N, n)


def test_controller_struct_layout_matches_header():
    import ctypes
    import subprocess
    import tempfile

    from isls import _capi as capi
    src = '#include <stdio.h>\n#include "isls_hip.h"\nint main(){printf("%zu\\n", sizeof(isls_sls_controller_args));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        size = int(subprocess.check_output([os.path.join(d, "s")]))
    assert size == ctypes.sizeof(capi.SlsControllerArgs)


# ---------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------
def run_kernel(A, Bm, PHI_U, du):
    """isls_sls_controller on device copies of the inputs (their dtype): K, k, flags as numpy."""
    import torch

    from isls import _capi as capi
    from isls.engine import kernels
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")    # noqa: E731
    B, R, Cn = PHI_U.shape
    N = R // Bm.shape[-1]
    K = torch.full((B, R, Cn), float("nan"), dtype=t(PHI_U).dtype, device="cuda")
    k = torch.full((B, R), float("nan"), dtype=K.dtype, device="cuda")
    flags = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    work = torch.empty(capi.sls_controller_work_elems(B, N, Bm.shape[-2]), dtype=K.dtype, device="cuda")
    kernels().sls_controller(t(A), t(Bm), t(PHI_U), t(du), K, k, flags, work, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return K.cpu().numpy(), k.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(2, 1), (6, 3), (9, 3), (4, 2), (5, 2)])
@pytest.mark.parametrize("N", [1, 2, 37, 100])
@pytest.mark.parametrize("ltv", [False, True])
def test_kernel_matches_dense_host_path(n, m, N, ltv):
    rng = np.random.default_rng(100 * n + 10 * m + N + ltv)
    B = 3
    A, Bm, PHI_U, du = random_problem(rng, B, N, n, m, ltv)
    mask = lower_mask(N, n, m)
    K, k, flags = run_kernel(A, Bm, PHI_U, du)
    assert (flags == 0).all()
    for b in range(B):
        Kd, kd = dense_reference(A, Bm, PHI_U, du, b)
        assert rel(K[b] * mask, Kd * mask) < 1e-10 and rel(k[b], kd) < 1e-10
        assert (K[b][~mask] == 0).all() and not np.signbit(K[b][~mask]).any()
    # fp32 entry point on the same problem rounded to fp32, against the fp64 dense path on those rounded inputs
    A32, B32, P32, d32 = (x.astype(np.float32) for x in (A, Bm, PHI_U, du))
    K32, k32, flags32 = run_kernel(A32, B32, P32, d32)
    assert (flags32 == 0).all()
    for b in range(B):
        Kd, kd = dense_reference(A32, B32, P32, d32, b)
        tol = fp32_tolerance(A32, B32, P32, b)
        assert rel(K32[b] * mask, Kd * mask) < tol and rel(k32[b], kd) < tol, tol
        assert (K32[b][~mask] == 0).all()


def make_sls(g, dtype=np.float64):
    import isls
    s = isls.SLS(g["A"].shape[0], g["B"].shape[1], int(g["N"]), dtype=dtype)
    s.AB = [g["A"], g["B"]]
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g7_sls_d1.npz", "g7_sls_d3.npz"])
def test_sls_controller_matches_reference(golden, name):
    g = golden(name)
    s = make_sls(g)
    K, k = s.controller(g["phi_u"], g["du"])
    assert isinstance(K, np.ndarray) and K.dtype == np.float64 and K.shape == g["K"].shape
    for b in range(g["du"].shape[0]):
        assert rel(K[b], g["K"][b]) < 1e-10 and rel(k[b], g["k"][b]) < 1e-10
        K1, k1 = s.controller(g["phi_u"][b], g["du"][b])
        assert K1.shape == g["K"][b].shape and rel(K1, g["K"][b]) < 1e-10 and rel(k1, g["k"][b]) < 1e-10
    assert (s.controller_flags == 0).all()


@pytest.mark.gpu
def test_isls_admm_controller_is_exact(golden):
    """isls_admm's PHI_U = [phi_u, 0] is non-zero only in block column 0: the recursions give K = PHI_U and k = du exactly."""
    import torch
    from test_isls_admm import arm_cfg, make_arm
    g = golden("g9_isls_admm.npz")
    s = make_arm(arm_cfg(), [0, 1])
    s.isls_admm(3, None, max_line_search=10, k_max=3, max_admm_iter=1, threshold=1e-4)      # engine.A: a linearisation
    PHI_U = np.zeros((2, 120, 360))
    PHI_U[:, :, :3] = g["phi_u"]
    K, k = s.controller(PHI_U, g["du"])
    assert (K == PHI_U).all() and (k == g["du"]).all()
    assert (s.controller_flags == 0).all()
    probe = np.random.default_rng(5).standard_normal(40 * 9)
    for b in range(2):
        assert rel(K[b] @ probe, g["ctl_K_probe"][b]) < 1e-9 and rel(k[b], g["ctl_k"][b]) < 1e-9
    Kt, kt = s.controller(torch.as_tensor(PHI_U, device="cuda"), torch.as_tensor(g["du"], device="cuda"))
    assert Kt.is_cuda and (Kt.cpu().numpy() == PHI_U).all() and (kt.cpu().numpy() == g["du"]).all()
    for b in range(2):
        x_t, u_t = s.get_trajectory_sls(g["mc_x0"][b], Kt[b], kt[b], problem=b)
        x_n, u_n = s.get_trajectory_sls(g["mc_x0"][b], K[b], k[b], problem=b)
        assert (x_t == x_n).all() and (u_t == u_n).all()


@pytest.mark.gpu
def test_full_size_di3d_batch():
    """Config 5's DI-3D at B = 8192, N = 50 from device tensors: two workspace chunks, every flag, 16 problems against the
    host path; two problems made non-causal take the host route."""
    import torch

    import isls
    from isls import sls_dense as dense
    B, N, n, m = 8192, 50, 6, 3
    g = np.load(os.path.join(ROOT, "tests", "golden", "g7_sls_d3.npz"))
    s = isls.SLS(n, m, N)
    s.AB = [g["A"], g["B"]]
    gen = torch.Generator(device="cuda").manual_seed(7)
    mask = torch.as_tensor(lower_mask(N, n, m), device="cuda")
    PHI_U = 0.1 * torch.randn(B, N * m, N * n, generator=gen, device="cuda", dtype=torch.float64) * mask
    du = torch.randn(B, N * m, generator=gen, device="cuda", dtype=torch.float64)
    bad = [5, 6000]
    for b in bad:
        PHI_U[b, 0, n] = 1e-3                                      # one entry right of block (0, 0)
    K, k = s.controller(PHI_U, du)
    assert K.is_cuda and K.dtype == torch.float64 and tuple(K.shape) == (B, N * m, N * n)
    expect = np.zeros(B, dtype=np.int32)
    expect[bad] = 1
    assert (s.controller_flags == expect).all()
    Sw, Su = s._transfer()
    for b in sorted(set(np.linspace(0, B - 1, 14).astype(int).tolist() + [B - 1, 4097]) | set(bad)):
        Kd, kd = dense.controller(Sw, Su, PHI_U[b].cpu().numpy(), du[b].cpu().numpy())
        Kb, kb = K[b].cpu().numpy(), k[b].cpu().numpy()
        if b in bad:
            assert (Kb == Kd).all() and (kb == kd).all()
        else:
            assert rel(Kb, Kd * lower_mask(N, n, m)) < 1e-10 and rel(kb, kd) < 1e-10, b


@pytest.mark.gpu
def test_full_size_arm_batch():
    """The 3R arm at B = 1024, N = 100 with a linearisation per problem in engine.A / engine.Bm (two workspace chunks)."""
    import torch

    import isls
    B, N, n, m = 1024, 100, 9, 3
    s = isls.iSLS(n, m, N, batch=B)
    rng = np.random.default_rng(11)
    A, Bm, _, _ = random_problem(rng, B, N, n, m, ltv=True)
    s.engine.A.copy_(torch.as_tensor(A))
    s.engine.Bm.copy_(torch.as_tensor(Bm))
    gen = torch.Generator(device="cuda").manual_seed(3)
    PHI_U = 0.1 * torch.randn(B, N * m, N * n, generator=gen, device="cuda", dtype=torch.float64) \
        * torch.as_tensor(lower_mask(N, n, m), device="cuda")
    du = torch.randn(B, N * m, generator=gen, device="cuda", dtype=torch.float64)
    K, k = s.controller(PHI_U, du)
    assert (s.controller_flags == 0).all()
    for b in (0, 1, 300, 511, 667, 668, 900, B - 1):
        P_, d_ = PHI_U[b:b + 1].cpu().numpy(), du[b:b + 1].cpu().numpy()
        Kd, kd = dense_reference(A[b:b + 1], Bm[b:b + 1], P_, d_, 0)
        assert rel(K[b].cpu().numpy(), Kd * lower_mask(N, n, m)) < 1e-10 and rel(k[b].cpu().numpy(), kd) < 1e-10, b


@pytest.mark.gpu
def test_controller_routing(golden):
    import torch

    from isls import sls_dense as dense
    g = golden("g7_sls_d3.npz")
    s64, s32 = make_sls(g), make_sls(g, np.float32)
    # torch in -> device tensors out, on the engine's device
    Kt, kt = s64.controller(torch.as_tensor(g["phi_u"], device="cuda"), torch.as_tensor(g["du"], device="cuda"))
    on_engine = torch.empty(0, device=s64.engine.device).device                  # 'cuda' resolved to its index
    assert isinstance(Kt, torch.Tensor) and Kt.device == on_engine and kt.device == on_engine
    # numpy in -> numpy float64 out
    K, k = s64.controller(g["phi_u"], g["du"])
    assert isinstance(K, np.ndarray) and K.dtype == np.float64 and k.dtype == np.float64
    assert (Kt.cpu().numpy() == K).all() and (kt.cpu().numpy() == k).all()
    # an fp32 solver keeps returning fp64 controllers
    K32, k32 = s32.controller(g["phi_u"], g["du"])
    assert K32.dtype == np.float64 and rel(K32, K) < 1e-10 and rel(k32, k) < 1e-10
    # a PHI_U that is not causal is flagged and takes the dense host route unchanged
    P = g["phi_u"].copy()
    P[1, 3, 40] = 0.25                                                         # row block 1, column block 6
    Kn, kn = s64.controller(P, g["du"])
    assert list(s64.controller_flags) == [0, 1]
    Kd, kd = dense.controller(s64.Sw, s64.Su, P[1], g["du"][1])
    assert (Kn[1] == Kd).all() and (kn[1] == kd).all()
    assert rel(Kn[0], g["K"][0]) < 1e-10
