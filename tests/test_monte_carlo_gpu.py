"""GPU tests of the Monte-Carlo closed loop (isls_mc_closed_loop_*, isls/montecarlo.py): parity with the reference's recorded
trajectories (G7 noise-free, G13 under its seeded noise), with the CPU oracle on nonlinear models, with a numpy loop; the
generator against its numpy restatement; the statistics against the trajectories of the same launch; edges; a user model; the
class surface.  fp64 unless said otherwise; rel = max-abs error over max(1, |ref|_max), the project's measure."""
import numpy as np
import pytest
import torch

import isls_problems as P
import user_models as um
from isls import _capi as capi
from isls import montecarlo
from mc_reference import dense_loop, normals

pytestmark = pytest.mark.gpu
STEP_X0 = 0xffffffff
TILE = 8                                                       # kMcTile (csrc/monte_carlo.hpp) at the fast families' dimensions


class Eng:
    """what montecarlo.run needs of an engine: dtype, device, kernels, host -> device"""

    def __init__(self, dtype=torch.float64):
        self.dtype, self.device = dtype, torch.device("cuda:0")
        self.kern = capi.Kernels(capi.library())

    def _t(self, x):
        if not isinstance(x, torch.Tensor):
            x = np.array(x)                                     # a copy: golden arrays and broadcast views are read-only
        return torch.as_tensor(x, dtype=self.dtype, device=self.device).contiguous()


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


def lti_par(A, B):
    return np.concatenate([np.asarray(A).reshape(-1), np.asarray(B).reshape(-1)])


def causal(rng, P_, N, n, m, scale):
    """random dense causal K [P, N m, N n] (exact zeros right of block i) and k [P, N m]"""
    K = scale * rng.standard_normal((P_, N * m, N * n))
    for i in range(N):
        K[:, i * m:(i + 1) * m, (i + 1) * n:] = 0.0
    return K, scale * rng.standard_normal((P_, N * m))


def embed(K0, k0):
    """stage-local gains [P,N,m,n], [P,N,m] as a block-diagonal dense controller"""
    P_, N, m, n = K0.shape
    K = np.zeros((P_, N * m, N * n))
    for i in range(N):
        K[:, i * m:(i + 1) * m, i * n:(i + 1) * n] = K0[:, i]
    return K, k0.reshape(P_, N * m)


def run(dtype=torch.float64, **kw):
    model, par, K, k, N, n, m = (kw.pop(a) for a in ("model", "par", "K", "k", "N", "n", "m"))
    e = Eng(dtype)
    return montecarlo.run(e, model, e._t(par), K, k, N, n, m, **kw)


STATS = ("viol_u", "viol_x", "viol_any", "u_min", "u_max", "x_min", "x_max")


def same_bits(a, b, names):
    return all(np.array_equal(getattr(a, s), getattr(b, s)) for s in names)


def di3d(N=9):
    from isls.utils import get_double_integrator_AB
    A, B = get_double_integrator_AB(3, 2, 0.05)
    return dict(model=capi.MODEL_LTI, par=lti_par(A, B), N=N, n=6, m=3), A, B


# ---- 1. the reference's noise-free closed loops, all problems of a fixture in one launch ---------------------------------
@pytest.mark.parametrize("tag", ["d1", "d3"])
def test_reference_parity_dense_noise_free(golden, tag):
    g = golden(f"g7_sls_{tag}.npz")
    n, m = g["A"].shape[0], g["B"].shape[1]
    N = g["K"].shape[-1] // n
    kw = dict(model=capi.MODEL_LTI, par=lti_par(g["A"], g["B"]), K=g["K"], k=g["k"], N=N, n=n, m=m, x0s=g["mc_x0"],
              return_trajectories=True)
    r = run(**kw)
    ex, eu = np.max(np.abs(r.x - g["mc_x"])), np.max(np.abs(r.u - g["mc_u"]))
    print(f"g7_{tag}: P={g['K'].shape[0]} fp64 abs err x {ex:.2e} u {eu:.2e}")
    assert ex < 1e-9 and eu < 1e-8
    r32 = run(torch.float32, **kw)
    print(f"g7_{tag}: fp32 rel err x {rel(r32.x, g['mc_x']):.2e} u {rel(r32.u, g['mc_u']):.2e}")
    assert rel(r32.x, g["mc_x"]) < 1e-4 and rel(r32.u, g["mc_u"]) < 1e-4


# ---- 2. the CPU oracle on nonlinear models, about a nominal --------------------------------------------------------------
@pytest.mark.parametrize("name", ["arm", "car", "lti52"])
def test_oracle_parity_about_a_nominal(oracle, name):
    rng = np.random.default_rng(21)
    P_, M, N = 3, 65, 7
    n, m, model, par = {"arm": (9, 3, capi.MODEL_ARM3R, np.array([0.01])), "car": (4, 2, capi.MODEL_CAR, np.array([0.05])),
                        "lti52": (5, 2, capi.MODEL_LTI, None)}[name]
    K, k = causal(rng, P_, N, n, m, 0.05)
    if name == "lti52":                                        # a pair outside the fast families: run-time dimensions, absolute form
        A, B = np.eye(5) + 0.1 * rng.standard_normal((5, 5)), 0.3 * rng.standard_normal((5, 2))
        par, xhat, uhat = lti_par(A, B), None, None
        x0s = rng.standard_normal((P_, M, n))
    else:
        xhat, uhat = 0.3 * rng.standard_normal((P_, N, n)), 0.3 * rng.standard_normal((P_, N, m))
        x0s = xhat[:, :1] + 0.1 * rng.standard_normal((P_, M, n))
    ref_x, ref_u = np.zeros((P_, M, N, n)), np.zeros((P_, M, N, m))
    for p in range(P_):                                        # the oracle takes one controller and one nominal per call
        c = np.ascontiguousarray
        if name == "lti52":
            oracle.sls_closed_loop(c(A), c(B), c(K[p]), c(k[p]), c(x0s[p]), ref_x[p], ref_u[p])
        else:
            oracle.dense_closed_loop(model, par, c(K[p]), c(k[p]), c(x0s[p]), ref_x[p], ref_u[p], xhat=c(xhat[p]), uhat=c(uhat[p]))
    assert np.isfinite(ref_x).all() and np.abs(ref_x).max() < 1e3 and np.abs(ref_u).max() < 1e3   # the loop stays bounded
    r = run(model=model, par=par, K=K, k=k, N=N, n=n, m=m, x0s=x0s, xhat=xhat, uhat=uhat, return_trajectories=True)
    print(f"{name}: rel err x {rel(r.x, ref_x):.2e} u {rel(r.u, ref_u):.2e}")
    assert rel(r.x, ref_x) < 1e-10 and rel(r.u, ref_u) < 1e-10


# ---- 3. the reference's noisy closed loops (G13), its draws replayed as explicit noise -----------------------------------
def replay(seed, scale, shape, N):
    """the reference's draws: one np.random.normal(0, scale, x0.shape) per step -> w [M,N,n]"""
    np.random.seed(seed)
    w = np.stack([np.random.normal(0, scale, shape) for _ in range(N)])
    return np.ascontiguousarray(np.moveaxis(w.reshape((N, -1, shape[-1])), 0, 1))


def test_reference_parity_under_noise_di(golden):
    g = golden("g13_noise.npz")
    c = P.config1(50)
    base = dict(model=capi.MODEL_LTI, par=lti_par(c["A"], c["B"]), N=50, n=2, m=1, x0s=g["x0s"][None], return_trajectories=True)
    r = run(K=g["K"], k=g["k"], w=replay(123, 0.05, g["x0s"].shape, 50)[None], **base)
    print(f"g13 dp: rel err x {rel(r.x[0], g['dp_x']):.2e} u {rel(r.u[0], g['dp_u']):.2e}")
    assert rel(r.x[0], g["dp_x"]) < 1e-10 and rel(r.u[0], g["dp_u"]) < 1e-10
    r = run(K=np.zeros((50, 1, 2)), k=g["batch_us"], w=replay(124, 0.02, g["x0s"].shape, 50)[None], **base)
    print(f"g13 batch: rel err x {rel(r.x[0], g['batch_x']):.2e} u {rel(r.u[0], g['batch_u']):.2e}")
    assert rel(r.x[0], g["batch_x"]) < 1e-10 and rel(r.u[0], g["batch_u"]) < 1e-10


def test_reference_parity_under_noise_arm(golden):
    """Tolerance max(1e-10, 10 s): s = how far a numpy loop through the notebook's arm model moves when x0 and w are perturbed
    by 1e-15 relative (the rule of DESIGN 2 for the ill-conditioned arm), computed here."""
    g = golden("g13_noise.npz")
    f = P.arm_f(0.01)
    K, k = g["arm_K"], g["arm_us"]

    def loop(x0s, w):
        x, xs, us = x0s.copy(), [], []
        for i in range(100):
            u = x @ K[i].T + k[i]
            xs.append(x), us.append(u)
            x = np.asarray(f(x, u)) + w[:, i]
        return np.stack(xs, 1), np.stack(us, 1)
    base = dict(model=capi.MODEL_ARM3R, par=np.array([0.01]), K=K, k=k, N=100, n=9, m=3, return_trajectories=True)
    for seed, x0s, gx, gu in ((126, g["arm_x0"][None], g["arm_dp_x"], g["arm_dp_u"]), (127, g["arm_x0s2"], g["arm_dp2_x0"], g["arm_dp2_u0"])):
        shape = g["arm_x0"].shape if seed == 126 else x0s.shape
        w = replay(seed, 0.01, shape, 100)
        rng = np.random.default_rng(seed)
        a, b = loop(x0s, w), loop(x0s * (1 + 1e-15 * rng.standard_normal(x0s.shape)), w * (1 + 1e-15 * rng.standard_normal(w.shape)))
        s = max(rel(b[0], a[0]), rel(b[1], a[1]))
        tol = max(1e-10, 10 * s)
        r = run(x0s=x0s[None], w=w[None], **base)
        ex, eu = rel(r.x[0, 0], gx), rel(r.u[0, 0], gu)        # row 0 is the reference's row (tests/test_callbacks.py)
        print(f"g13 arm seed {seed}: sensitivity {s:.2e} tol {tol:.2e} rel err x {ex:.2e} u {eu:.2e}")
        assert ex < tol and eu < tol


# ---- 4. a dense controller under noise against a numpy loop ----------------------------------------------------------------
def test_dense_form_with_noise_against_numpy():
    rng = np.random.default_rng(4)
    base, A, B = di3d(N=9)
    P_, M, N, n, m = 2, 70, 9, 6, 3
    K, k = causal(rng, P_, N, n, m, 0.2)
    x0s, w = rng.standard_normal((P_, M, n)), 0.1 * rng.standard_normal((P_, M, N, n))
    r = run(K=K, k=k, x0s=x0s, w=w, return_trajectories=True, **base)
    for p in range(P_):
        x, u = dense_loop(lambda x_, u_: x_ @ A.T + u_ @ B.T, K[p], k[p], x0s[p], w[p])
        print(f"problem {p}: rel err x {rel(r.x[p], x):.2e} u {rel(r.u[p], u):.2e}")
        assert rel(r.x[p], x) < 1e-10 and rel(r.u[p], u) < 1e-10
    assert np.array_equal(r.w, w) and np.array_equal(r.x0, x0s)


@pytest.mark.parametrize("n,m", [(5, 2), (16, 8)])
def test_run_time_dimensions_about_a_nominal_with_noise(n, m):
    """Pairs outside the fast families run the instantiation with run-time dimensions; (16, 8) is the size at which the launcher
    halves the time tile.  About a nominal, explicit noise: the dense form against the numpy loop, stage-local gains against
    their dense embedding bit for bit, drawn noise replayed bit for bit."""
    rng = np.random.default_rng(40 + n)
    P_, M, N = 2, 70, 9
    A, B = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n), 0.3 * rng.standard_normal((n, m))
    base = dict(model=capi.MODEL_LTI, par=lti_par(A, B), N=N, n=n, m=m)
    K, k = causal(rng, P_, N, n, m, 0.05)
    xhat, uhat = 0.3 * rng.standard_normal((P_, N, n)), 0.3 * rng.standard_normal((P_, N, m))
    x0s, w = xhat[:, :1] + 0.1 * rng.standard_normal((P_, M, n)), 0.05 * rng.standard_normal((P_, M, N, n))
    r = run(K=K, k=k, x0s=x0s, w=w, xhat=xhat, uhat=uhat, return_trajectories=True, **base)
    for p in range(P_):
        x, u = dense_loop(lambda x_, u_: x_ @ A.T + u_ @ B.T, K[p], k[p], x0s[p], w[p], xhat[p], uhat[p])
        print(f"({n},{m}) problem {p}: rel err x {rel(r.x[p], x):.2e} u {rel(r.u[p], u):.2e}")
        assert rel(r.x[p], x) < 1e-10 and rel(r.u[p], u) < 1e-10
    K0, k0 = 0.1 * rng.standard_normal((P_, N, m, n)), 0.1 * rng.standard_normal((P_, N, m))
    kw = dict(x0=xhat[:, 0], x0_std=0.1, noise_scale=0.05, seed=9, samples=M, xhat=xhat, uhat=uhat, u_bounds=(-0.4, 0.4),
              return_trajectories=True, **base)
    r0 = run(K=K0, k=k0, **kw)
    Kd, kd = embed(K0, k0)
    r1 = run(K=Kd, k=kd, **kw)
    assert np.isfinite(r0.x).all() and r0.viol_any.sum() > 0
    assert np.array_equal(r0.x, r1.x) and np.array_equal(r0.u, r1.u) and np.array_equal(r0.w, r1.w) and same_bits(r0, r1, STATS)
    kw.pop("x0"), kw.pop("x0_std"), kw.pop("noise_scale"), kw.pop("samples")
    back = run(K=K0, k=k0, x0s=r0.x0, w=r0.w, **kw)
    assert np.array_equal(back.x, r0.x) and np.array_equal(back.u, r0.u) and same_bits(back, r0, STATS)


# ---- 5. the generator --------------------------------------------------------------------------------------------------------
def drawn(P_, M, seed=7, **kw):
    base, _, _ = di3d(N=8)
    rng = np.random.default_rng(5)
    K0, k0 = 0.2 * rng.standard_normal((3, 8, 3, 6)), 0.1 * rng.standard_normal((3, 8, 3))
    mean = rng.standard_normal((3, 6))
    std, nstd = np.array([.3, .2, .1, 0., .5, .4]), np.array([.05, .0, .02, .03, .01, .04])
    return run(K=K0[:P_], k=k0[:P_], x0=mean[:P_], x0_std=std, noise_scale=nstd, seed=seed, samples=M, return_trajectories=True,
               u_bounds=(-0.5, 0.5), x_bounds=(-1.5, None), **base, **kw), (mean, std, nstd, K0, k0, base)


def test_generator_matches_its_numpy_restatement_and_replays():
    r, (mean, std, nstd, K0, k0, base) = drawn(3, 130)
    p, s, i = np.arange(3)[:, None, None], np.arange(130)[None, :, None], np.arange(8)[None, None, :]
    w_ref = nstd * normals(7, p, s, i, 6)
    x0_ref = mean[:, None] + std * normals(7, p[:, :, 0], s[:, :, 0], STEP_X0, 6)
    print(f"draws: abs err w {np.max(np.abs(r.w - w_ref)):.2e} x0 {np.max(np.abs(r.x0 - x0_ref)):.2e}")
    assert np.max(np.abs(r.w - w_ref)) < 1e-12 and np.max(np.abs(r.x0 - x0_ref)) < 1e-12
    back = run(K=K0, k=k0, x0s=r.x0, w=r.w, return_trajectories=True, u_bounds=(-0.5, 0.5), x_bounds=(-1.5, None), **base)
    assert np.array_equal(back.x, r.x) and np.array_equal(back.u, r.u) and same_bits(back, r, STATS)
    assert r.viol_any.min() > 0                                # the bounds bite: the statistics compared are not all zero


def test_draws_do_not_depend_on_the_launch_shape():
    full, _ = drawn(3, 130)
    one, _ = drawn(1, 64)
    assert np.array_equal(one.w[0], full.w[0, :64]) and np.array_equal(one.x0[0], full.x0[0, :64])
    assert np.array_equal(one.x[0], full.x[0, :64])
    cut, _ = drawn(3, 130, chunk_problems=2, chunk_samples=50)
    assert all(np.array_equal(getattr(cut, a), getattr(full, a)) for a in ("x", "u", "w", "x0")) and same_bits(cut, full, STATS)
    other, _ = drawn(3, 130, seed=8)
    assert not np.array_equal(other.w, full.w)


def test_draws_are_standard_normal():
    base, _, _ = di3d(N=8)
    r = run(K=np.zeros((8, 3, 6)), k=np.zeros((8, 3)), x0=np.zeros(6), noise_scale=1.0, seed=3, samples=4096,
            return_trajectories=True, **base)
    z = r.w.reshape(-1)
    assert z.size == 4096 * 8 * 6
    print(f"mean {z.mean():.2e} (bound {5 / np.sqrt(z.size):.2e}) var {z.var():.5f}")
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1.0) < 0.02


# ---- 6. the statistics are those of the trajectories written ---------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 63, 65, 130])
@pytest.mark.parametrize("form", [0, 1])
def test_statistics_equal_those_of_the_trajectories(M, form):
    rng = np.random.default_rng(60 + M)
    base, _, _ = di3d(N=9)
    P_, N, n, m = 3, 9, 6, 3
    K0, k0 = 0.3 * rng.standard_normal((P_, N, m, n)), 0.2 * rng.standard_normal((P_, N, m))
    K, k = (K0, k0) if form == 0 else causal(rng, P_, N, n, m, 0.2)
    mean = 0.3 * rng.standard_normal((P_, n))
    kw = dict(K=K, k=k, x0=mean, x0_std=0.5, noise_scale=0.05, seed=M, samples=M, **base)
    # per-problem bounds at the 99.5th percentile of |u|, |x| of the same loops: a few samples beyond them per coordinate, roughly
    # a tenth of the samples with a violation somewhere (M = 1: the one sample is its own maximum somewhere)
    free = run(return_trajectories=True, **kw)
    u_hi = np.quantile(np.abs(free.u), 0.995, axis=(1, 2)).reshape(P_, 1, m)
    x_hi = np.quantile(np.abs(free.x), 0.995, axis=(1, 2)).reshape(P_, 1, n)
    kw.update(u_bounds=(-u_hi, u_hi), x_bounds=(-x_hi, x_hi))
    r = run(return_trajectories=True, **kw)
    vu, vx = (r.u < -u_hi[:, None]) | (r.u > u_hi[:, None]), (r.x < -x_hi[:, None]) | (r.x > x_hi[:, None])
    assert np.array_equal(r.viol_u, vu.sum(1)) and np.array_equal(r.viol_x, vx.sum(1))
    assert np.array_equal(r.viol_any, (vu.any((2, 3)) | vx.any((2, 3))).sum(1))
    assert np.array_equal(r.u_min, r.u.min(1)) and np.array_equal(r.u_max, r.u.max(1))
    assert np.array_equal(r.x_min, r.x.min(1)) and np.array_equal(r.x_max, r.x.max(1))
    print(f"M={M} form {form}: violation rate per problem {r.rate}")
    if M >= 63:
        assert r.viol_u.sum() > 0 and r.viol_x.sum() > 0 and r.viol_any.min() < M
    only = run(**kw)                                           # statistics only: every trajectory pointer NULL
    assert only.x is None and same_bits(only, r, STATS)


# ---- 7. edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, TILE + 1])
def test_edges(N):
    rng = np.random.default_rng(70 + N)
    base, A, B = di3d(N=N)
    P_, M, n, m = 3, 70, 6, 3
    K0, k0 = 0.3 * rng.standard_normal((P_, N, m, n)), 0.2 * rng.standard_normal((P_, N, m))
    x0s, w = rng.standard_normal((P_, M, n)), 0.1 * rng.standard_normal((P_, M, N, n))
    xhat, uhat = 0.3 * rng.standard_normal((P_, N, n)), 0.3 * rng.standard_normal((P_, N, m))
    kw = dict(x0s=x0s, w=w, return_trajectories=True, u_bounds=(-0.5, 0.5), **base)
    # stage-local gains against their block-diagonal embedding in the dense form, about a nominal: the same bits
    r0 = run(K=K0, k=k0, xhat=xhat, uhat=uhat, **kw)
    Kd, kd = embed(K0, k0)
    r1 = run(K=Kd, k=kd, xhat=xhat, uhat=uhat, **kw)
    assert np.array_equal(r0.x, r1.x) and np.array_equal(r0.u, r1.u) and same_bits(r0, r1, STATS)
    for p in range(P_):                                        # and both are the loop they claim to be
        x, u = dense_loop(lambda x_, u_: x_ @ A.T + u_ @ B.T, Kd[p], kd[p], x0s[p], w[p], xhat[p], uhat[p])
        assert rel(r1.x[p], x) < 1e-10 and rel(r1.u[p], u) < 1e-10
    # one controller for all problems (stride 0) against its copies
    for K, k in ((K0, k0), (Kd, kd)):
        shared = run(K=K[0], k=k[0], problems=P_, **kw)
        copies = run(K=np.repeat(K[:1], P_, 0), k=np.repeat(k[:1], P_, 0), **kw)
        assert np.array_equal(shared.x, copies.x) and np.array_equal(shared.u, copies.u) and same_bits(shared, copies, STATS)
    # the absolute form against a zero nominal
    for K, k in ((K0, k0), (Kd, kd)):
        a = run(K=K, k=k, **kw)
        z = run(K=K, k=k, xhat=np.zeros((P_, N, n)), uhat=np.zeros((P_, N, m)), **kw)
        assert np.array_equal(a.x, z.x) and np.array_equal(a.u, z.u) and same_bits(a, z, STATS)


# ---- 8. a user model ------------------------------------------------------------------------------------------------------------
def test_monte_carlo_custom_car_equals_builtin():
    import isls
    from isls import models
    cfg = P.config4(batch=2, N=200, seed=0)
    rng = np.random.default_rng(3)
    N, n, m = 200, 4, 2
    K, k = causal(rng, 2, N, n, m, 1e-3)
    res = []
    for mdl in (models.CarSimple(cfg["dt"]), models.Custom(4, 2, [cfg["dt"]], um.CAR)):
        s = isls.iSLS(n, m, N, batch=2)
        s.forward_model = mdl
        s.set_cost_variables(cfg["zs"][[0, 1]] if cfg["zs"].ndim == 3 else cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
        xs, us = zip(*[P.initial_nominal(cfg, b) for b in (0, 1)])
        s.reset()
        s.nominal_values = np.stack(xs), np.stack(us)
        res.append(s.monte_carlo(K, k, samples=70, x0_std=0.05, noise_scale=0.01, seed=5, u_bounds=(-0.3, 0.3),
                                 return_trajectories=True))
    a, b = res
    assert np.isfinite(a.x).all() and a.x.shape == (2, 70, N, n)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.u, b.u) and np.array_equal(a.w, b.w) and same_bits(a, b, STATS)


def test_callable_forward_model_is_refused():
    import isls
    s = isls.iSLS(4, 2, 20)
    s.forward_model = lambda x, u: x
    with pytest.raises(capi.IslsError, match="models.Custom"):
        s.monte_carlo(np.zeros((20, 2, 4)), np.zeros((20, 2)), samples=4)


# ---- 9. the class surface ---------------------------------------------------------------------------------------------------------
def test_sls_monte_carlo_class_surface(golden):
    import isls
    g = golden("g7_sls_d1.npz")
    P_, n, m = g["K"].shape[0], 2, 1
    N = g["K"].shape[-1] // n
    s = isls.SLS(n, m, N)
    s.AB = [g["A"], g["B"]]
    samples = 1000
    bound = g["upper_u"].reshape(P_, 1, 1)                    # the notebook's control bound, per problem
    # the fixture spreads the initial POSITION with variance var_x0 about 0 (tests/golden/make_golden.py); x0_std is one vector per
    # launch, so the problems of the fixture that share a variance go together
    for var in np.unique(g["var_x0"]):
        sel = np.flatnonzero(g["var_x0"] == var)
        s_ = lambda seed: s.monte_carlo(g["K"][sel], g["k"][sel], samples=samples, x0=np.zeros(2),   # noqa: E731
                                        x0_std=[np.sqrt(var), 0.0], seed=seed, u_bounds=(-bound[sel], bound[sel]))
        r, again, other = s_(1), s_(1), s_(2)
        assert r.viol_u.shape == (len(sel), N, m) and r.u_min.shape == (len(sel), N, m) and r.viol_x.shape == (len(sel), N, n)
        assert r.viol_u.min() >= 0 and r.viol_u.max() <= samples and np.all(r.viol_any <= samples) and r.samples == samples
        assert same_bits(r, again, STATS)
        assert not np.array_equal(r.u_max, other.u_max)
        print(f"var_x0 {var}: empirical violation rate per problem {r.rate} (reported, not asserted)")
