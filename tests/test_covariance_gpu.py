"""isls_cov_closed_loop_* (csrc/covariance.hip) and its class surface on the device: the kernel against the numpy restatement
(tests/cov_reference.py) at every shape where the mapping can go wrong, its exact properties, the probabilities, its agreement with
the Monte-Carlo kernel on deterministic sigma points, and iSLS.covariance / SLS.covariance.

Tolerances: fp64 max-abs error <= 1e-10 max(1, |ref|_max) per output array, fp32 1e-4.  The fp32 bound was checked
before it was relied on: the restatement run in float32 on the CPU stays within 8.4e-6 (same measure) of the float64 one over all
cases of CASES and of test_every_operand_layout below (entries up to 8.9), so the format alone leaves a factor of 12 to the bound."""
import itertools

import numpy as np
import pytest
import torch

import isls_problems as P
import user_models as um
from cov_reference import closed_loop
from isls import _capi as capi
from isls import covariance

pytestmark = pytest.mark.gpu
TOL = {torch.float64: 1e-10, torch.float32: 1e-4}
NAMES = ("x_mean", "u_mean", "x_var", "u_var", "x_cov", "u_cov", "p_x", "p_u")


class Eng:
    """what covariance.run needs of an engine: dtype, device, kernels, host -> device"""

    def __init__(self, dtype=torch.float64):
        self.dtype, self.device = dtype, torch.device("cuda:0")
        self.kern = capi.Kernels(capi.library())

    def _t(self, x):
        if not isinstance(x, torch.Tensor):
            x = np.array(x)
        return torch.as_tensor(x, dtype=self.dtype, device=self.device).contiguous()


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


def make_case(seed, P_, N, n, m, ab="ltv", w="none", with_k=True, bounds=False):
    """Inputs of one case: A_t random with spectral norm in [0.7, 1.05], |B|, |K| <= 0.5; S0 = L L' positive semi-definite with
    min(2, n - 1) zero-variance coordinates (its rows and columns exactly zero); W none, one shared [n,n] or one per problem and
    step; A, B per problem and step or one shared pair."""
    rng = np.random.default_rng(seed)

    def contraction(*lead):
        G = rng.standard_normal(lead + (n, n))
        return G * (rng.uniform(0.7, 1.05, lead) / np.linalg.norm(G, 2, axis=(-2, -1)))[..., None, None]
    c = dict(A=contraction(P_, N) if ab == "ltv" else contraction(), K=rng.uniform(-0.5, 0.5, (P_, N, m, n)))
    c["B"] = rng.uniform(-0.5, 0.5, (P_, N, n, m) if ab == "ltv" else (n, m))
    c["k"] = rng.uniform(-0.5, 0.5, (P_, N, m)) if with_k else None
    L = rng.uniform(-1.0, 1.0, (P_, n, n))
    L[:, :min(2, n - 1)] = 0.0
    c["S0"] = L @ np.swapaxes(L, -1, -2)
    c["S0"][:, n - 1, max(n - 2, 0)] *= 1.0 + 2.0 ** -20       # ... and, for n > 2, not exactly symmetric: Sig_0 = (S0 + S0')/2 is tested
    if w == "shared":
        Lw = 0.2 * rng.uniform(-1.0, 1.0, (n, n))
        c["W"] = Lw @ Lw.T
    elif w == "step":
        Lw = 0.2 * rng.uniform(-1.0, 1.0, (P_, N, n, n))
        c["W"] = Lw @ np.swapaxes(Lw, -1, -2)
    else:
        c["W"] = None
    c["xhat"], c["uhat"] = rng.standard_normal((P_, N, n)), rng.standard_normal((P_, N, m))
    c["dx0"] = 0.1 * rng.standard_normal((P_, n))
    c["u_bounds"] = c["x_bounds"] = None
    if bounds:                                                 # two-sided per problem and step on u, one-sided per coordinate on x
        c["u_bounds"] = (c["uhat"] - rng.uniform(0.5, 3.0, (P_, N, m)), c["uhat"] + rng.uniform(0.5, 3.0, (P_, N, m)))
        c["x_bounds"] = (None, rng.uniform(0.0, 4.0, n))
    return c


def reference(c, dtype=np.float64, P_=None):
    return closed_loop(c["A"], c["B"], c["K"], c["S0"], k=c["k"], W=c["W"], xhat=c["xhat"], uhat=c["uhat"], dx0=c["dx0"],
                       u_bounds=c["u_bounds"], x_bounds=c["x_bounds"], dtype=dtype, P=P_)


def device(c, dtype=torch.float64, full=True, sel=None, **kw):
    """covariance.run on the case (sel: these problems only); the noise is given in the shape the caller would hold it in"""
    pick = lambda x, nd: x if x is None or sel is None or np.ndim(x) < nd else x[sel]      # noqa: E731
    N, m, n = c["K"].shape[-3:]
    bnd = lambda b: None if b is None else tuple(pick(s, 3) for s in b)                     # noqa: E731
    return covariance.run(Eng(dtype), pick(c["A"], 4), pick(c["B"], 4), pick(c["K"], 4), pick(c["k"], 3), N, n, m,
                          xhat=pick(c["xhat"], 3), uhat=pick(c["uhat"], 3), dx0=pick(c["dx0"], 2), x0_cov=pick(c["S0"], 3),
                          noise_cov=pick(c["W"], 4), u_bounds=bnd(c["u_bounds"]), x_bounds=bnd(c["x_bounds"]), full=full, **kw)


def check(got, ref, tol, rows=None):
    for name in NAMES:
        r, g = ref[name], getattr(got, name)
        assert (r is None) == (g is None), name
        if r is not None:
            r, g = (r, g) if rows is None else (r[rows], g[rows])
            err = rel(g, r)
            print(f"{name}: {err:.2e}")
            assert err <= tol, (name, err)


# the variants cycle through the shapes: every (A/B layout, W form, k, bounds) combination occurs, every shape runs both precisions
VARIANTS = list(itertools.product(("ltv", "shared"), ("none", "shared", "step"), (True, False), (False, True)))
CASES = [(n, m, N, P_) for (n, m) in ((2, 1), (6, 3), (9, 3)) for N in (1, 2, 13) for P_ in (1, 10, 11, 23)]


def case_of(idx):
    n, m, N, P_ = CASES[idx]
    ab, w, with_k, bounds = VARIANTS[(5 * idx) % len(VARIANTS)]
    return make_case(100 + idx, P_, N, n, m, ab=ab, w=w, with_k=with_k, bounds=bounds)


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"n{n}m{m}-N{N}-P{P_}" for n, m, N, P_ in CASES])
def test_kernel_matches_restatement(idx):
    """(n, m) x N in 1, 2, 13 (no multiple of a ring depth) x P in 1, 10, 11, 23 (at n = 6: one slot, one wavefront, one wavefront
    and a slot, a partial third), both precisions, the layouts of A / B / W / k / bounds cycling through the cases"""
    c = case_of(idx)
    ref = reference(c)
    for dtype in (torch.float64, torch.float32):
        check(device(c, dtype), ref, TOL[dtype])


@pytest.mark.parametrize("ab,w,with_k,bounds", VARIANTS)
def test_every_operand_layout(ab, w, with_k, bounds):
    """A, B per problem and step or one shared pair (both strides 0); W absent, shared [n,n], per step; k absent and present; with
    and without bounds -- the full cross at (6, 3), N = 13, P = 23"""
    c = make_case(7, 23, 13, 6, 3, ab=ab, w=w, with_k=with_k, bounds=bounds)
    check(device(c), reference(c), TOL[torch.float64])


def test_results_without_the_full_covariances():
    """full=False: the instantiation that writes no x_cov / u_cov gives the same vectors, bit for bit"""
    c = make_case(8, 11, 13, 6, 3, w="shared", bounds=True)
    a, b = device(c, full=True), device(c, full=False)
    assert b.x_cov is None and b.u_cov is None
    for name in ("x_mean", "u_mean", "x_var", "u_var", "p_x", "p_u"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_noise_per_problem_and_torch_operands():
    """noise_cov [P,n,n] is one matrix per problem at every step; torch operands stay on the device and give torch results"""
    c = make_case(9, 11, 5, 6, 3, w="none")
    rng = np.random.default_rng(1)
    Lw = 0.2 * rng.uniform(-1, 1, (11, 6, 6))
    Wp = Lw @ np.swapaxes(Lw, -1, -2)
    ref = reference(dict(c, W=Wp[:, None]))
    got = device(dict(c, W=Wp))
    check(got, ref, 1e-10)
    e = Eng()
    t = covariance.run(e, e._t(c["A"]), e._t(c["B"]), e._t(c["K"]), e._t(c["k"]), 5, 6, 3, xhat=e._t(c["xhat"]), uhat=e._t(c["uhat"]),
                       dx0=e._t(c["dx0"]), x0_cov=e._t(c["S0"]), noise_cov=e._t(Wp), full=True)
    assert isinstance(t.x_cov, torch.Tensor) and t.x_cov.is_cuda
    assert np.array_equal(t.x_cov.cpu().numpy(), got.x_cov) and np.array_equal(t.u_mean.cpu().numpy(), got.u_mean)
    assert np.array_equal(t.u_std.cpu().numpy(), got.u_std)


def test_active_mask_keeps_the_sentinel():
    """the whole first wavefront (10 problems at n = 6) and one more problem inactive: their outputs keep what they were created
    with (NaN), the others are the restatement's"""
    c = make_case(10, 23, 13, 6, 3, w="step", bounds=True)
    active = np.ones(23, dtype=np.int32)
    active[:10] = 0
    active[15] = 0
    got = device(c, active=active)
    on = np.flatnonzero(active)
    check(got, reference(c), 1e-10, rows=on)
    for name in NAMES:
        assert np.isnan(getattr(got, name)[active == 0]).all(), name
        assert np.isfinite(getattr(got, name)[on]).all(), name


# ---- 2. exact properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(2, 1), (6, 3), (9, 3)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_exact_properties(n, m, dtype):
    c = make_case(20 + n, 23, 13, n, m, w="step")
    r = device(c, dtype)
    assert np.array_equal(r.x_cov, np.swapaxes(r.x_cov, -1, -2)) and np.array_equal(r.u_cov, np.swapaxes(r.u_cov, -1, -2))
    assert np.array_equal(r.x_var, np.diagonal(r.x_cov, axis1=-2, axis2=-1))
    assert np.array_equal(r.u_var, np.diagonal(r.u_cov, axis1=-2, axis2=-1))
    assert (r.x_var >= 0).all() and (r.u_var >= 0).all()
    S0 = c["S0"].astype(np.float32 if dtype == torch.float32 else np.float64)
    assert n == 2 or not np.array_equal(S0, np.swapaxes(S0, -1, -2))
    assert np.array_equal(r.x_cov[:, 0], S0.dtype.type(0.5) * (S0 + np.swapaxes(S0, -1, -2)))
    # batch invariance: a problem inside the batch of 23 gives the bits of the same problem alone
    for b in (0, 10, 22):
        alone = device(c, dtype, sel=[b])
        for name in ("x_mean", "u_mean", "x_var", "u_var", "x_cov", "u_cov"):
            assert np.array_equal(getattr(alone, name)[0], getattr(r, name)[b]), (name, b)


@pytest.mark.parametrize("k_given", [False, True])
def test_no_spread_gives_exact_zeros_and_the_nominal(k_given):
    """S0 = 0, no W, k = 0 (absent or given as zeros), no initial deviation: every covariance exactly 0, the means the nominal"""
    c = make_case(30, 23, 13, 6, 3, w="none", with_k=False)
    c.update(S0=np.zeros((23, 6, 6)), dx0=None, k=np.zeros((23, 13, 3)) if k_given else None)
    r = device(c)
    for name in ("x_var", "u_var", "x_cov", "u_cov"):
        assert not getattr(r, name).any(), name
    assert np.array_equal(r.x_mean, c["xhat"]) and np.array_equal(r.u_mean, c["uhat"])


# ---- 3. probabilities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_probabilities(dtype):
    """bounds one- and two-sided, per problem and per step, infinite entries; at t = 0 coordinates 0 and 1 of x have no spread
    (sigma == 0): their probability is the indicator -- mean inside: 0, outside: 1, exactly on the bound: 0 -- and so has u_0 of
    problem 0, whose gain row reads those two coordinates only"""
    P_, N, n, m = 11, 13, 6, 3
    c = make_case(40, P_, N, n, m, w="shared")
    c["K"][0, 0, 0, 2:] = 0.0
    c["dx0"][3:5] = 0.0                                       # the means that will lie exactly on a bound: xhat_0 itself, a number
    c["xhat"][3:5, 0] = c["xhat"][3:5, 0].astype(np.float32)  # ... that both precisions (and the restatement) hold exactly
    plain = device(c, dtype)                                  # the means as the kernel rounds them: the bounds are put on them
    xm, um = plain.x_mean.astype(np.float64), plain.u_mean.astype(np.float64)
    assert not plain.x_var[:, 0, :2].any() and plain.x_var[:, 0, 2:].all() and plain.u_var[0, 0, 0] == 0 and plain.u_var[1:, 0].all()
    x_lo, x_hi = xm - 1.5, xm + 2.5                            # per problem and step
    x_lo[0, 0, 0], x_hi[0, 0, 0] = xm[0, 0, 0] - 1.0, xm[0, 0, 0] + 1.0          # inside
    x_hi[1, 0, 0] = xm[1, 0, 0] - 0.5                                            # above the upper bound
    x_lo[2, 0, 1] = xm[2, 0, 1] + 0.25                                           # below the lower bound
    x_lo[3, 0, 0] = xm[3, 0, 0]                                                  # exactly on the lower bound
    x_hi[4, 0, 1] = xm[4, 0, 1]                                                  # exactly on the upper bound
    x_lo[5], x_hi[6] = -np.inf, np.inf                                           # infinite sides
    u_hi = um + np.random.default_rng(2).uniform(0.1, 2.0, um.shape)             # one-sided: no lower bound at all
    u_hi[0, 0, 0] = um[0, 0, 0] - 1.0                                            # sigma == 0 and outside
    c["x_bounds"], c["u_bounds"] = (x_lo, x_hi), (None, u_hi)
    got, ref = device(c, dtype), reference(c)
    check(got, ref, TOL[dtype])
    assert (got.p_x >= 0).all() and (got.p_x <= 1).all() and (got.p_u >= 0).all() and (got.p_u <= 1).all()
    point = got.x_var == 0
    assert point[:, 0, :2].all() and set(np.unique(got.p_x[point])) <= {0.0, 1.0}
    assert got.p_x[0, 0, 0] == 0 and got.p_x[1, 0, 0] == 1 and got.p_x[2, 0, 1] == 1 and got.p_x[3, 0, 0] == 0 and got.p_x[4, 0, 1] == 0
    assert got.p_u[0, 0, 0] == 1
    # a lower bound alone is the mirror image
    c["u_bounds"] = (um - 1.0, None)
    check(device(c, dtype), reference(c), TOL[dtype])


# ---- 4. agreement with the Monte-Carlo kernel, deterministic ------------------------------------------------------------------------
def test_sigma_points_through_the_monte_carlo_kernel():
    """SLS on the 1-D double integrator, N = 6, fp64, stage-local gains of solve_dp.  The joint noise (dx_0, w_0 .. w_4) has
    dimension D = 12; its 2 D sigma points +-sqrt(D) L e_j (L L' = blockdiag(S0, W, .., W)) go through monte_carlo as explicit x0s
    and w.  The model is linear, so the second moments of the returned x, u about their means ARE Sig_t, Su_t up to rounding:
    this ties the step index of W_t (added behind step t) to the Monte-Carlo kernel's x_{t+1} = f(x_t, u_t) + w_t."""
    import isls
    cfg = P.config1(N=6)
    N, n, m = 6, 2, 1
    s = isls.SLS(n, m, N)
    s.AB = [cfg["A"], cfg["B"]]
    s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    K, k = s.solve_dp()
    rng = np.random.default_rng(5)
    L0, Lw = rng.uniform(-0.3, 0.3, (n, n)), rng.uniform(-0.05, 0.05, (n, n))
    S0, W = L0 @ L0.T, Lw @ Lw.T
    D = n * N
    Lj = np.zeros((D, D))
    Lj[:n, :n] = np.linalg.cholesky(S0)
    for t in range(N - 1):
        Lj[n * (t + 1):n * (t + 2), n * (t + 1):n * (t + 2)] = np.linalg.cholesky(W)
    pts = np.sqrt(D) * np.concatenate([Lj.T, -Lj.T])          # [2 D, D]: row j = +- sqrt(D) L e_j
    x0 = np.array([0.3, -0.1])
    w = np.zeros((1, 2 * D, N, n))
    w[0, :, :N - 1] = pts[:, n:].reshape(2 * D, N - 1, n)
    mc = s.monte_carlo(K, k, x0s=(x0 + pts[:, :n])[None], w=w, return_trajectories=True)
    cov = s.covariance(K, k, x0=x0, x0_cov=S0, noise_cov=W, full=True)
    for name, z, mean in (("x", mc.x[0], cov.x_mean[0]), ("u", mc.u[0], cov.u_mean[0])):
        mu = z.mean(axis=0)
        dz = z - mu
        second = np.einsum("sti,stj->tij", dz, dz) / (2 * D)
        err_m, err_c = rel(mean, mu), rel(getattr(cov, name + "_cov")[0], second)
        print(f"{name}: mean {err_m:.2e}, covariance {err_c:.2e}")
        assert err_m <= 1e-10 and err_c <= 1e-10, (name, err_m, err_c)
    assert cov.x_var[0, 1:].min() > 0                          # (the comparison is not one of zeros)


# ---- 5. the class surface -----------------------------------------------------------------------------------------------------------
def _car(model, batch=5, N=12):
    import isls
    cfg = P.config4(batch=batch, N=N, seed=0)
    s = isls.iSLS(4, 2, N, batch=batch)
    s.forward_model = model(cfg["dt"])
    s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in range(batch)])
    s.reset()
    s.nominal_values = np.stack(xs), np.stack(us)
    s.solve(max_iter=2)
    return s


@pytest.mark.parametrize("which", ["builtin", "custom"])
def test_isls_covariance_class_surface(which):
    """iSLS with models.CarSimple and with the Custom car of tests/user_models.py after two solve iterations, batch = 5, N = 12:
    covariance() is the restatement on model.get_AB(xhat, uhat) and iSLS.K, k; tightened is its formula"""
    from isls import models
    mk = (lambda dt: models.CarSimple(dt)) if which == "builtin" else (lambda dt: models.Custom(4, 2, [dt], um.CAR))
    s = _car(mk)
    B_, N, n, m = 5, 12, 4, 2
    xh, uh, K, k = s.x_nom, s.u_nom, s.K, s.k
    AB = [models.CarSimple(P.config4(batch=B_, N=N, seed=0)["dt"]).get_AB(xh[b], uh[b]) for b in range(B_)]
    A, Bm = np.stack([a for a, _ in AB]), np.stack([b for _, b in AB])
    x0 = xh[:, 0] + 0.01
    std0, wstd = np.array([0.05, 0.05, 0.02, 0.0]), 0.01
    got = s.covariance(x0=x0, x0_std=std0, noise_scale=wstd, u_bounds=(-0.6, 0.6), x_bounds=(None, 5.0), full=True)
    ref = closed_loop(A, Bm, K, np.diag(std0 * std0), k=k, W=wstd * wstd * np.eye(n), xhat=xh, uhat=uh, dx0=x0 - xh[:, 0],
                      u_bounds=(-0.6, 0.6), x_bounds=(None, 5.0), P=B_)
    check(got, ref, 1e-10)
    assert got.x_mean.shape == (B_, N, n) and got.u_cov.shape == (B_, N, m, m)
    # explicit gains and the matrix forms of the two spreads say the same
    again = s.covariance(K=K, k=k, x0=x0, x0_cov=np.diag(std0 * std0), noise_cov=wstd * wstd * np.eye(n), u_bounds=(-0.6, 0.6),
                         x_bounds=(None, 5.0), full=True)
    for name in NAMES:
        assert np.array_equal(getattr(got, name), getattr(again, name)), name
    sd = np.sqrt(got.u_var)
    psi = 0.5 * 0.6 / sd.max()                                 # half the box at the widest spread: nothing crosses
    lo, hi = got.tightened(-0.6, 0.6, psi)
    assert lo.shape == hi.shape == (B_, N, m) and np.array_equal(lo, -0.6 + psi * sd) and np.array_equal(hi, 0.6 - psi * sd)
    assert (lo <= hi).all() and (lo >= -0.6).all() and lo.max() > -0.6
    with pytest.raises(ValueError, match="cross"):
        got.tightened(-0.6, 0.6, 1.01 * 0.6 / sd.max())


def test_class_surface_errors():
    import isls
    from isls import models
    s = _car(models.CarSimple)
    N, n, m = 12, 4, 2
    with pytest.raises(ValueError, match=r"stage-local gains.*phi_u S0 phi_u'"):
        s.covariance(K=np.zeros((N * m, N * n)), k=np.zeros(N * m))
    with pytest.raises(ValueError, match=r"stage-local gains.*phi_u S0 phi_u'"):
        s.covariance(K=np.zeros((5, N * m, N * n)), k=np.zeros((5, N * m)))
    with pytest.raises(ValueError, match="not both"):
        s.covariance(x0_std=0.1, x0_cov=np.eye(n))
    with pytest.raises(ValueError, match="not both"):
        s.covariance(noise_scale=0.1, noise_cov=np.eye(n))
    with pytest.raises(capi.IslsError, match=r"families\.def.*\(6, 3\)"):
        covariance.run(Eng(), np.eye(5), np.zeros((5, 1)), np.zeros((3, 1, 5)), None, 3, 5, 1)
    # a forward model that is a Python callable: served with the caller's linearisation only
    c = isls.iSLS(2, 1, 6)
    c.forward_model = lambda x, u: x
    with pytest.raises(ValueError, match="get_AB"):
        c.covariance(K=np.zeros((6, 1, 2)), k=np.zeros((6, 1)), x0_std=0.1)
    cfg = P.config1(N=6)
    c.AB = [cfg["A"], cfg["B"]]
    r = c.covariance(K=np.zeros((6, 1, 2)), k=np.zeros((6, 1)), x0_std=0.1)
    assert r.x_var.shape == (1, 6, 2) and np.allclose(r.x_var[0, 0], 0.01) and not r.u_var.any()
