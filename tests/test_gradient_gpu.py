"""iSLS.gradient on the device against its numpy restatement (grad_reference.py): the costate sweep for built-in, user-written and
table models at the fast and a generic pair, the parameter and table directions, masks, repeatability, the solver state it must
leave alone, and what the numbers mean at a converged solve.  f64 bound: 1e-9 of each array's largest entry (the end-to-end bound
of the augmented-Lagrangian tests for sums of this length); f32: 1e-4, the bound the user-cost expansion tests state."""
import numpy as np
import pytest
import torch

from isls import _capi as capi
from isls import Box, Regularization, costs, iSLS, models
from isls.engine import kernels

import al_reference as al
import grad_reference as gr
import table_models as tm
import user_models as um
from test_gradient_host import TRACK, WINDY, quad_problem

pytestmark = pytest.mark.gpu

ALL = ("u", "x0", "cost_params", "model_params", "cost_table", "model_table")


def check(got, ref, names, tol=1e-9, what=""):
    for k in names:
        a, b = np.asarray(getattr(got, k), dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        err, scale = np.abs(a - b).max(initial=0.0), np.abs(b).max(initial=0.0)
        print(f"{what} {k}: max |device - restatement| {err:.3e}, max |restatement| {scale:.3e}")
        assert err <= tol * scale, (what, k, err, scale)


def lti_problem(rng, n, m, N, B, dtype=np.float64):
    """A stable random LTI pair, a via-point cost with a mid-horizon and a terminal target, a rolled-out random nominal"""
    A = np.eye(n) + 0.1 * rng.standard_normal((n, n))
    Bm = 0.3 * rng.standard_normal((n, m))
    zs, Qs = rng.standard_normal((2, n)), np.stack([np.diag(1.0 + rng.random(n)), 10 * np.eye(n)])
    seq = np.zeros(N, dtype=np.int32)
    seq[N - 1] = 1
    u = rng.standard_normal((B, N, m))
    x = np.stack([gr.rollout(gr.lti_f(A, Bm), rng.standard_normal(n), u[b], np.zeros(0)) for b in range(B)])
    q = iSLS(n, m, N, batch=B, dtype=dtype)
    q.forward_model = models.LTI(A, Bm)
    q.set_quadratic_cost(zs, Qs, seq, 0.1)
    q.nominal_values = x, u
    return q, A, Bm, gr.via_cost(zs, Qs, seq, 0.1), x, u


@pytest.mark.parametrize("n, m", [(2, 1), (6, 2), (9, 3), (5, 2)])
@pytest.mark.parametrize("N, B", [(2, 65), (5, 3), (70, 1)])
def test_sweep_lti_every_pair_and_shape(n, m, N, B):
    """costate, u, x0, cost of a built-in LTI model with the via-point cost: the extremes of n + m, the README's pair and a generic
    pair; one transition, an odd short horizon, a long one; fewer, odd and more trajectories than a wavefront's slots"""
    rng = np.random.default_rng(100 * n + m + N)
    q, A, Bm, c, x, u = lti_problem(rng, n, m, N, B)
    g = q.gradient()
    ref = gr.batch(gr.lti_f(A, Bm), c, x, u, np.zeros(0), np.zeros(0))
    check(g, ref, ("cost", "costate", "u", "x0"), what=f"lti ({n},{m}) N={N} B={B}")
    assert g.model_params is None and g.cost_table is None
    assert np.array_equal(g.x0, g.costate[:, 0])
    g2 = q.gradient(as_tensors=True)                           # repeatability: the same bits, and tensors on the device
    assert g2.u.is_cuda and np.array_equal(g2.u.cpu().numpy(), g.u) and np.array_equal(g2.costate.cpu().numpy(), g.costate)


@pytest.mark.parametrize("n, m", [(2, 1), (6, 2), (9, 3), (5, 2)])
def test_sweep_f32(n, m):
    rng = np.random.default_rng(7 * n + m)
    q, A, Bm, c, x, u = lti_problem(rng, n, m, 5, 3, dtype=np.float32)
    ref = gr.batch(gr.lti_f(A, Bm), c, x, u, np.zeros(0), np.zeros(0))
    check(q.gradient(), ref, ("cost", "costate", "u", "x0"), tol=1e-4, what=f"f32 lti ({n},{m})")


def test_sweep_car_and_shared_pair_and_mask():
    """CarSimple (a nonlinear built-in); a caller's shared pair through the AB setter (batch stride 0) against per-trajectory A, B;
    and the mask of the entry point: masked trajectories keep their sentinel bits"""
    rng = np.random.default_rng(3)
    N, B = 5, 3
    u = 0.5 * rng.standard_normal((B, N, 2))
    x0 = np.concatenate([rng.standard_normal((B, 2)), 1.0 + rng.random((B, 1)), 1.0 + rng.random((B, 1))], axis=1)
    x = np.stack([gr.rollout(gr.car_f, x0[b], u[b], np.array([0.1])) for b in range(B)])
    zs, Qs, seq = rng.standard_normal((1, 4)), np.eye(4)[None] * 2.0, np.zeros(N, dtype=np.int32)
    q = iSLS(4, 2, N, batch=B)
    q.forward_model = models.CarSimple(0.1)
    q.set_quadratic_cost(zs, Qs, seq, 0.1)
    q.nominal_values = x, u
    c = gr.via_cost(zs, Qs, seq, 0.1)
    check(q.gradient(), gr.batch(gr.car_f, c, x, u, np.array([0.1]), np.zeros(0)), ("cost", "costate", "u", "x0"), what="car")
    # a caller's shared pair: the sweep reads it with stride 0
    A, Bm = np.eye(4) + 0.1 * rng.standard_normal((4, 4)), rng.standard_normal((4, 2))
    q.AB = A, Bm
    ref = gr.batch(gr.car_f, c, x, u, np.array([0.1]), np.zeros(0), A=np.broadcast_to(A, (N, 4, 4)), Bm=np.broadcast_to(Bm, (N, 4, 2)))
    shared = q.gradient()
    check(shared, ref, ("costate", "u", "x0"), what="shared pair")
    q.AB = np.broadcast_to(A, (B, N, 4, 4)).copy(), np.broadcast_to(Bm, (B, N, 4, 2)).copy()
    per = q.gradient()
    assert np.array_equal(per.costate, shared.costate) and np.array_equal(per.u, shared.u)
    # the mask
    e, kern = q.engine, kernels()
    lam, gu, gx0 = (torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((B, N, 4), (B, N, 2), (B, 4)))
    on = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    kern.adjoint_sweep(e.A, e.Bm, e.c0x, e.c0u, lam, gu, gx0, active=on, stream=torch.cuda.current_stream().cuda_stream)
    assert (lam[1] == 7.0).all() and (gu[1] == 7.0).all() and (gx0[1] == 7.0).all()
    assert np.array_equal(lam[[0, 2]].cpu().numpy(), per.costate[[0, 2]]) and np.array_equal(gx0[[0, 2]].cpu().numpy(), per.x0[[0, 2]])


@pytest.mark.parametrize("per_traj, N, B", [(False, 5, 3), (True, 70, 3), (False, 2, 65)])
def test_quadrotor_params_and_tracking_table(per_traj, N, B):
    """models.Custom (P = 5) with the tracking cost (P = 2, W = 8): every entry, shared and per-trajectory parameters / tables"""
    rng = np.random.default_rng(11 + N)
    x0, u, tab = quad_problem(rng, N, B)
    mpar = um.QUAD_PAR * (1 + 0.1 * rng.random((B, 5))) if per_traj else um.QUAD_PAR.copy()
    cpar = np.array([0.05, 2.0]) * (1 + rng.random((B, 2))) if per_traj else np.array([0.05, 2.0])
    ctab = tab if per_traj else tab[0]
    x = np.stack([gr.rollout(gr.quad_f, x0[b], u[b], mpar[b] if per_traj else mpar) for b in range(B)])
    q = iSLS(6, 2, N, batch=B)
    q.forward_model = models.Custom(6, 2, mpar, um.QUAD)
    q.cost_function = costs.Custom(6, 2, cpar, TRACK, table=ctab)
    q.nominal_values = x, u
    want = ("u", "x0", "cost_params", "model_params", "cost_table")
    g = q.gradient(wrt=want)
    ref = gr.batch(gr.quad_f, gr.track_cost, x, u, mpar, cpar, None, ctab)
    check(g, ref, ("cost", "costate") + want, what=f"quad per_traj={per_traj} N={N} B={B}")
    assert g.model_table is None
    g2 = q.gradient(wrt=want)
    assert all(np.array_equal(getattr(g, k), getattr(g2, k)) for k in ("cost", "costate") + want)   # no atomics: the same bits
    only = q.gradient(wrt=("cost_table", "model_params"))      # a launch of the table directions alone gives the same bits
    assert only.u is None and np.array_equal(only.cost_table, g.cost_table) and np.array_equal(only.model_params, g.model_params)


POLY = """template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {
    S c = u[0] * u[0];
    for (int k = 0; k < ISLS_TEST_P; ++k) c += par[k] * x[k % 2] * x[(k + 1) % 2] * P(k + 1);
    return c;
}"""


@pytest.mark.parametrize("P", [1, 16])
def test_fewest_and_most_parameters(P):
    rng = np.random.default_rng(P)
    q, A, Bm, _, x, u = lti_problem(rng, 2, 1, 5, 3)
    par = rng.standard_normal((3, P))
    q.cost_function = costs.Custom(2, 1, par, f"#define ISLS_TEST_P {P}\n" + POLY + "\n#undef ISLS_TEST_P\n")
    q.nominal_values = x, u

    def c(x_, u_, p, row, t, N):
        return u_[0] * u_[0] + sum(p[k] * x_[k % 2] * x_[(k + 1) % 2] * (k + 1) for k in range(P))
    check(q.gradient(wrt=("u", "cost_params")), gr.batch(gr.lti_f(A, Bm), c, x, u, np.zeros(0), par), ("cost", "costate", "u", "cost_params"),
          what=f"P={P}")


@pytest.mark.parametrize("per_traj", [False, True])
def test_table_model_without_parameters(per_traj):
    """the LTV table model: P = 0, W = 16, more steps than lanes; row N-1 of the table's gradient is exactly 0"""
    rng = np.random.default_rng(2)
    N, B = 70, 3
    mtab = tm.ltv_table(rng, N, B if per_traj else None, scale=0.05)
    u = rng.standard_normal((B, N, 2))
    x = np.stack([gr.rollout(gr.ltv_f, rng.standard_normal(4), u[b], np.zeros(0), mtab[b] if per_traj else mtab) for b in range(B)])
    zs, Qs, seq = rng.standard_normal((1, 4)), np.eye(4)[None], np.zeros(N, dtype=np.int32)
    q = iSLS(4, 2, N, batch=B)
    q.forward_model = models.Custom(4, 2, [], tm.LTV, table=mtab)
    q.set_quadratic_cost(zs, Qs, seq, 0.1)
    q.nominal_values = x, u
    g = q.gradient(wrt=("u", "x0", "model_table"))
    check(g, gr.batch(gr.ltv_f, gr.via_cost(zs, Qs, seq, 0.1), x, u, np.zeros(0), np.zeros(0), mtab), ("cost", "costate", "u", "x0", "model_table"),
          what=f"ltv per_traj={per_traj}")
    assert (g.model_table[:, N - 1] == 0).all() and np.abs(g.model_table[:, :N - 1]).max() > 0
    with pytest.raises(capi.IslsError, match="without parameters"):
        q.gradient(wrt=("model_params",))


# al_reference's parameters with a wide obstacle and a tight speed limit: both constraints are violated along the random nominal,
# so the rounds of solve_al leave multipliers that are not zero
AL_PAR = al.PAR.copy()
AL_PAR[5], AL_PAR[6] = 2.0, 0.05


def windy_al(rng, N, B):
    x0, u, _ = quad_problem(rng, N, B)
    mtab, ctab = 0.5 * rng.standard_normal((N, 1)), 0.2 * rng.standard_normal((N, 1))
    x = np.stack([gr.rollout(gr.windy_f, x0[b], u[b], um.QUAD_PAR, mtab) for b in range(B)])
    q = iSLS(6, 2, N, batch=B)
    q.forward_model = models.Custom(6, 2, um.QUAD_PAR, WINDY, table=mtab)
    keep = costs.Custom(6, 2, AL_PAR, al.full_source(6, 2, 1, 2), table=ctab, constraints=2)
    q.cost_function = keep
    q.nominal_values = x, u
    return q, keep, mtab, ctab


def test_constraint_cost_at_nonzero_multipliers_and_solver_state():
    """W = 1 tables on both sides, K = 2 constraints: after two rounds of solve_al the multipliers are non-zero; the gradient is that
    of the PHR-augmented cost, the cost's table gradient has the user's W columns only.  Then: a gradient call between two solves
    changes nothing the second solve returns."""
    rng = np.random.default_rng(9)
    N, B = 5, 3
    q, keep, mtab, ctab = windy_al(rng, N, B)
    q.solve_al(max_outer=2, max_iter=3, tol_con=1e-9, regularization=Regularization())
    lam, mu = keep.multipliers.copy(), keep.penalty.copy()
    assert np.abs(lam).max() > 0
    x, u = q.engine.xhat.cpu().numpy(), q.engine.uhat.cpu().numpy()
    g = q.gradient(wrt=ALL)
    assert g.cost_table.shape == (B, N, 1) and g.cost_params.shape == (B, AL_PAR.size)
    rows = [gr.gradient(gr.windy_f, gr.al_cost(1, 2, lam[b], mu[b]), x[b], u[b], um.QUAD_PAR, AL_PAR, mtab, ctab) for b in range(B)]
    ref = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    check(g, ref, ("cost", "costate") + ALL, what="windy + al")
    assert np.array_equal(keep.multipliers, lam) and np.array_equal(q.engine.cost_tab.cpu().numpy()[..., 1:3], lam)

    def run(with_gradient):
        q2, keep2, _, _ = windy_al(np.random.default_rng(9), N, B)
        q2.solve(max_iter=3, regularization=Regularization())
        if with_gradient:
            q2.gradient(wrt=ALL)
        q2.solve(max_iter=3, regularization=Regularization())
        e = q2.engine
        return [t.cpu().numpy().copy() for t in (e.xhat, e.uhat, e.K, e.k, e.cost, e.status, e.reg_mu)]
    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


def test_ilqr_admm_state_untouched_and_meaning_at_convergence():
    rng = np.random.default_rng(4)
    n, m, N, B = 6, 2, 5, 3

    def run(with_gradient):
        q, *_ = lti_problem(np.random.default_rng(4), n, m, N, B)
        kw = dict(project_u=Box(-0.5, 0.5), rho_u=0.1, max_iter=3, max_admm_iter=3)
        q.ilqr_admm(**kw)
        if with_gradient:
            q.gradient()
        q.ilqr_admm(**kw)
        e = q.engine
        return [t.cpu().numpy().copy() for t in (e.xhat, e.uhat, e.K, e.k, e.cost, e.zu, e.lu)]
    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)
    # meaning: an LTI problem with the quadratic cost, solved to convergence -- max |dJ/du| falls by the factor the restatement shows
    # for the same iterates; both sides within 1e-9 of the gradient's scale before the solve (what is left after it is cancellation)
    q, A, Bm, c, x, u = lti_problem(rng, n, m, N, B)
    u[:, N - 1] = 0.0                                          # the last control is costed but never updated by the Riccati pass: start it at its optimum
    q.nominal_values = x, u
    before = q.gradient()
    q.solve(max_iter=20)
    after = q.gradient()
    x1, u1 = q.engine.xhat.cpu().numpy(), q.engine.uhat.cpu().numpy()
    r0 = gr.batch(gr.lti_f(A, Bm), c, x, u, np.zeros(0), np.zeros(0))
    r1 = gr.batch(gr.lti_f(A, Bm), c, x1, u1, np.zeros(0), np.zeros(0))
    scale = np.abs(r0["u"]).max()
    fall_dev, fall_ref = np.abs(after.u).max() / np.abs(before.u).max(), np.abs(r1["u"]).max() / scale
    print(f"max |dJ/du| before {scale:.3e}; after / before: device {fall_dev:.3e}, restatement {fall_ref:.3e}")
    assert abs(fall_dev - fall_ref) <= 1e-9 and fall_ref < 1e-6
    assert np.abs(after.u - r1["u"]).max() <= 1e-9 * scale
