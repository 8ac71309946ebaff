"""GPU tests of the receding-horizon loop iSLS.mpc (isls/isls.py): its orchestration against a host-driven loop of the same
kernels (ilqr_admm, Kernels.mpc_step -- proved against numpy in tests/test_mpc_step_gpu.py --, Engine.nominal_rewritten), the
logged states against the numpy models, the tracking window, a plant that is not the model, seeds, the state it leaves, refusals.
B = 5, N = 20, T = 4, iters = 2, J = 3; fp64.  rel = max-abs error over max(1, |ref|_max), bound 1e-10 as in
tests/test_monte_carlo_gpu.py."""
import numpy as np
import pytest
import torch

import isls_problems as P
import table_costs as tc
import user_models as um
from isls import _capi as capi

pytestmark = pytest.mark.gpu
B, N, T, ITERS, J, L = 5, 20, 4, 2, 3, 20
U_STD = 1e-2


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


def di_solver():
    import isls
    from isls import models
    cfg = P.config2(batch=B, N=N, seed=0)
    s = isls.iSLS(6, 3, N, batch=B)
    s.forward_model = models.LTI(cfg["A"], cfg["B"])
    s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in range(B)])
    s.reset()
    s.nominal_values = np.stack(xs), np.stack(us)
    return s, cfg, models.LTI(cfg["A"], cfg["B"])


def car_solver(dt=0.1, table=None, seed=4):
    import isls
    from isls import costs, models
    rng = np.random.default_rng(seed)
    mdl = models.CarSimple(dt)
    tab = tc.make_table(rng, N, 4, B, terminal=5.0) if table is None else table
    us = 0.3 * rng.normal(size=(B, N, 2))
    xs = np.zeros((B, N, 4))
    xs[:, 0] = [0.0, 0.0, 0.3, 1.0]
    for t in range(N - 1):
        xs[:, t + 1] = mdl(xs[:, t], us[:, t])
    s = isls.iSLS(4, 2, N, batch=B)
    s.forward_model = mdl
    s.cost_function = costs.Custom(4, 2, [U_STD], tc.tracking_source(4, 2), table=tab)
    s.reset()
    s.nominal_values = xs, us
    return s, mdl, tab


def box_u(lim):
    from isls import Box
    return Box(-lim, lim)


def host_loop(q, steps, iters, w=None, warm_start_z=False, **admm):
    """the loop the parent code allows, on the same kernels in the same order: ilqr_admm(max_iter=iters), the control step on the
    engine's buffers, the nominal-rewritten method; with warm_start_z the moved z survives the next call's set-up"""
    e = q.engine
    xl, ul = np.zeros((B, steps + 1, e.n)), np.zeros((B, steps, e.m))
    cl, il = np.zeros((B, steps)), np.zeros((B, steps), dtype=np.int32)
    keep = {}
    plain_set_admm = e.set_admm

    def set_admm(*a, **k):
        plain_set_admm(*a, **k)
        for name, zz in keep.items():
            getattr(e, name).copy_(zz)
    e.set_admm = set_admm
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=e.dtype, device=e.device)   # noqa: E731
    for s in range(steps):
        q.ilqr_admm(max_iter=iters, max_admm_iter=J, max_line_search_iter=L, tol=1e-3, **admm)
        cl[:, s], il[:, s] = e.cost.cpu().numpy(), e.admm_iters.cpu().numpy()
        xm, ua, xn = (torch.zeros(B, d, dtype=e.dtype, device=e.device) for d in (e.n, e.m, e.n))
        e.kern.mpc_step(e.model, e.model_par, e.xhat, e.uhat, K=e.K, zx=e.zx if warm_start_z else None,
                        zu=e.zu if warm_start_z else None, tab=e.cost_tab, w=None if w is None else dev(w[:, s]), step=s,
                        x_meas_out=xm, u_out=ua, x_next_out=xn, stream=torch.cuda.current_stream().cuda_stream)
        e.nominal_rewritten()
        if warm_start_z:
            keep = {name: getattr(e, name).clone() for name in ("zx", "zu") if getattr(e, name) is not None}
        xl[:, s], ul[:, s], xl[:, s + 1] = xm.cpu().numpy(), ua.cpu().numpy(), xn.cpu().numpy()
    return xl, ul, cl, il


# ---- orchestration -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True], ids=["fresh_z", "warm_z"])
@pytest.mark.parametrize("problem", ["di", "car"])
def test_loop_equals_host_driven_loop(problem, warm):
    rng = np.random.default_rng(1)
    make = (lambda: di_solver()[0]) if problem == "di" else (lambda: car_solver()[0])
    admm = dict(project_u=box_u(2.0 if problem == "di" else 0.4), rho_u=1e-2 if problem == "di" else 1e-1)
    n = 6 if problem == "di" else 4
    w = 0.01 * rng.standard_normal((B, T, n))
    q1, q2 = make(), make()
    r = q1.mpc(steps=T, iters=ITERS, max_admm_iter=J, max_line_search_iter=L, tol=1e-3, w=w, warm_start_z=warm, **admm)
    xl, ul, cl, il = host_loop(q2, T, ITERS, w=w, warm_start_z=warm, **admm)
    print(f"{problem} warm={warm}: max |dx| {np.max(np.abs(r.x - xl)):.2e} |du| {np.max(np.abs(r.u - ul)):.2e} "
          f"|dcost| {np.max(np.abs(r.cost - cl)):.2e} admm iters {r.admm_iters.tolist()} / {il.tolist()}")
    assert np.array_equal(r.admm_iters, il)
    assert np.array_equal(r.x, xl) and np.array_equal(r.u, ul) and np.array_equal(r.cost, cl)
    assert r.x.shape == (B, T + 1, n) and r.status.shape == (B, T) and not r.status.any()
    assert np.array_equal(q1.x_nom, q2.x_nom) and np.array_equal(q1.K, q2.K)


# ---- end to end against numpy ------------------------------------------------------------------------------------------------
def test_di_logged_states_follow_the_model_and_approach_the_target():
    q, cfg, mdl = di_solver()
    lo, hi = -1.5, 1.5
    r = q.mpc(steps=T, iters=ITERS, max_admm_iter=J, project_u=box_u(2.0), rho_u=1e-2, clip_u=(lo, hi))
    assert np.all(r.u >= lo) and np.all(r.u <= hi)
    for s in range(T):
        assert rel(r.x[:, s + 1], mdl(r.x[:, s], r.u[:, s])) < 1e-10
    target = cfg["zs"][:, 1, :3]
    d0, dT = np.linalg.norm(r.x[:, 0, :3] - target, axis=1), np.linalg.norm(r.x[:, T, :3] - target, axis=1)
    print("distance to the target at s = 0 / T:", d0, dT)
    assert np.all(dT < d0)
    # the state the call leaves: the last plan starts at the last measurement, and the validation tools run on it
    assert np.array_equal(q.x_nom[:, 0], r.x[:, T])
    cov = q.covariance(x0_std=0.01, noise_scale=0.01)
    assert cov.x_var.shape == (B, N, 6) and np.isfinite(cov.x_var).all()
    mc = q.monte_carlo(q.K, q.k, samples=8, x0_std=0.01)
    assert mc.samples == 8


def test_car_logged_states_follow_the_model():
    q, mdl, _ = car_solver()
    r = q.mpc(steps=T, iters=ITERS, max_admm_iter=J, project_u=box_u(0.4), rho_u=1e-1)
    for s in range(T):
        assert rel(r.x[:, s + 1], mdl(r.x[:, s], r.u[:, s])) < 1e-10
    assert np.isfinite(r.cost).all()


# ---- the tracking window -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["per_trajectory", "shared"])
@pytest.mark.parametrize("future", [True, False], ids=["future", "held"])
def test_tracking_window(shared, future):
    rng = np.random.default_rng(6)
    tab = tc.make_table(rng, N, 4, None if shared else B, terminal=5.0)
    fut = tc.make_table(rng, T, 4, None if shared else B, terminal=1.0)
    q, _, _ = car_solver(table=tab)
    q.mpc(steps=T, iters=1, max_admm_iter=J, table_future=fut if future else None)
    got = q.engine.cost_tab.cpu().numpy()
    if future:
        want = np.concatenate([tab, fut], axis=-2)[..., T:T + N, :]
    else:
        want = np.concatenate([tab] + [tab[..., -1:, :]] * T, axis=-2)[..., T:T + N, :]
    assert np.array_equal(got, want)
    assert np.array_equal(q.cost_function.table, want)          # the cost object follows the window


# ---- a plant that is not the model -------------------------------------------------------------------------------------------
def test_plant_mismatch_follows_the_plants_parameters():
    from isls import models
    q, mdl, _ = car_solver()
    dts = 0.1 * (1 + 0.3 * np.linspace(-1, 1, B))
    r = q.mpc(steps=T, iters=1, max_admm_iter=J, plant_params=dts[:, None])
    for s in range(T):
        plant = np.stack([models.CarSimple(dts[b])(r.x[b, s], r.u[b, s]) for b in range(B)])
        assert rel(r.x[:, s + 1], plant) < 1e-10
        assert rel(r.x[:, s + 1], mdl(r.x[:, s], r.u[:, s])) > 1e-4      # not the model's


def test_custom_model_loop():
    import isls
    from isls import models
    quad = models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
    f = um.quad_numpy()[0]
    q = isls.iSLS(6, 2, N, batch=B)
    q.forward_model = quad
    zs, Qs, seq = P.via_point_cost(6, N, [0.5, 0.5, 0, 0, 0, 0], 10.0 * np.eye(6))
    q.set_cost_variables(zs, Qs, seq, 1e-2)
    us = np.full((B, N, 2), 4.905) + 0.01 * np.random.default_rng(0).standard_normal((B, N, 2))
    xs = np.zeros((B, N, 6))
    for t in range(N - 1):
        xs[:, t + 1] = f(xs[:, t], us[:, t])
    q.reset()
    q.nominal_values = xs, us
    r = q.mpc(steps=T, iters=1, max_admm_iter=J)
    for s in range(T):
        assert rel(r.x[:, s + 1], f(r.x[:, s], r.u[:, s])) < 1e-10


# ---- seeds -------------------------------------------------------------------------------------------------------------------
def test_seeds():
    runs = [di_solver()[0].mpc(steps=T, iters=1, max_admm_iter=J, noise_scale=0.02, seed=sd).x for sd in (3, 3, 4)]
    assert np.array_equal(runs[0], runs[1])
    assert not np.array_equal(runs[0][:, 1:], runs[2][:, 1:])
    assert np.array_equal(runs[0][:, 0], runs[2][:, 0])         # the first measurement is the given initial state


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from isls import Regularization
    q, _, mdl = di_solver()
    with pytest.raises(capi.IslsError, match="regularization"):
        q.mpc(steps=1, regularization=Regularization())
    with pytest.raises(capi.IslsError, match="plant_params"):
        q.mpc(steps=1, plant_params=np.zeros((B + 1, 3)))
    with pytest.raises(capi.IslsError, match="table_future"):
        q.mpc(steps=1, table_future=np.zeros((1, 8)))
    with pytest.raises(capi.IslsError, match="Box or ConvexSets"):
        q.mpc(steps=1, project_u=lambda v: v / max(1.0, float(np.linalg.norm(v))), rho_u=1e-2)   # no box: a host projection
    q.cost_function = lambda x, u: np.zeros(x.shape[0])
    with pytest.raises(capi.IslsError, match="costs.Custom"):
        q.mpc(steps=1)
    q2, _, _ = di_solver()
    q2.forward_model = lambda x, u: mdl(x, u)
    with pytest.raises(capi.IslsError, match="models.Custom"):
        q2.mpc(steps=1)
