"""User-written forward models (isls.models.Custom) on the device.

A model restated as a Custom source with the built-in's operation order runs the built-ins' rollout kernel template under the
built-ins' launch plan, so the line search gives the same bits.  Its Jacobians come from dual numbers and agree with the
closed forms to rounding.  A model with no built-in (a planar quadrotor) reproduces the host path of the same model given as
numpy callables, through every driver: solve, ilqr_admm, the timed outer driver with advance(), and at full batch size."""
import numpy as np
import pytest
import torch

import isls_problems as P
from test_isls_api import _check_final, _tols, make_isls, rel

import user_models as um

pytestmark = pytest.mark.gpu


def custom(name, dt):
    from isls import models
    if name == "car":
        return models.Custom(4, 2, [dt], um.CAR)
    return models.Custom(9, 3, [dt], um.ARM3R)


def builtin(name, dt):
    from isls import models
    return models.CarSimple(dt) if name == "car" else models.Planar3R(dt)


def cfg_of(name, batch):
    return P.config4(batch=batch, N=200, seed=0) if name == "car" else P.config3(batch=batch, N=100, seed=0)


def build(cfg, bsel, model, dtype=np.float64):
    import isls
    s = isls.iSLS(cfg["n"], cfg["m"], cfg["N"], batch=len(bsel), dtype=dtype)
    s.forward_model = model
    zs = cfg["zs"][bsel] if cfg["zs"].ndim == 3 else cfg["zs"]
    s.set_cost_variables(zs, cfg["Qs"], cfg["seq"], cfg["u_std"])
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in bsel])
    s.reset()
    s.nominal_values = np.stack(xs), np.stack(us)
    return s


# ---- 1. same kernel, same bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["car", "arm"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", [33, 4096])
def test_line_search_bitwise_equals_builtin(name, dtype, B):
    """The same A, B (one host get_AB for both engines), then the line search of `solve` (NaN rule, acceptance test) and one
    isls_ilqr_admm_outer iteration (box projections: the ADMM update fused into the rollout): the built-in model and its Custom
    restatement leave bit-identical x_out, u_out, cost_new, best and ADMM state.  (Compared as bit patterns: where fp32 leaves
    the arm's Quu indefinite, the NaNs must match as well.)"""
    from isls import Box
    from isls import _capi as capi
    cfg = cfg_of(name, B)
    dt = cfg["dt"]
    ref = builtin(name, dt)
    get_AB = lambda x, u: ref.get_AB(x, u)                                  # noqa: E731  (a callable: the host route)
    runs = []
    for mdl in (ref, custom(name, dt)):
        s = build(cfg, list(range(B)), mdl, dtype)
        e = s.engine
        s._linearize(get_AB)
        s._expand()
        e.gain(active=e.outer_active)
        e.feedforward(active=e.outer_active)
        e.rollout(20, flags=capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST, active=e.outer_active)
        out = [t.clone() for t in (e.xx, e.xu, e.cost_new, e.best)]
        s._setup_admm(Box(cfg["x_lo"], cfg["x_hi"]), Box(cfg["u_lo"], cfg["u_hi"]), cfg["rho_x"], cfg["rho_u"], 1.0)
        s._expand_regularised(None)
        e.build_outer(20, 4)
        e.run_outer()
        torch.cuda.synchronize()
        out += [t.clone() for t in (e.xx, e.xu, e.cost_new, e.best, e.zx, e.zu, e.lx, e.lu, e.res, e.admm_iters)]
        runs.append(out)
    bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)   # noqa: E731
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(bits(a), bits(b)), (i, (a.double() - b.double()).abs().max().item())
    assert torch.isfinite(runs[0][0]).any()


# ---- 2. Jacobians -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["car", "arm"])
def test_dual_number_jacobians(name):
    from isls import _capi as capi
    cfg = cfg_of(name, 5)
    s = build(cfg, list(range(5)), builtin(name, cfg["dt"]))
    e = s.engine
    cm = custom(name, cfg["dt"])
    capi.user_model_load(cm.model_id)
    xh, uh = e.xhat, e.uhat + 0.3 * torch.randn_like(e.uhat)               # away from zero controls
    A0, B0 = torch.zeros_like(e.A), torch.zeros_like(e.Bm)
    e.kern.linearize(builtin(name, cfg["dt"]).model_id, e.model_par, xh, uh, A0, B0)
    A1, B1 = torch.full_like(e.A, 7.0), torch.full_like(e.Bm, 7.0)
    active = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32, device=e.device)
    e.kern.linearize(cm.model_id, e.model_par, xh, uh, A1, B1, active=active)
    torch.cuda.synchronize()
    on = active.bool()
    assert rel(A1[on].cpu().numpy(), A0[on].cpu().numpy()) <= 1e-13 and rel(B1[on].cpu().numpy(), B0[on].cpu().numpy()) <= 1e-13
    assert (A1[~on] == 7.0).all() and (B1[~on] == 7.0).all()            # inactive trajectories: left untouched
    # the reference's convention on the host side: Custom.get_AB against the built-in descriptor's numpy Jacobians
    x, u = xh[0].cpu().numpy(), uh[0].cpu().numpy()
    Ah, Bh = builtin(name, cfg["dt"]).get_AB(x, u)
    Ad, Bd = cm.get_AB(x, u)
    assert rel(Ad, Ah) <= 1e-13 and rel(Bd, Bh) <= 1e-13


# ---- 3. the notebooks end to end --------------------------------------------------------------------------------------------
def test_ilqr_admm_custom_arm_and_car(golden):
    """test_isls_api.test_ilqr_admm_arm_and_car with the Custom sources in place of the built-in models."""
    from isls import Box
    for name, gname, cfg in (("arm", "g4_arm3r.npz", P.config3(batch=2, N=100, seed=0)),
                             ("car", "g5_car.npz", P.config4(batch=2, N=200, seed=0))):
        g = golden(gname)
        s = make_isls(cfg, [0, 1])
        s.forward_model = custom(name, cfg["dt"])
        L = cfg.get("max_line_search", 20)
        s.ilqr_admm(project_x=Box(cfg["x_lo"], cfg["x_hi"]), project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=3,
                    max_line_search_iter=L, max_admm_iter=cfg["max_admm_iter"], rho_x=cfg["rho_x"], rho_u=cfg["rho_u"],
                    alpha=1.0, tol=0.0)
        _check_final(s, g, "o2", [0, 1], 3, cfg["max_admm_iter"], _tols(g, "o2"))


def test_isls_admm_custom_arm(golden):
    """test_isls_admm.test_isls_admm_unconstrained_columns with the Custom arm."""
    from test_isls_admm import UNC_TOL, arm_cfg
    g = golden("g9_isls_admm.npz")
    cfg = arm_cfg()
    s = make_isls(cfg, [0, 1])
    s.forward_model = custom("arm", cfg["dt"])
    du, phi = s.isls_admm(3, None, max_line_search=10, k_max=3, max_admm_iter=1, threshold=1e-4)
    for b in range(2):
        assert rel(du[b], g["unc_du"][b]) < UNC_TOL and rel(phi[b], g["unc_phi_u"][b]) < UNC_TOL
        assert rel(np.array(s.cost_log)[:, b], g["unc_cost_log"][b]) < 1e-7


# ---- 4. a model with no built-in: the planar quadrotor ----------------------------------------------------------------------
def quad_problem(batch, N=40, seed=0):
    """Fly from near the origin to (1, 0.5) and hover there; hover thrust as the initial controls."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((batch, 6))
    x0[:, :2] = rng.uniform(-0.3, 0.3, (batch, 2))
    x0[:, 2] = rng.uniform(-0.05, 0.05, batch)
    zs = np.stack([np.zeros(6), np.array([1.0, 0.5, 0.0, 0.0, 0.0, 0.0])])
    Qs = np.stack([np.diag([0.0, 0.0, 1.0, 0.1, 0.1, 0.1]), 1e2 * np.eye(6)])
    seq = np.zeros(N, dtype=np.int32)
    seq[-1] = 1
    u0 = np.full((batch, N, 2), 0.5 * um.QUAD_PAR[1] * um.QUAD_PAR[4])
    return dict(x0=x0, zs=zs, Qs=Qs, seq=seq, u_std=1e-1, u0=u0, N=N)


def quad_isls(pb, bsel, host=False):
    import isls
    from isls import models
    f, get_AB = um.quad_numpy()
    s = isls.iSLS(6, 2, pb["N"], batch=len(bsel))
    s.forward_model = (lambda x, u: f(x, u)) if host else models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
    s.set_cost_variables(pb["zs"], pb["Qs"], pb["seq"], pb["u_std"])
    xs = []
    for b in bsel:
        x = np.zeros((pb["N"], 6))
        x[0] = pb["x0"][b]
        for t in range(pb["N"] - 1):
            x[t + 1] = f(x[t], pb["u0"][b, t])
        xs.append(x)
    s.reset()
    s.nominal_values = np.stack(xs), pb["u0"][bsel]
    return s, get_AB


def test_quadrotor_matches_the_host_path():
    from isls import Box
    pb = quad_problem(3)
    box = Box(np.array([0.0, 0.0]), np.array([8.0, 8.0]))
    d, _ = quad_isls(pb, [0, 1, 2])
    h, get_AB = quad_isls(pb, [0, 1, 2], host=True)
    d.solve(max_iter=4, max_line_search_iter=20)
    h.solve(get_AB, max_iter=4, max_line_search_iter=20)
    assert rel(d.x_nom, h.x_nom) < 1e-9 and rel(d.u_nom, h.u_nom) < 1e-9 and rel(d.cost, h.cost) < 1e-9
    d, _ = quad_isls(pb, [0, 1, 2])
    h, get_AB = quad_isls(pb, [0, 1, 2], host=True)
    d.ilqr_admm(project_u=box, max_iter=3, max_line_search_iter=20, max_admm_iter=5, rho_u=0.1, tol=0.0)
    h.ilqr_admm(get_AB, project_u=box, max_iter=3, max_line_search_iter=20, max_admm_iter=5, rho_u=0.1, tol=0.0)
    assert rel(d.x_nom, h.x_nom) < 1e-9 and rel(d.u_nom, h.u_nom) < 1e-9 and rel(d.cost, h.cost) < 1e-9
    assert (d.status == 0).all()
    # __call__ and get_AB of the descriptor against the numpy restatement
    from isls import models
    q = models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
    f, gAB = um.quad_numpy()
    x, u = d.x_nom[0], d.u_nom[0]
    assert rel(q(x, u), f(x, u)) <= 1e-13
    A, B = q.get_AB(x, u)
    An, Bn = gAB(x, u)
    assert rel(A, An) <= 1e-13 and rel(B, Bn) <= 1e-13


# ---- 5. the timed driver --------------------------------------------------------------------------------------------------
def test_quadrotor_timed_driver_with_advance():
    """build_outer(begin_done=True) / run_outer / advance() (the advance runs without the fused linearisation and launches
    the user model's own behind it) equal the launch-by-launch sequence accept_x_step, linearize, expand."""
    from isls import Box
    pb = quad_problem(6)
    box = Box(np.array([0.0, 0.0]), np.array([8.0, 8.0]))
    outs = []
    for timed in (True, False):
        s, _ = quad_isls(pb, list(range(6)))
        s._setup_admm(False, box, None, 0.1, 1.0)
        s._linearize(None)
        s._expand_regularised(None)
        e = s.engine
        if timed:
            e.begin_outer()
            e.build_outer(20, 4, begin_done=True)
            for _ in range(2):
                e.run_outer()
                e.advance()
        else:
            e.build_outer(20, 4)
            for _ in range(2):
                e.run_outer()
                e.accept_x_step()
                e.linearize()
                e.expand()
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (e.xhat, e.uhat, e.cost, e.A, e.Bm, e.c0x, e.c0u, e.K, e.k)])
    for i, (a, b) in enumerate(zip(*outs)):
        assert rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-12, i


# ---- 6. batch independence at full size -----------------------------------------------------------------------------------
def test_quadrotor_full_batch(monkeypatch):
    """Two outer iterations at B = 4096; eight of the trajectories against a batch-8 run of the same problems.  The engine picks
    the time-parallel feed-forward pass below 2048 trajectories (equal up to rounding); the batch-8 run is held to the
    sequential pass that B = 4096 runs, so that the comparison is about the user model's kernels."""
    from isls import Box
    B = 4096
    pb = quad_problem(B, seed=1)
    box = Box(np.array([0.0, 0.0]), np.array([8.0, 8.0]))
    kw = dict(project_u=box, max_iter=2, max_line_search_iter=20, max_admm_iter=5, rho_u=0.1, tol=0.0)
    s, _ = quad_isls(pb, list(range(B)))
    s.ilqr_admm(**kw)
    assert np.isfinite(s.x_nom).all() and np.isfinite(s.u_nom).all() and np.isfinite(s.cost).all()
    assert (s.status == 0).all()
    pick = [0, 1, 63, 64, 1000, 2047, 4000, 4095]
    monkeypatch.setenv("ISLS_FF_NSEG", "1")
    t, _ = quad_isls(pb, pick)
    t.ilqr_admm(**kw)
    assert rel(s.x_nom[pick], t.x_nom) < 1e-12 and rel(s.u_nom[pick], t.u_nom) < 1e-12 and rel(s.cost[pick], t.cost) < 1e-12


# ---- 7. closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_custom_car_equals_builtin():
    cfg = P.config4(batch=2, N=200, seed=0)
    rng = np.random.default_rng(3)
    N, n, m = 200, 4, 2
    K = 1e-3 * np.tril(rng.standard_normal((N * m, N * n)))
    k = 1e-2 * rng.standard_normal(N * m)
    dx0 = 0.05 * rng.standard_normal((8, n))
    res = []
    for mdl in (builtin("car", cfg["dt"]), custom("car", cfg["dt"])):
        s = build(cfg, [0, 1], mdl)
        res.append(s.get_trajectory_sls(s.x_nom[1][0] + dx0, K, k, problem=1))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.isfinite(res[0][0]).all()
