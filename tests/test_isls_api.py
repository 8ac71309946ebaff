"""GPU parity of the host-side mirror of the reference class surface (`isls.iSLS`, `isls.SLS`) against golden
vectors produced by the reference itself (tests/golden/*.npz), plus batch invariance.  fp64 tolerance 1e-10
(relative to max(1,|ref|)); the arm problem uses the conditioning-aware bound stored with its golden trace."""
import numpy as np
import pytest

import isls_problems as P

pytestmark = pytest.mark.gpu
TOL = 1e-10


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def make_isls(cfg, bsel):
    import isls
    from isls import models
    bsel = list(bsel)
    n, m, N = cfg["n"], cfg["m"], cfg["N"]
    s = isls.iSLS(n, m, N, batch=len(bsel))
    if cfg["model"] == P.MODEL_LTI:
        s.forward_model = models.LTI(cfg["A"], cfg["B"])
    elif cfg["model"] == P.MODEL_ARM3R:
        s.forward_model = models.Planar3R(cfg["dt"])
    else:
        s.forward_model = models.CarSimple(cfg["dt"])
    zs = cfg["zs"][bsel] if cfg["zs"].ndim == 3 else cfg["zs"]
    s.set_cost_variables(zs[0] if len(bsel) == 1 and zs.ndim == 3 else zs, cfg["Qs"], cfg["seq"], cfg["u_std"])
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in bsel])
    s.reset()
    s.nominal_values = (xs[0], us[0]) if len(bsel) == 1 else (np.stack(xs), np.stack(us))
    return s


# ---------------------------------------------------------------------------------------------------------
# SLS (config 1 of BASELINE.json and the notebook problem)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,N", [("n50", 50), ("n100", 100)])
def test_sls_dp_and_admm_lqt_dp(golden, tag, N):
    import isls
    g = golden("g1_di1d_lqt.npz")
    c = P.config1(N)
    sls = isls.SLS(2, 1, N)
    sls.AB = [c["A"], c["B"]]
    sls.set_quadratic_cost(c["zs"], c["Qs"], c["seq"], c["u_std"])
    K, k = sls.solve(method="dp")
    assert rel(K, g[f"{tag}_dp_K"]) < TOL and rel(k, g[f"{tag}_dp_k"]) < TOL
    Qr, Rr = sls.compute_Rr_Qr(rho_x=None, rho_u=c["rho_u"], dp=True)
    K2, k2, Quu, Quu_inv, Qux = sls.solve_dp(Rr=Rr, Qr=Qr, xr=np.zeros(2 * N), ur=g[f"{tag}_reg_ur"], return_Qs=True)
    for mine, key in ((K2, "reg_K"), (k2, "reg_k"), (Quu, "reg_Quu"), (Quu_inv, "reg_Quu_inv"), (Qux, "reg_Qux")):
        assert rel(mine, g[f"{tag}_{key}"]) < TOL, key
    kff = sls.solve_dp_ff(K2, Quu, Qux, Quu_inv, Qr=Qr, Rr=Rr, ur=g[f"{tag}_ff_ur"], xr=np.zeros(2 * N))
    assert rel(kff, g[f"{tag}_ff_k"]) < TOL
    # the notebook call, lambda and all (control bounds.ipynb cell 13)
    x, u, Ka, ka, logs = sls.ADMM_LQT_DP(c["x0"], project_u=lambda v: isls.project_bound(v, c["u_lo"], c["u_hi"]),
                                         max_iter=500, rho_u=c["rho_u"], tol=c["tol"], verbose=False, log=True)
    gl = g[f"{tag}_admm_dp_logs"]
    assert len(logs) == len(gl)
    assert rel(np.stack(logs), gl) < TOL
    assert rel(x, g[f"{tag}_admm_dp_x"]) < TOL and rel(u, g[f"{tag}_admm_dp_u"]) < TOL
    assert rel(Ka, g[f"{tag}_admm_dp_K"]) < TOL and rel(ka, g[f"{tag}_admm_dp_k"]) < TOL
    assert abs(sls.compute_cost(x, u) - float(g[f"{tag}_admm_dp_cost"])) < 1e-9
    # Monte-Carlo closed-loop evaluation (sls_base.py:76-89) is batch-invariant
    x0s = np.random.default_rng(0).normal(scale=0.1, size=(33, 2))
    xs, us = sls.get_trajectory_dp(x0s, Ka, ka)
    x1, u1 = sls.get_trajectory_dp(x0s[7], Ka, ka)
    assert np.array_equal(xs[7], x1) and np.array_equal(us[7], u1)


@pytest.mark.parametrize("tag,N", [("n50", 50), ("n100", 100)])
def test_sls_batch_form_through_the_riccati_pass(golden, tag, N):
    """solve_batch / ADMM_LQT_Batch (config 1's second oracle, isls/sls.py:60-82,252-293) against the unmodified reference.
    The reference solves dense normal equations (Su'Q Su + R, Q = 1e6, R = 1e-2: condition number ~1e9), ours is the
    Riccati pass + the dense form's last control; the two agree to the accuracy of the reference's own dense solve."""
    import isls
    g = golden("g1_di1d_lqt.npz")
    c = P.config1(N)
    sls = isls.SLS(2, 1, N)
    sls.AB = [c["A"], c["B"]]
    sls.set_quadratic_cost(c["zs"], c["Qs"], c["seq"], c["u_std"])
    x, u = sls.solve(c["x0"], method="batch")
    assert x.shape == (N, 2) and u.shape == (N, 1)
    assert rel(x, g[f"{tag}_batch_x"]) < 1e-7 and rel(u, g[f"{tag}_batch_u"]) < 1e-7
    xb, ub, logs = sls.ADMM_LQT_Batch(x0=c["x0"], project_u=lambda v: isls.project_bound(v, c["u_lo"], c["u_hi"]), max_iter=100,
                                      rho_u=1e-2, tol=1e-4, verbose=False, log=True)
    gl = g[f"{tag}_admm_batch_logs"]
    assert len(logs) == len(gl)                                    # n100: 20 iterations, the notebook's count
    assert rel(np.stack(logs), gl) < 1e-6
    assert rel(ub, g[f"{tag}_admm_batch_u"]) < 1e-7
    if N == 100:
        assert abs(np.max(ub) - 5.000018035934772) < 1e-7          # control bounds.ipynb:204-207


def test_sls_admm_with_state_constraints(golden):
    """SLS.ADMM_SLS(project_x=..., project_u=...) as the state-bounds notebook calls it (cells 12-17: the callables are
    closures over project_set_convex acting on single rows of the (N n) x 2 state variable) against the unmodified
    reference (G11).  Ours iterates over the feedback columns with the Riccati kernels; the reference inverts the dense
    (N m)^2 normal equations."""
    import isls
    from isls.projections import project_set_convex, project_soc_unit
    from scipy.stats import norm
    g = golden("g11_sls_state.npz")
    N, n = 40, 2
    for b in range(2):
        target, upper_u, var_x0, conf = (float(g[k][b]) for k in ("targets", "upper_u", "var_x0", "conf"))
        sls = isls.SLS(2, 1, N)
        sls.AB = [g["A"], g["B"]]
        seq = np.zeros(N, dtype=np.int32)
        seq[N - 1] = 1
        sls.set_quadratic_cost(np.stack([np.zeros(n), [target, 0.0]]), np.stack([np.zeros((n, n)), 1e6 * np.eye(n)]), seq, 1e-2)
        psi_inv = norm.ppf(conf)
        mu, sigma = np.array([1.0, 0.0]), np.array([0.0, var_x0])
        Au = np.diag(np.sqrt(sigma))
        A_ = [np.concatenate([Au, (-mu / psi_inv)[None]], 0), np.concatenate([Au, (mu / psi_inv)[None]], 0)]
        b_u = [np.append(np.zeros(2), upper_u / psi_inv), np.append(np.zeros(2), upper_u / psi_inv)]
        b_pos = [np.append(np.zeros(2), (target + 0.05) / psi_inv), np.append(np.zeros(2), -(target - 0.05) / psi_inv)]
        b_vel = [np.append(np.zeros(2), 0.0), np.append(np.zeros(2), 0.0)]
        kw = dict(projections=[project_soc_unit] * 2, rho=1e1, max_iter=20, threshold=1e-2)
        project_u = lambda y: project_set_convex(y, A_, b_u, **kw)             # noqa: E731

        def project_x(x):
            x_ = x.copy()
            x_[-2:-1] = project_set_convex(x_[-2:-1], A_, b_pos, **kw)
            x_[-1:] = project_set_convex(x_[-1:], A_, b_vel, **kw)
            return x_
        du, phi_u, logs = sls.ADMM_SLS(project_u=project_u, project_x=project_x, max_iter=30, rho_x=g["rho_x"][b], rho_u=1e-3,
                                       alpha=1.0, tol=1e-5, verbose=0, log=True)
        n_it = int(g["n_it"][b])
        assert len(logs) == n_it
        assert rel(np.stack(logs), g["logs"][b][:n_it]) < 1e-6
        assert rel(du, g["du"][b]) < 1e-7 and rel(phi_u[:, :1], g["phi_u"][b][:, :1]) < 1e-7
        assert phi_u.shape == g["phi_u"][b].shape and rel(phi_u, g["phi_u"][b]) < 1e-3   # tail columns: solve_sls' Woodbury chain (see G7)
        # the same call with the constraints as device descriptors: the state projection touches two rows, each with its
        # own set -- one stage per row (row masks + `then` chain, ISLS_PROJ_SETS): nothing leaves the GPU
        from isls.projections import chance_constraint_rows
        ckw = dict(rho=1e1, max_iter=20, threshold=1e-2)
        pos = chance_constraint_rows(1, target + 0.05, target - 0.05, var_x0, psi_inv, **ckw)
        vel = chance_constraint_rows(1, 0.0, 0.0, var_x0, psi_inv, **ckw)
        pos.rows, vel.rows, pos.then = [N * n - 2], [N * n - 1], vel
        dev_u = chance_constraint_rows(1, upper_u, -upper_u, var_x0, psi_inv, **ckw)
        sl2 = isls.SLS(2, 1, N)
        sl2.AB = [g["A"], g["B"]]
        sl2.set_quadratic_cost(np.stack([np.zeros(n), [target, 0.0]]), np.stack([np.zeros((n, n)), 1e6 * np.eye(n)]), seq, 1e-2)
        du2, phi2, logs2 = sl2.ADMM_SLS(project_u=dev_u, project_x=pos, max_iter=30, rho_x=g["rho_x"][b], rho_u=1e-3, alpha=1.0,
                                        tol=1e-5, verbose=0, log=True)
        assert len(logs2) == n_it and rel(np.stack(logs2), g["logs"][b][:n_it]) < 1e-6
        assert rel(du2, g["du"][b]) < 1e-7 and rel(phi2[:, :1], g["phi_u"][b][:, :1]) < 1e-7


def test_sls_lqt_admm_with_numpy_callables(golden):
    """ADMM_LQT_DP / ADMM_LQT_Batch with an arbitrary numpy state projection -- the spherical-obstacle notebook's
    project_state (project_set_convex + Dykstra over quadratic shells, cells 12-14) -- against the unmodified reference
    (G12): x-step on the device, z-step through the caller's function (host mirror of the reference's ADMM())."""
    import importlib
    import isls
    projmod = importlib.import_module("isls.projections")       # (`isls.projections` the attribute is a dict, as in the reference)
    g = golden("g12_obstacles.npz")
    N, x_dim, d = 60, 2, 4
    sls = isls.SLS(d, x_dim, N)
    sls.AB = [g["A"], g["B"]]
    seq = np.zeros(N, dtype=np.int32)
    seq[N - 1] = 1
    sls.set_quadratic_cost(np.stack([np.zeros(d), [1.0, 1.0, 0.0, 0.0]]), np.stack([np.zeros((d, d)), 1e3 * np.eye(d)]), seq, 1e-4)
    lowers = [0.5 * (1.1 * r) ** 2 for r in g["radii"]]
    shells = [lambda x, lo=lo, c=c: projmod.project_quadratic(x - c, lo, 1e2) + c for lo, c in zip(lowers, g["centres"])]

    def project_state(x):
        x_ = x.reshape(-1, d).copy()
        x_[:, :x_dim] = projmod.project_set_convex(x_[:, :x_dim], [np.eye(x_dim)] * 2, [np.zeros(x_dim)] * 2, shells, max_iter=5,
                                                   verbose=0, threshold=1e-2)
        x_[:, :x_dim] = projmod.project_set_convex_dykstra(x_[:, :x_dim], shells, max_iter=50, verbose=0, tol=1e-5)
        return x_.flatten()
    rho_x = np.zeros((N, d, d))
    rho_x[:, :x_dim, :x_dim] = np.eye(x_dim)
    # Keeping points out of a ball is a non-convex projection and the iteration is chaotic: from iteration ~25 on it amplifies
    # rounding differences ~10x per iteration (measured: ours vs the reference 1e-12 for 25 iterations, 1e-1 after 45), so
    # the golden vectors stop at 20 / 25 iterations, where the reference's own trace is still reproducible.
    xb, ub, logb = sls.ADMM_LQT_Batch(np.zeros(d), project_x=project_state, max_iter=20, rho_x=rho_x, alpha=1.0, tol=1e-3, log=True)
    assert len(logb) == len(g["batch_logs"]) and rel(np.stack(logb), g["batch_logs"]) < 1e-8
    assert rel(xb, g["batch_x"]) < 1e-8 and rel(ub, g["batch_u"]) < 1e-7
    xd, ud, Kd, kd, logd = sls.ADMM_LQT_DP(np.zeros(d), project_x=project_state, max_iter=25, rho_x=rho_x, tol=1e-4, log=True)
    assert len(logd) == len(g["dp_logs"]) and rel(np.stack(logd), g["dp_logs"]) < 1e-9
    assert rel(xd, g["dp_x"]) < 1e-9 and rel(ud, g["dp_u"]) < 1e-8 and rel(kd, g["dp_k"]) < 1e-8
    sl2 = isls.SLS(d, x_dim, N, batch=2)
    sl2.AB = [g["A"], g["B"]]
    sl2.set_quadratic_cost(np.stack([np.zeros(d), [1.0, 1.0, 0.0, 0.0]]), np.stack([np.zeros((d, d)), 1e3 * np.eye(d)]), seq, 1e-4)
    with pytest.raises(NotImplementedError):
        sl2.ADMM_LQT_DP(np.zeros(d), project_x=project_state, rho_x=rho_x)
    # the same state constraint as a device descriptor (ISLS_SET_SHELL: project_set_convex, then Dykstra): the
    # whole ADMM iteration stays on the GPU -- batched -- and reproduces the reference's trace in its reproducible window
    cs = projmod.spherical_keepout(d, g["centres"], g["radii"], q=x_dim)
    xd2, ud2, Kd2, kd2, logd2 = sl2.ADMM_LQT_DP(np.zeros(d), project_x=cs, max_iter=25, rho_x=rho_x, tol=1e-4, log=True)
    assert rel(np.stack(logd2)[:, 0], g["dp_logs"]) < 1e-8 and rel(np.stack(logd2)[:, 1], g["dp_logs"]) < 1e-8
    assert rel(xd2[0], g["dp_x"]) < 1e-8 and rel(ud2[1], g["dp_u"]) < 1e-7


def test_sls_replanning_and_open_loop_helpers():
    """initialize_replanning_procedure / replan_feedforward (isls/sls.py:244-248), u_optimal / x_optimal and
    get_trajectory_batch (isls/sls_base.py:55-74): replanning the feed-forward term for moved targets equals the
    controller computed from scratch for them."""
    import isls
    N = 20
    c = P.config1(N)
    sls = isls.SLS(2, 1, N)
    sls.AB = [c["A"], c["B"]]
    sls.set_quadratic_cost(c["zs"], c["Qs"], c["seq"], c["u_std"])
    PHI_U, du = sls.solve_sls()
    K, k = sls.controller(PHI_U, du)
    sls.initialize_replanning_procedure(K)
    Su, (Q, R, xd) = sls.Su, sls._dense_cost()
    xd2 = xd + np.random.default_rng(3).normal(scale=0.1, size=xd.shape)
    du2 = np.linalg.solve(Su.T @ Q @ Su + R, Su.T @ Q @ xd2)
    assert rel(sls.replan_feedforward(k, xd2), (np.eye(N) - K @ Su) @ du2) < 1e-8
    x0 = np.array([0.3, -0.1])
    u_opt = sls.u_optimal(x0, PHI_U, du)
    assert u_opt.shape == (N - 1, 1)
    xs, us = sls.get_trajectory_batch(x0[None].repeat(3, 0), np.pad(u_opt, ((0, 1), (0, 0))))
    x = x0.copy()
    for t in range(N - 1):                                          # the open-loop sequence reproduces x = Sx x0 + Su u
        assert rel(xs[1, t], x) < 1e-12
        x = c["A"] @ x + c["B"] @ u_opt[t]
    assert rel(sls.x_optimal(x0, sls.Sw + Su @ PHI_U, Su @ du)[:N - 1], xs[0, :N - 1]) < 1e-9


# ---------------------------------------------------------------------------------------------------------
# iSLS: kernels through the class surface
# ---------------------------------------------------------------------------------------------------------
def test_isls_backward_rollout_iterate(golden):
    g = golden("g3_di3d.npz")
    cfg = P.config2(batch=int(g["cfg_batch"]), N=100, seed=int(g["cfg_seed"]))
    for b in range(2):
        s = make_isls(cfg, [b])
        K, k = s.backward_pass_DP()
        assert rel(K, g["bp_quad_K"][b]) < TOL and rel(k, g["bp_quad_k"][b]) < TOL
        k_new = k[None] * s.alphas[[0, 7, 19], None, None]
        x_noms, u_noms = s.rollout_DP(K, k_new)
        assert rel(x_noms, g["ro_x_sel"][b]) < TOL and rel(u_noms, g["ro_u_sel"][b]) < TOL
        ok, _, _ = s.iterate_once_dp(max_line_search=20)
        io = g["iter_once"][b]
        assert ok and abs(s.cost - io[1]) < 1e-9 * max(1, abs(io[1]))
        assert rel(s.x_nom.ravel(), io[2:2 + 600]) < TOL and rel(s.u_nom.ravel(), io[2 + 600:]) < TOL


@pytest.mark.parametrize("which", ["di3d", "arm", "arm_task2"])
def test_isls_solve_cost_logs(golden, which):
    if which == "di3d":
        g = golden("g3_di3d.npz")
        cfg = P.config2(batch=int(g["cfg_batch"]), N=100, seed=int(g["cfg_seed"]))
        refs, kw = g["ilqr_cost_log"], dict(max_iter=10, max_line_search_iter=20)
    elif which == "arm":
        g = golden("g4_arm3r.npz")
        cfg = P.config3(batch=2, N=100, seed=0)
        refs, kw = g["ilqr_cost_log"], dict(max_iter=30, max_line_search_iter=20)
    else:
        g = golden("g4_arm3r.npz")
        cfg = P.config3(batch=1, N=100, seed=0)
        cfg["zs"], cfg["Qs"], cfg["seq"] = P.via_point_cost(9, 100, [0, 0, 0, 0, 0, 0, 1.5, 2.0, 0.0],
                                                             np.diag([0, 0, 0, 1e3, 1e3, 1e3, 1e3, 1e3, 0.0]))
        cfg["u0"] = np.zeros_like(cfg["u0"])
        refs, kw = g["task2_cost_log"][None], dict(max_iter=30, max_line_search_iter=20)
    for b in range(len(refs)):
        ref = refs[b][~np.isnan(refs[b])]
        s = make_isls(cfg, [b])
        s.solve(**kw)
        # at the optimum the acceptance test `cost_new - cost < 0` (isls.py:365-367) is decided by the last bits
        # (the reference rejects a step that changes the cost by 2 ulp, an FMA-contracted build may accept it):
        # the log must reproduce the reference's entries; extra entries may only repeat the converged cost
        mine = np.array(s.cost_log)
        assert len(mine) >= len(ref), (s.cost_log, ref)
        tol = TOL if which == "di3d" else max(TOL, 10 * float(np.max(g["o2_sens"])))     # arm: conditioning-aware
        assert rel(mine[:len(ref)], ref) < tol, (mine, ref)
        assert np.allclose(mine[len(ref):], ref[-1], rtol=1e-6, atol=0)
    if which == "arm_task2":       # numbers recorded in the reference's notebook
        assert abs(s.cost_log[0] - 6775.068343357641) < 1e-9 and abs(s.cost_log[-1] - 0.1180803005667605) < 1e-9


# ---------------------------------------------------------------------------------------------------------
# iSLS.ilqr_admm (DP form) against the reference-composed O2 traces
# ---------------------------------------------------------------------------------------------------------
def test_isls_open_loop_and_monte_carlo_helpers():
    """get_trajectory_batch (isls/isls_base.py:44-57) before any cost is set, Monte-Carlo get_trajectory_dp over M initial
    states with batch == 1, and the dense Sw / Su (C / D) of the last linearisation (isls/base.py:98-119)."""
    import isls
    from isls import models
    cfg = P.config4(batch=1, N=30, seed=1)
    s = isls.iSLS(4, 2, 30)
    s.forward_model = models.CarSimple(cfg["dt"])
    f = P.car_f(cfg["dt"])
    u = 0.1 * np.random.default_rng(0).standard_normal((30, 2))
    x_ol, u_ol = s.get_trajectory_batch(cfg["x0"][0], u)
    assert rel(x_ol, P.rollout_open_loop(f, cfg["x0"][0], u)) < 1e-12 and np.array_equal(u_ol, u)
    x0s = cfg["x0"][0] + 0.05 * np.random.default_rng(1).standard_normal((7, 4))
    K, k = 0.1 * np.random.default_rng(2).standard_normal((30, 2, 4)), u
    xs, us = s.get_trajectory_dp(x0s, K, k)
    assert xs.shape == (7, 30, 4)
    x1, u1 = s.get_trajectory_dp(x0s[3], K, k)
    assert np.array_equal(xs[3], x1) and np.array_equal(us[3], u1)
    s.set_cost_variables(cfg["zs"][0] if cfg["zs"].ndim == 3 else cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    s.nominal_values = x_ol, u_ol
    s.backward_pass_DP()                                          # linearises about the nominal
    Sw, Su = s.Sw, s.Su
    assert s.C is not None and Sw.shape == (120, 120) and Su.shape == (120, 60) and not Su[:, -2:].any()
    A = s.engine.A.cpu().numpy()[0]
    assert rel(Sw[4:8, :4], A[0]) < 1e-14 and rel(Sw[8:12, :4], A[1] @ A[0]) < 1e-13


@pytest.mark.parametrize("name", ["arm", "car"])
def test_isls_batch_form_ilqr(golden, name):
    """backward_pass_batch / iterate_once_batch / solve(method='batch') (isls/isls.py:156-228) against the reference's dense
    least squares (G10).  The reference solves normal equations with condition number ~1e10 (arm: Q = 1e6, R = 1e-4), so its
    own delta_u carries ~1e-6 relative error; the cost logs agree much better because the minimiser is flat there."""
    g = golden("g10_batch_ilqr.npz")
    cfg = P.config3(batch=2, N=40, seed=3) if name == "arm" else P.config4(batch=2, N=60, seed=2)
    s = make_isls(cfg, [0, 1])
    du0 = s.backward_pass_batch()
    assert rel(du0, g[f"{name}_du0"]) < 2e-5
    x_ol, _ = s.rollout_batch(s.x_nom[0], (s.u_nom[0] + du0[0])[None])            # open-loop rollout of one candidate
    assert x_ol.shape == (2, 1, cfg["N"], cfg["n"]) and np.array_equal(x_ol[0, 0, 0], s.x_nom[0, 0])
    s.solve(method='batch', max_iter=6, max_line_search_iter=20)
    logs = np.array(s.cost_log)
    for b in range(2):
        n_it = int(g[f"{name}_n_it"][b])
        mine = logs[:n_it, b]
        assert rel(mine, g[f"{name}_cost_log"][b][:n_it]) < 1e-6
        assert (logs[n_it - 1:, b] == logs[n_it - 1, b]).all()                    # stopped where the reference stopped
        assert rel(s.x_nom[b], g[f"{name}_x_fin"][b]) < 1e-5 and rel(s.u_nom[b], g[f"{name}_u_fin"][b]) < 1e-4


def _check_final(s, g, prefix, bsel, n_outer, J, tols):
    e = s.engine
    o = n_outer - 1
    for i, b in enumerate(bsel):
        T = lambda k: tols.get(k, TOL)   # noqa: E731

        def err(mine, key):
            ref_all = g[f"{prefix}_{key}"]
            return float(np.max(np.abs(mine - ref_all[b, o]))) / max(1.0, float(np.nanmax(np.abs(ref_all))))
        assert float(np.max(np.abs(e.xhat[i].cpu().numpy() - g[f"{prefix}_xx"][b, o, J - 1]))) / max(1.0, float(np.nanmax(np.abs(g[f"{prefix}_xx"])))) < T("xx")
        assert float(np.max(np.abs(e.uhat[i].cpu().numpy() - g[f"{prefix}_xu"][b, o, J - 1]))) / max(1.0, float(np.nanmax(np.abs(g[f"{prefix}_xu"])))) < T("xu")
        assert err(e.K[i].cpu().numpy(), "K") < T("K")
        assert err(e.cost[i].cpu().numpy(), "cost") < T("cost")
        if e.zu is not None:
            assert err(e.zu[i].cpu().numpy(), "zu") < T("xu") and err(e.lu[i].cpu().numpy(), "lu") < T("xu")
        if e.zx is not None:
            assert err(e.zx[i].cpu().numpy(), "zx") < T("xx") and err(e.lx[i].cpu().numpy(), "lx") < T("xx")


def _tols(g, prefix):
    if f"{prefix}_sens" not in g.files:
        return {}
    return {str(k): max(TOL, 10.0 * float(v)) for k, v in zip(g[f"{prefix}_sens_keys"], g[f"{prefix}_sens"])}


def test_ilqr_admm_di3d(golden):
    from isls import Box
    g = golden("g3_di3d.npz")
    cfg = P.config2(batch=int(g["cfg_batch"]), N=100, seed=int(g["cfg_seed"]))
    s = make_isls(cfg, [0, 1])
    logs = s.ilqr_admm(project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=3, max_line_search_iter=20, max_admm_iter=5,
                       rho_u=cfg["rho_u"], alpha=cfg["relax"], tol=0.0, log=True)
    _check_final(s, g, "o2", [0, 1], 3, 5, _tols(g, "o2"))
    assert rel(np.stack(logs).transpose(1, 0, 2), g["o2_logs"][:, 2]) < TOL
    # batch invariance: the same trajectory solved alone gives the same bits
    s1 = make_isls(cfg, [1])
    s1.ilqr_admm(project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=3, max_line_search_iter=20, max_admm_iter=5,
                 rho_u=cfg["rho_u"], alpha=cfg["relax"], tol=0.0)
    assert np.array_equal(s1.x_nom, s.x_nom[1]) and np.array_equal(s1.u_nom, s.u_nom[1])
    # notebook-style call: lambda projection, notebook-era keyword names, natural stopping
    import isls
    s = make_isls(cfg, [0])
    logs = s.ilqr_admm(project_u=lambda u: isls.project_bound(u, cfg["u_lo"], cfg["u_hi"]), k_max=8, max_line_search=20,
                       max_admm_iter=10, rho_u=cfg["rho_u"], alpha=cfg["relax"], threshold=1e-3, log=True)
    n_outer = int(g["o2stop_n_outer"][0])
    assert len(s.cost_log) == n_outer + 1
    assert np.allclose(s.cost_log[1:], g["o2stop_cost"][0, :n_outer], rtol=1e-9)
    ji = int(g["o2stop_n_inner"][0, n_outer - 1])
    assert len(logs) == ji and rel(np.stack(logs), g["o2stop_logs"][0, n_outer - 1, :ji]) < TOL


def test_ilqr_admm_state_box_relaxed(golden):
    from isls import Box
    g = golden("g3_di3d.npz")
    cfg = P.config2(batch=int(g["cfg_batch"]), N=100, seed=int(g["cfg_seed"]))
    s = make_isls(cfg, [0, 1])
    s.ilqr_admm(project_x=Box(g["o2x_x_lo"], g["o2x_x_hi"]), project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=2,
                max_line_search_iter=20, max_admm_iter=4, rho_x=0.05, rho_u=cfg["rho_u"], alpha=1.5, tol=0.0)
    _check_final(s, g, "o2x", [0, 1], 2, 4, {})


def test_ilqr_admm_arm_and_car(golden):
    from isls import Box
    for name, cfg in (("g4_arm3r.npz", P.config3(batch=2, N=100, seed=0)), ("g5_car.npz", P.config4(batch=2, N=200, seed=0))):
        g = golden(name)
        s = make_isls(cfg, [0, 1])
        L = cfg.get("max_line_search", 20)
        s.ilqr_admm(project_x=Box(cfg["x_lo"], cfg["x_hi"]), project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=3,
                    max_line_search_iter=L, max_admm_iter=cfg["max_admm_iter"], rho_x=cfg["rho_x"], rho_u=cfg["rho_u"],
                    alpha=1.0, tol=0.0)
        _check_final(s, g, "o2", [0, 1], 3, cfg["max_admm_iter"], _tols(g, "o2"))


def test_ilqr_admm_car_keepout_state_constraint(golden):
    """Config 4 with the notebook's state constraint (two rotated keep-out rectangles, project_set_convex) running
    entirely on the device (ISLS_PROJ_SETS), against the reference's O2 trace; the same ConvexSets object passed as an
    opaque callable takes the host route and must agree."""
    import sys
    pj = sys.modules["isls.projections"]
    g = golden("g5_car.npz")
    cfg = P.config4(batch=2, N=200, seed=0)
    rho_x = np.zeros((200, 4, 4)); rho_x[:, :2, :2] = 0.1 * np.eye(2)
    cs = pj.keepout_rectangles(4, [[-7.0, -3.0], [-3.0, -7.0]], [[2.0, 1.0], [2.0, 1.0]], -np.pi / 4)
    s = make_isls(cfg, [0, 1])
    s.ilqr_admm(project_x=cs, max_iter=3, max_line_search_iter=20, max_admm_iter=10, rho_x=rho_x, alpha=1.0, tol=0.0)
    _check_final(s, g, "o2k", [0, 1], 3, 10, _tols(g, "o2k"))
    h = make_isls(cfg, [0, 1])
    h.ilqr_admm(project_x=lambda x: cs(x), max_iter=3, max_line_search_iter=20, max_admm_iter=10, rho_x=rho_x, alpha=1.0,
                tol=0.0)
    assert rel(s.x_nom, h.x_nom) < 1e-9 and rel(s.u_nom, h.u_nom) < 1e-9


def test_ilqr_admm_host_projection_path(golden):
    """A projection the device has no kernel for goes through the caller's numpy function; on a box it must agree
    with the device path."""
    from isls import Box
    g = golden("g3_di3d.npz")
    cfg = P.config2(batch=int(g["cfg_batch"]), N=100, seed=int(g["cfg_seed"]))

    def opaque(u):
        if np.max(np.abs(u)) > 1e200:            # defeats identify_box: this callable stays opaque
            raise ValueError("not probing")
        return np.clip(u, cfg["u_lo"], cfg["u_hi"])
    s = make_isls(cfg, [0, 1])
    s.ilqr_admm(project_u=opaque, max_iter=2, max_line_search_iter=20, max_admm_iter=5, rho_u=cfg["rho_u"], tol=0.0)
    d = make_isls(cfg, [0, 1])
    d.ilqr_admm(project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=2, max_line_search_iter=20, max_admm_iter=5,
                rho_u=cfg["rho_u"], tol=0.0)
    assert rel(s.x_nom, d.x_nom) < 1e-12 and rel(s.u_nom, d.u_nom) < 1e-12


@pytest.mark.parametrize("n,m", [(5, 2), (12, 6)])
def test_any_dimension_through_the_class_surface(oracle, n, m):
    """iSLS with a state / control dimension that has no instantiation of the fast kernels (the reference takes any,
    isls/base.py:11-14): `solve` (plain DP iLQR) and `ilqr_admm` (box on u) run on the generic kernels through the same class
    surface and the C driver, and reproduce the oracle's outer loop on the same problem (nominal, cost log, K)."""
    from helpers import OracleDriver, problem_arrays
    from isls import Box
    cfg = P.config_generic(n, m, batch=4, N=40, seed=2)
    s = make_isls(cfg, [0, 1, 2])
    assert not s.engine.fast_dims and s.engine.ff_record() is None
    s.ilqr_admm(project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=2, max_line_search_iter=9, max_admm_iter=3, rho_u=cfg["rho_u"],
                alpha=cfg["relax"], tol=0.0)
    d = OracleDriver(oracle, problem_arrays(cfg, range(3)), rho_u=cfg["rho_u"], relax=cfg["relax"])
    d.run(2, 9, 3, 0.0)
    assert rel(s.x_nom, d.xhat) < TOL and rel(s.u_nom, d.uhat) < TOL and rel(s.K, d.K) < TOL
    assert rel(np.array(s.cost_log)[-1], d.cost) < TOL
    assert (s.status == 0).all()


def test_unbuilt_paths_fail_loudly():
    import isls
    s = isls.iSLS(6, 3, 20)
    with pytest.raises(TypeError):
        s.forward_model = 3.0                                   # neither a model descriptor nor a callable
    with pytest.raises(NotImplementedError):
        s.solve(method='sls')
    s.forward_model = lambda x, u: x                            # a callable model has no built-in linearisation
    s.set_cost_variables(np.zeros((1, 6)), np.zeros((1, 6, 6)), np.zeros(20, dtype=np.int32), 1e-3)
    s.nominal_values = np.zeros((20, 6)), np.zeros((20, 3))
    with pytest.raises(ValueError):
        s.solve(None, max_iter=1)
    s.cost_function = lambda x, u: np.zeros(x.shape[0])         # a callable cost needs its get_Cs
    with pytest.raises(ValueError):
        s.ilqr_admm(lambda x, u: (np.zeros((20, 6, 6)), np.zeros((20, 6, 3))), max_iter=1)


def test_sls_config5_api(golden):
    """`SLS.solve_sls / ADMM_SLS / controller / get_trajectory_sls` (config 5) through the reference's class surface on a
    batch of problems that differ in target, bound, variance and confidence; fp64 and fp32."""
    import sys
    from isls import SLS
    pj = sys.modules["isls.projections"]
    g = golden("g7_sls_d1.npz")
    N, P_ = int(g["N"]), g["targets"].shape[0]
    for dtype, tol in ((np.float64, 1e-2), (np.float32, 1e-2)):
        s = SLS(2, 1, N, batch=P_, dtype=dtype)
        s.AB = [g["A"], g["B"]]
        zs = np.stack([np.stack([np.zeros(2), t]) for t in g["targets"]])
        seq = np.zeros(N, dtype=np.int32); seq[N - 1] = 1
        s.set_quadratic_cost(zs, np.stack([np.zeros((2, 2)), 1e6 * np.eye(2)]), seq, float(g["u_std"]))
        PHI_U, du0 = s.solve_sls()
        assert rel(du0, g["du0"]) < 1e-7
        cs = pj.chance_constraint_rows(1, g["upper_u"], -g["upper_u"], g["var_x0"], g["psi_inv"])
        du, phi_u, logs = s.ADMM_SLS(project_u=cs, max_iter=50, rho_u=1e2, alpha=1.0, tol=1e-3, log=True)
        assert du.shape == (P_, N) and phi_u.shape == (P_, N, 2 * N)
        # the stop iteration is decided by rounding noise (tests/test_oracle_golden.py::_check_sls_admm): the solution
        # is compared at the stationary tail, where it still drifts by ~3e-4 per 6 iterations
        for b in range(P_):
            if dtype == np.float32 and int(g["n_it"][b]) == 50:
                continue                                        # infeasible bound, no contraction: not trackable in fp32
            assert rel(du[b], g["du"][b]) < tol and rel(phi_u[b][:, :1], g["phi_u"][b][:, :1]) < tol
            assert 0.4 * int(g["n_it"][b]) <= int(s.sls_iters[b]) <= 50
        # with both stop rules off and the reference's own iteration count every problem is reproduced at the metric's
        # precision: 1e-7 in fp64, in fp32 1e-4 or ten times the reference's measured fp32 sensitivity of the problem
        from test_oracle_golden import fp32_tols
        for b in range(P_):
            if dtype == np.float32 and int(g["n_it"][b]) == 50:
                continue                                        # no contraction (see above): fp64 only
            one = SLS(2, 1, N, dtype=dtype)
            one.AB = [g["A"], g["B"]]
            one.set_quadratic_cost(zs[b], np.stack([np.zeros((2, 2)), 1e6 * np.eye(2)]), seq, float(g["u_std"]))
            cs1 = pj.chance_constraint_rows(1, g["upper_u"][b:b + 1], -g["upper_u"][b:b + 1], g["var_x0"][b:b + 1], g["psi_inv"][b:b + 1])
            du1, phi1 = one.ADMM_SLS(project_u=cs1, max_iter=int(g["n_it"][b]), rho_u=1e2, alpha=1.0, tol=0.0, rel_tol=0.0)
            xt = 1e-7 if dtype == np.float64 else fp32_tols(g)[b]
            assert int(one.sls_iters[0]) == int(g["n_it"][b])
            assert rel(du1, g["du"][b]) < xt and rel(phi1[:, :1], g["phi_u"][b][:, :1]) < xt, (b, rel(du1, g["du"][b]), xt)
        if dtype == np.float64:
            K, k = s.controller(phi_u[1], du[1])                 # problem 1 ran all 50 iterations in both
            assert rel(K, g["K"][1]) < 1e-3
            one = SLS(2, 1, N, dtype=dtype)
            one.AB = [g["A"], g["B"]]
            xl, ul = one.get_trajectory_sls(g["mc_x0"][1], g["K"][1], g["k"][1])
            assert rel(xl, g["mc_x"][1]) < 1e-9 and rel(ul, g["mc_u"][1]) < 1e-9


def test_tassa_car_parking_api(golden):
    """notebooks/Tutorial.ipynb through the class surface: TassaCar model, PseudoHuber cost, `solve(get_AB, get_Cs)` and
    `ilqr_admm(get_Cs=..., project_u=box)` against the reference run on the notebook's own callbacks."""
    from isls import Box, costs, iSLS, models
    g = golden("g8_tassa.npz")
    N = int(g["N"])
    cost = costs.PseudoHuber(g["par_cu"], g["par_cx"], g["par_px"], g["par_cf"], g["par_pf"])
    mdl = models.TassaCar(float(g["dt"]), float(g["dist"]))
    # host versions of the callbacks agree with the reference-side ones
    A, B = mdl.get_AB(g["fd_x"], g["fd_u"])
    cs, Cs = cost.get_Cs(g["fd_x"], g["fd_u"])
    assert rel(A, g["fd_A"]) < 1e-13 and rel(B, g["fd_B"]) < 1e-13 and rel(cs, g["fd_cs"]) < 1e-13 and rel(Cs, g["fd_Cs"]) < 1e-13

    def fresh():
        s = iSLS(4, 2, N, batch=2)
        s.forward_model = mdl
        s.cost_function = cost
        s.nominal_values = g["x_nom0"], g["u0"]
        return s
    s = fresh()
    assert rel(s.cost, g["cost0"]) < 1e-12 and rel(cost(g["x_nom0"], g["u0"]), g["cost0"]) < 1e-12
    s.solve(get_Cs=cost.get_Cs, max_iter=6, max_line_search_iter=40, method='dp')
    assert rel(s.cost, g["cost_log"][:, 6]) < 1e-7 and rel(s.x_nom, g["x_fin"]) < 1e-5 and rel(s.u_nom, g["u_fin"]) < 1e-5
    s = fresh()
    s.ilqr_admm(get_Cs=cost.get_Cs, project_u=Box(np.array([-0.5, -2.0]), np.array([0.5, 2.0])), max_iter=3,
                max_line_search_iter=40, max_admm_iter=5, rho_u=np.diag([1e-1, 1e-2]), tol=0.0)
    _check_final(s, g, "o2", [0, 1], 3, 5, {k: 1e-7 for k in ("xx", "xu", "K", "cost")})


def test_admm_lqt_dp_with_convex_sets(golden):
    """`SLS.ADMM_LQT_DP` with a `ConvexSets` control constraint (ISLS_PROJ_SETS): a single box set through
    project_set_convex must land on the same solution as the plain box projection."""
    import sys
    from isls import SLS
    pj = sys.modules["isls.projections"]
    c = P.config1(50)
    outs = []
    for proj in (pj.Box(-5.0, 5.0),
                 pj.ConvexSets(1, (0, 1), [dict(kind=pj.SET_BOX, dim=1, A=np.eye(1), b=np.zeros(1), par=np.array([-5.0, 5.0]))],
                               rho=1.0, max_iter=200, threshold=1e-10)):
        s = SLS(2, 1, 50)
        s.AB = [c["A"], c["B"]]
        s.set_quadratic_cost(c["zs"], c["Qs"], c["seq"], c["u_std"])
        outs.append(s.ADMM_LQT_DP(np.zeros(2), project_u=proj, max_iter=300, rho_u=c["rho_u"], tol=1e-6))
    assert rel(outs[0][1], outs[1][1]) < 1e-6 and np.max(np.abs(outs[1][1])) < 5.0 + 1e-4


@pytest.mark.parametrize("nseg", ["3", "1"])
def test_headline_size_properties(monkeypatch, nseg):
    """BASELINE.json's full size (B = 4096, N = 100, n = 6, m = 3, fp64) through size-independent properties:
    batch invariance (a trajectory solved inside the 4096-batch equals the same trajectory solved in a batch of 5, bit for
    bit: slots never interact), the consensus variable is inside the box exactly, every cost is finite and below the
    initial one, no status bit is raised, and the ADMM primal residual does not grow over the inner iterations.
    nseg "3": the time-parallel feed-forward passes (dense records) in both batches; "1": the sequential passes on the model's
    structure (lean records) in both -- the form bench.py times."""
    from isls import Box
    # the engine picks the number of time-parallel feed-forward segments from the batch size, which changes the association
    # of a few sums; with the same segmentation the results are bit-identical
    monkeypatch.setenv("ISLS_FF_NSEG", nseg)
    B = 4096
    cfg = P.config2(batch=B, N=100, seed=0)
    box = Box(cfg["u_lo"], cfg["u_hi"])
    kw = dict(max_iter=3, max_line_search_iter=20, max_admm_iter=5, rho_u=cfg["rho_u"], alpha=cfg["relax"], tol=0.0)
    big = make_isls(cfg, range(B))
    c0 = np.array(big.cost, dtype=np.float64).copy()
    logs = big.ilqr_admm(project_u=box, log=True, **kw)
    sel = [0, 1, 777, 2048, 4095]
    small = make_isls(cfg, sel)
    small.ilqr_admm(project_u=box, **kw)
    e, es = big.engine, small.engine
    if nseg == "1":
        assert e._outer_args.gain.lin_on == 1 and e._outer_args.ff.lin_on == 1 and es._outer_args.gain.lin_on == 1
    for name in ("xhat", "uhat", "K", "k", "zu", "lu", "cost"):
        a, b_ = getattr(e, name)[sel].cpu().numpy(), getattr(es, name).cpu().numpy()
        assert np.array_equal(a, b_), name
    zu = e.zu.cpu().numpy()
    assert np.all(zu >= cfg["u_lo"]) and np.all(zu <= cfg["u_hi"])
    c1 = np.array(big.cost, dtype=np.float64)
    assert np.all(np.isfinite(c1)) and np.all(c1 < c0) and not e.status.cpu().numpy().any()
    lg = np.stack(logs)                                            # [J, B, 2] of the last outer iteration
    assert lg.shape == (5, B, 2) and np.all(np.isfinite(lg)) and np.all(lg >= 0)
    act = lg[0, :, 0] > 1e-9                                       # trajectories whose control bound is active at all
    assert act.any() and np.median(lg[-1, act, 0]) <= np.median(lg[0, act, 0])
