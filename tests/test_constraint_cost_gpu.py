"""Costs with nonlinear path constraints (isls.costs.Custom(constraints=K)) on the device, against the numpy restatement of
tests/al_reference.py: the multiplier and penalty update at the edges of its lane stride, zero multipliers against the same stage
registered without constraints (bit for bit), value, expansion and line search of the augmented cost, iSLS.solve_al against the
restatement's outer loop through the host route of solve, and the composition with ilqr_admm, mpc and set_table."""
import numpy as np
import pytest
import torch

from test_isls_api import rel as _rel

import al_reference as al

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-10, torch.float32: 1e-4}


def rel(a, b):
    """test_isls_api.rel; nothing to compare: 0"""
    return 0.0 if np.size(b) == 0 else _rel(a, b)


def make_cost(n, m, W, K, table=None, constraints=True):
    from isls import costs
    if not constraints:
        return costs.Custom(n, m, al.PAR, al.full_source(n, m, W, K, constraints=False), table=table)
    return costs.Custom(n, m, al.PAR, al.full_source(n, m, W, K), table=table, constraints=K)


# ---- 1. the update kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m, W, K", [(4, 2, 0, 1), (4, 2, 0, 3), (4, 2, 1, 2), (4, 2, 12, 3), (9, 3, 0, 3), (9, 3, 1, 2)])
def test_update_kernel_against_numpy(n, m, W, K):
    """N at the edges of the lane stride (one wavefront walks the steps 64 at a time), B = 1 and 5; per shape: an update with some
    penalties growing, some capped at mu_max and some staying; an active mask with zeros (rows bit for bit); update = 0 (the table
    bit for bit); a NaN in g (violation +inf, its multipliers stay)."""
    from isls import _capi as capi
    from isls.engine import kernels
    kern, dev = kernels(), torch.device("cuda")
    eta, phi, mu_max = 0.25, 10.0, 30.0
    for dt in (torch.float64, torch.float32):
        cst = make_cost(n, m, W, K, table=np.zeros((1, W)) if W else None)
        capi.user_cost_load(cst.cost_model, -1, dt)
        for N in (1, 2, 63, 64, 65, 130):
            for B in (1, 5):
                rng = np.random.default_rng(1000 * N + 10 * B + W + K)
                x, u = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
                nan_at = (B - 1, N // 2)
                x[nan_at][0] = np.nan
                tab = np.zeros((B, N, W + K + 1))
                tab[..., :W] = 0.1 * rng.normal(size=(B, N, W))
                tab[..., W:W + K] = np.abs(rng.normal(size=(B, N, K))) * (rng.random((B, N, K)) < 0.6)
                mu = np.array([0.5, 2.0, 5.0, 1.0, 4.0])[:B].copy()          # 5.0 and 4.0 * phi pass mu_max = 30
                tab[..., W + K] = mu[:, None]
                t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)   # noqa: E731
                xt, ut, par = t(x), t(u), t(al.PAR)
                xr, ur, tr = (v.double().cpu().numpy() for v in (xt, ut, t(tab)))           # what the kernel reads, in its precision
                g_ref = al.constraint(xr, ur, al.PAR, tr[..., :W], W, K)[0]
                v_ref = np.where(np.isnan(g_ref), np.inf, np.maximum(g_ref, 0)).reshape(B, -1).max(-1)
                assert np.isinf(v_ref[-1])
                prev = np.where(np.isfinite(v_ref), v_ref * np.array([0.1, 100.0, 0.1, 0.1, 0.1])[:B], 1.0)
                active = np.array([1, 1, 0, 1, 1])[:B] if B > 1 else None
                lam2, mu2, viol, prev2 = al.update(g_ref, tr[..., W:W + K], tr[:, 0, W + K], prev, eta, phi, mu_max, active=active)
                for upd in (0, 1):
                    tt, vt, pt = t(tab), torch.full((B,), -7.0, dtype=dt, device=dev), t(prev)
                    gt = torch.full((B, N, K), -7.0, dtype=dt, device=dev)
                    kern.user_constraint_update(cst.cost_model, par, tt, xt, ut, vt, pt, update=upd, eta=eta, phi=phi, mu_max=mu_max,
                                                g_out=gt, active=None if active is None else torch.as_tensor(active, dtype=torch.int32, device=dev))
                    torch.cuda.synchronize()
                    out, g_out = tt.double().cpu().numpy(), gt.double().cpu().numpy()
                    on = np.ones(B, dtype=bool) if active is None else active.astype(bool)
                    what = f"({n},{m}) W={W} K={K} N={N} B={B} {dt} update={upd}"
                    off = torch.as_tensor(~on, device=dev)
                    assert torch.equal(tt[off], t(tab)[off]), what                               # masked: bit for bit
                    assert (gt[off] == -7.0).all() and (vt[off] == -7.0).all(), what
                    assert np.array_equal(np.isnan(g_out[on]), np.isnan(g_ref[on])), what
                    assert rel(np.nan_to_num(g_out[on]), np.nan_to_num(g_ref[on])) < TOL[dt], what
                    vo, po = vt.double().cpu().numpy(), pt.double().cpu().numpy()
                    fin = on & np.isfinite(v_ref)
                    assert np.array_equal(np.isinf(vo[on]), np.isinf(v_ref[on])) and rel(vo[fin], v_ref[fin]) < TOL[dt], what
                    assert np.array_equal(np.isinf(po), np.isinf(prev2)) and rel(po[np.isfinite(prev2)], prev2[np.isfinite(prev2)]) < TOL[dt], what
                    if not upd:
                        assert torch.equal(tt, t(tab)), what                                    # update = 0: the table bit for bit
                        continue
                    assert np.array_equal(out[..., :W], tr[..., :W]), what                      # the user's columns: never written
                    assert rel(out[..., W:W + K], lam2) < TOL[dt], what
                    assert rel(out[..., W + K], np.broadcast_to(mu2[:, None], (B, N))) < TOL[dt], what
                    k_nan = np.isnan(g_ref[nan_at])
                    assert np.array_equal(out[nan_at][W:W + K][k_nan], tr[nan_at][W:W + K][k_nan]), what   # a NaN g leaves its lambda
                if B == 5:
                    assert mu2[2] == mu[2] and mu2[1] == mu[1] and mu2[4] == mu_max              # masked, stays, capped


# ---- 2. zero multipliers are the plain cost ------------------------------------------------------------------------------------
def car_pair(cst_a, cst_b, B, N, seed, dtype=np.float64):
    """Two iSLS on CarSimple with the same nominal and gains, one per cost"""
    from isls import iSLS, models
    rng = np.random.default_rng(seed)
    mdl = models.CarSimple(0.1)
    us = 0.3 * rng.normal(size=(B, N, 2))
    xs = np.zeros((B, N, 4))
    xs[:, 0] = rng.normal(size=(B, 4)) * [0.5, 0.5, 0.3, 0.5] + [0, 0, 0, 1.0]
    for t in range(N - 1):
        xs[:, t + 1] = mdl(xs[:, t], us[:, t])
    sides = []
    for c in (cst_a, cst_b):
        s = iSLS(4, 2, N, batch=B, dtype=dtype)
        s.forward_model = mdl
        s.cost_function = c
        s.nominal_values = xs, us
        s.engine.K.copy_(s.engine._t(0.2 * np.random.default_rng(seed + 1).normal(size=(B, N, 2, 4))))
        s.engine.k.copy_(s.engine._t(0.3 * np.random.default_rng(seed + 2).normal(size=(B, N, 2))))
        sides.append(s)
    return sides, xs, us


@pytest.mark.parametrize("W", [0, 1])
def test_zero_multipliers_are_the_plain_cost_bit_for_bit(W):
    from isls import _capi as capi
    B, N, L, K = 5, 12, 20, 3
    tab = 0.1 * np.random.default_rng(3).normal(size=(N, W)) if W else None
    con, plain = make_cost(4, 2, W, K, table=tab), make_cost(4, 2, W, K, table=tab, constraints=False)
    (sc, sp), xs, us = car_pair(con, plain, B, N, seed=5)
    assert sc.engine.cost_tab.shape == (B, N, W + K + 1) and float(sc.engine.cost_tab[..., W:].abs().max()) == 0.0
    assert np.array_equal(con(xs, us), plain(xs, us))
    assert torch.equal(sc.engine.cost, sp.engine.cost)
    ca, cb = (torch.zeros(B, L, dtype=torch.float64, device="cuda") for _ in range(2))
    flags = capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST
    sc.engine.rollout(L, flags=flags, cost_all=ca, active=sc.engine.outer_active)
    sp.engine.rollout(L, flags=flags, cost_all=cb, active=sp.engine.outer_active)
    torch.cuda.synchronize()
    assert torch.equal(ca, cb) and torch.equal(sc.engine.cost_new, sp.engine.cost_new) and torch.equal(sc.engine.best, sp.engine.best)
    assert torch.equal(sc.engine.xx, sp.engine.xx) and torch.equal(sc.engine.xu, sp.engine.xu)


# ---- 3. expansion and value against the analytic restatement -------------------------------------------------------------------
def multipliers(rng, B, N, K):
    lam = np.abs(rng.normal(size=(B, N, K))) * (rng.random((B, N, K)) < 0.5)
    return lam, np.array([0.7, 3.0, 11.0, 1.5, 2.5])[:B].copy()


@pytest.mark.parametrize("n, m, N, W", [(4, 2, 2, 0), (4, 2, 12, 1), (9, 3, 5, 0)])
def test_expansion_and_value_against_the_restatement(n, m, N, W):
    B, K = 3, 3
    rng = np.random.default_rng(n + N)
    x, u = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
    tab = 0.1 * rng.normal(size=(B, N, W)) if W else None
    cst = make_cost(n, m, W, K, table=tab)
    cst._lam, cst._mu = multipliers(rng, B, N, K)
    c, gr, H, h = al.augmented(x, u, al.PAR, tab, cst._lam, cst._mu, W, K)
    print(f"({n},{m}) N={N}: min |lambda + mu g| = {np.abs(h).min():.3e}; active {int((h > 0).sum())} of {h.size}")
    assert np.abs(h).min() > 1e-6 and (h > 0).any() and (h <= 0).any()
    cs, Cs = cst.get_Cs(x, u)
    val = cst(x, u)
    e = rel(val, c.sum(-1)), rel(cs, gr), rel(Cs, H)
    print("value %.2e gradient %.2e Hessian %.2e" % e)
    assert max(e) < 1e-10
    assert rel(cst.constraint(x, u), al.constraint(x, u, al.PAR, tab, W, K)[0]) < 1e-10


# ---- 4. line search ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [0, 1])
@pytest.mark.parametrize("preset_last", [False, True], ids=["recorded", "replayed"])
def test_line_search_against_numpy(W, preset_last):
    """Every candidate's augmented cost, the arg-min and the winner's states against numpy rollouts of the car.  preset_last: `best`
    preset to the last candidate, which loses -- the prediction misses and the winner is replayed."""
    from isls import _capi as capi
    from isls import models
    B, N, L, K = 4, 12, 20, 3
    rng = np.random.default_rng(40 + W)
    tab = 0.1 * rng.normal(size=(B, N, W)) if W else None
    cst = make_cost(4, 2, W, K, table=tab)
    (s, _), xs, us = car_pair(cst, make_cost(4, 2, W, K, table=tab, constraints=False), B, N, seed=9)
    cst._lam, cst._mu = multipliers(rng, B, N, K)
    cst._mult_version += 1                                         # as reset_multipliers does: the iSLS copies them in
    e = s.engine
    s._sync_tables()
    lam, mu = cst.multipliers, cst.penalty
    assert rel(e.cost_tab[..., W:W + K].cpu().numpy(), lam) == 0.0
    Kg, kg, alphas = e.K.cpu().numpy(), e.k.cpu().numpy(), np.asarray(s.alphas[:L])
    mdl = models.CarSimple(0.1)
    xl, ul = np.zeros((B, L, N, 4)), np.zeros((B, L, N, 2))
    xcur = np.repeat(xs[:, None, 0], L, axis=1)
    for t in range(N):
        ucur = (np.einsum("blj,bij->bli", xcur - xs[:, None, t], Kg[:, t]) + alphas[None, :, None] * kg[:, None, t]) + us[:, None, t]
        xl[:, :, t], ul[:, :, t] = xcur, ucur
        xcur = mdl(xcur, ucur)
    row = None if tab is None else tab[:, None]
    ref = al.augmented(xl, ul, al.PAR, row, lam[:, None], mu[:, None], W, K)[0].sum(-1)
    ca = torch.zeros(B, L, dtype=torch.float64, device="cuda")
    if preset_last:
        e.best.fill_(L - 1)
    e.rollout(L, flags=capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST, cost_all=ca, active=e.outer_active)
    torch.cuda.synchronize()
    got, best = ca.cpu().numpy(), e.best.cpu().numpy()
    srt = np.sort(ref, axis=1)
    assert ((srt[:, 1] - srt[:, 0]) > 1e-8 * np.abs(srt[:, 0])).all()                       # tie-free inputs
    assert rel(got, ref) < 1e-10
    cur = al.augmented(xs, us, al.PAR, tab, lam, mu, W, K)[0].sum(-1)
    assert rel(e.cost.cpu().numpy(), cur) < 1e-10
    win = np.argmin(ref, axis=1)
    ok = ref[np.arange(B), win] < cur
    assert ok.any() and np.array_equal(best[ok], win[ok])
    assert np.array_equal(((e.status.cpu().numpy() & capi.ST_LS_REJECT) == 0), ok)
    rows = np.arange(B)
    assert rel(e.xx.cpu().numpy()[ok], xl[rows, win][ok]) < 1e-10 and rel(e.xu.cpu().numpy()[ok], ul[rows, win][ok]) < 1e-10
    assert rel(e.cost_new.cpu().numpy()[ok], ref[rows, win][ok]) < 1e-10


# ---- 5. solve_al end to end ----------------------------------------------------------------------------------------------------
def e2e_device():
    from isls import iSLS, models
    p = al.E2E
    A, Bm = al.double_integrator()
    N, B, K = p["N"], p["B"], p["K"]
    x0 = al.e2e_starts()
    q = iSLS(4, 2, N, batch=B)
    q.forward_model = models.LTI(A, Bm)
    cst = make_cost(4, 2, 0, K)
    q.cost_function = cst
    q.nominal_values = np.stack([al.rollout(A, Bm, x0[b], np.zeros((N, 2))) for b in range(B)]), np.zeros((B, N, 2))
    return q, cst, A, Bm, x0


def host_route_outer_loop(rounds, stop):
    """The restatement's outer loop with the host route of iSLS.solve as its inner solver: the augmented cost and its analytic
    expansion as Python callables, one iSLS of batch 1 per trajectory"""
    from isls import Regularization, iSLS, models
    p = al.E2E
    A, Bm = al.double_integrator()
    N, B, K = p["N"], p["B"], p["K"]
    x0 = al.e2e_starts()
    cur = dict(lam=np.zeros((B, N, K)), mu=np.full(B, p["mu0"]))
    hosts = []
    for b in range(B):
        s = iSLS(4, 2, N, batch=1)
        s.forward_model = models.LTI(A, Bm)
        s.cost_function = lambda x, u, b=b: al.augmented(x, u, al.PAR, None, cur["lam"][b], cur["mu"][b], 0, K)[0].sum(-1)
        s.al_get_Cs = lambda x, u, b=b: al.augmented(x, u, al.PAR, None, cur["lam"][b], cur["mu"][b], 0, K)[1:3]
        s.nominal_values = al.rollout(A, Bm, x0[b], np.zeros((N, 2))), np.zeros((N, 2))
        hosts.append(s)

    def solve(lam, mu):
        cur["lam"], cur["mu"] = lam, mu
        for s in hosts:
            s.nominal_values = s.x_nom, s.u_nom                     # the nominal's cost under the new multipliers
            s.solve(get_Cs=s.al_get_Cs, max_iter=p["max_iter"], regularization=Regularization())
        return np.stack([s.x_nom for s in hosts]), np.stack([s.u_nom for s in hosts])

    evaluate = lambda x, u: al.constraint(x, u, al.PAR, None, 0, K)[0]   # noqa: E731
    return al.outer_loop(solve, evaluate, cur["lam"], cur["mu"], rounds, p["tol_con"], p["eta"], p["phi"], p["mu_max"], stop=stop)


def test_solve_al_against_the_host_route_restatement():
    """Four rounds of twenty inner iterations on both sides (with the default Regularization: the disc's curvature makes Quu
    indefinite on the way), then the comparison; tolerance 1e-9, what the device-against-host-route
    tests of `solve` assert on x_nom, u_nom and the cost (test_user_cost_gpu.py, test_user_model_gpu.py)."""
    p = al.E2E
    R = 4
    q, cst, *_ = e2e_device()
    from isls import Regularization
    r = q.solve_al(max_outer=R, max_iter=p["max_iter"], tol_con=0.0, mu0=p["mu0"], phi=p["phi"], mu_max=p["mu_max"], eta=p["eta"],
                   regularization=Regularization())
    x, u, lam, mu, viol, rounds = host_route_outer_loop(R, stop=False)
    errs = dict(viol=rel(r.viol, viol), mu=rel(r.mu, mu), x=rel(q.x_nom, x), u=rel(q.u_nom, u), lam=rel(cst.multipliers, lam))
    print("solve_al against the host route after", R, "rounds:", {k: f"{v:.2e}" for k, v in errs.items()}, "viol", r.viol[:, -1])
    assert r.viol.shape == (p["B"], R) and np.array_equal(r.rounds, np.full(p["B"], R))
    assert max(errs.values()) < 1e-9


def test_solve_al_converges():
    from isls import Regularization
    p = al.E2E
    q, cst, *_ = e2e_device()
    r = q.solve_al(max_outer=p["max_outer"], max_iter=p["max_iter"], tol_con=p["tol_con"], mu0=p["mu0"], phi=p["phi"],
                   mu_max=p["mu_max"], eta=p["eta"], regularization=Regularization())
    print("viol per round:\n", r.viol, "\nmu", r.mu, "rounds", r.rounds)
    assert r.converged.all() and (r.viol[:, -1] <= p["tol_con"]).all() and (r.viol[:, 0] > p["tol_con"]).all()
    assert (cst.constraint(q.x_nom, q.u_nom) <= p["tol_con"]).all()
    assert rel(cst.penalty, r.mu) == 0.0 and cst.multipliers.max() > 0
    assert rel(q.cost, cst(q.x_nom, q.u_nom)) < 1e-10            # the object's multipliers are the device's


# ---- 6. composition ------------------------------------------------------------------------------------------------------------
def test_ilqr_admm_after_solve_al_keeps_the_constraints():
    from isls import Box, Regularization
    p = al.E2E
    q, cst, *_ = e2e_device()
    q.solve_al(max_outer=p["max_outer"], max_iter=p["max_iter"], tol_con=p["tol_con"], regularization=Regularization())
    ub = np.abs(q.u_nom).max()                                    # a box the plan touches
    tol = 1e-3
    q.ilqr_admm(project_u=Box(np.full(2, -ub), np.full(2, ub)), rho_u=1e-1 * np.eye(2), max_iter=10, max_admm_iter=20, tol=tol,
                regularization=Regularization())
    v = np.maximum(cst.constraint(q.x_nom, q.u_nom), 0).max()
    print("violation after ilqr_admm with a control box:", v, "max |u|", np.abs(q.u_nom).max(), "box", ub)
    assert v <= p["tol_con"] + tol


def test_mpc_moves_the_multipliers_with_the_window_and_set_table_leaves_them():
    from isls import iSLS, models
    B, N, W, K, T = 3, 8, 1, 2, 3
    rng = np.random.default_rng(8)
    A, Bm = al.double_integrator()
    tab = 0.05 * rng.normal(size=(N, W))
    cst = make_cost(4, 2, W, K, table=tab)
    q = iSLS(4, 2, N, batch=B)
    q.forward_model = models.LTI(A, Bm)
    q.cost_function = cst
    x0 = al.e2e_starts()[:B]
    q.nominal_values = np.stack([al.rollout(A, Bm, x0[b], np.zeros((N, 2))) for b in range(B)]), np.zeros((B, N, 2))
    cst._lam, cst._mu = 0.05 * np.abs(rng.normal(size=(B, N, K))), np.array([0.1, 0.2, 0.3])
    cst._mult_version += 1
    q._sync_tables()
    e = q.engine
    before = e.cost_tab.clone()
    # set_table: the user's columns only
    new = 0.05 * rng.normal(size=(N, W))
    cst.set_table(new)
    q._sync_tables()
    assert torch.equal(e.cost_tab[..., W:], before[..., W:])
    assert torch.equal(e.cost_tab[..., :W], torch.as_tensor(np.broadcast_to(new, (B, N, W)).copy(), device=e.device))
    before = e.cost_tab.clone()
    fut = 0.05 * rng.normal(size=(T, W))
    q.mpc(T, iters=1, max_admm_iter=2, table_future=fut)
    hand = torch.cat([before[:, T:], before[:, -1:].expand(B, T, W + K + 1)], dim=1).clone()
    hand[:, N - T:, :W] = torch.as_tensor(fut, device=e.device)
    assert torch.equal(e.cost_tab, hand)                           # lambda and mu one row per step, the last row held; bit for bit
    assert np.array_equal(cst.multipliers, hand[..., W:W + K].cpu().numpy()) and np.array_equal(cst.penalty, [0.1, 0.2, 0.3])
    assert np.array_equal(cst.table, hand[0, :, :W].cpu().numpy())


def test_refusals():
    from isls import _capi as capi
    q, cst, A, Bm, _ = e2e_device()
    with pytest.raises(capi.IslsError, match="isls_admm"):
        q.isls_admm(1)
    with pytest.raises(capi.IslsError, match="batch form"):
        q.solve(method="batch", max_iter=1)
    # the host routes: a forward model given as a Python callable, a projection given as one
    from isls import models
    lti = models.LTI(A, Bm)
    q.forward_model = lambda x, u: lti(x, u)
    with pytest.raises(capi.IslsError, match="host route"):
        q.solve(get_AB=lti.get_AB, max_iter=1)
    with pytest.raises(capi.IslsError, match="Python callable"):
        q.solve_al(max_outer=1)
    q.forward_model = lti
    with pytest.raises(capi.IslsError, match="through the host"):
        # (a ball: a clip would be recognised as a Box and run on the device)
        q.ilqr_admm(project_u=lambda v: v / np.maximum(1.0, np.linalg.norm(v, axis=-1, keepdims=True)), rho_u=1e-1 * np.eye(2),
                    max_iter=1)
    # mpc: a per-trajectory table_future against a cost whose own table is shared
    N = al.E2E["N"]
    shared = make_cost(4, 2, 1, 2, table=np.zeros((N, 1)))
    q.cost_function = shared
    with pytest.raises(ValueError, match="shared"):
        q.mpc(2, table_future=np.zeros((al.E2E["B"], 2, 1)))
    # one iSLS at a time: a second one of another batch does not silently reset the multipliers
    from isls import iSLS
    q2 = iSLS(4, 2, N, batch=2)
    with pytest.raises(capi.IslsError, match="one iSLS"):
        q2.cost_function = shared
    q.cost_function = lambda x, u: np.sum(x * x, axis=(-1, -2))
    with pytest.raises(capi.IslsError, match="Python callable"):
        q.solve_al()
