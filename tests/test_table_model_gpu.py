"""User models with a per-step table (isls.models.Custom(..., table=)) on the GPU: step and Jacobians against numpy closed forms,
the line search bit for bit against the same constants in `params`, time-varying rows against the numpy rollout (recorded and
replayed winners), a model table with a cost table, the class surface against the host route (solve, ilqr_admm), mpc bit for bit
against the hand-driven loop of the same kernels, the costs of every sample of sample_nominal, set_table and the refusals.
fp64 bound 1e-10, fp32 bound 1e-4, both relative to max(1, |ref|_max)."""
import numpy as np
import pytest
import torch

from isls import _capi as capi
from isls import Box, costs, iSLS, models
from isls.engine import Engine

import table_costs as tc
import table_models as tm
from sampling_reference import draws

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


# ---- 1. step and Jacobians -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ltv", "car"])
@pytest.mark.parametrize("N", [1, 5, 67])
@pytest.mark.parametrize("B", [1, 5])
def test_step_and_jacobians_against_numpy(which, N, B):
    rng = np.random.default_rng(N * 10 + B)
    src, mk, W = (tm.LTV, tm.ltv_table, 16) if which == "ltv" else (tm.CAR, tm.car_table, 2)
    x, u = rng.standard_normal((B, N, 4)), rng.standard_normal((B, N, 2))
    shared, per = mk(rng, N), mk(rng, N, B)
    for tab in (shared, per):
        mdl = models.Custom(4, 2, [0.0], src, table=tab)
        rows = np.broadcast_to(tab, (B, N, W))
        if which == "ltv":
            ref, (Ar, Br) = tm.ltv_step(x, u, rows), tm.ltv_AB(rows)
        else:
            ref, (Ar, Br) = tm.car_step(x, u, rows), tm.car_AB(x, u, rows)
        xn = mdl(x, u)
        A, Bm = mdl.get_AB(x, u)
        for got, want in ((xn, ref), (A, Ar), (Bm, Br)):
            assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
        # single rows with t=
        t = min(N - 1, 3)
        x1 = mdl(x[:, t], u[:, t], t=t)
        assert np.array_equal(x1, xn[:, t])
        A1, B1 = mdl.get_AB(x[:, t], u[:, t], t=t)
        assert np.array_equal(A1, A[:, t]) and np.array_equal(B1, Bm[:, t])
    # a per-trajectory table of identical rows is the shared one, bit for bit
    a = models.Custom(4, 2, [0.0], src, table=shared)
    b = models.Custom(4, 2, [0.0], src, table=np.broadcast_to(shared, (B, N, W)).copy())
    assert np.array_equal(a(x, u), b(x, u))
    for p, q in zip(a.get_AB(x, u), b.get_AB(x, u)):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("which", ["ltv", "car"])
@pytest.mark.parametrize("N, B", [(1, 1), (5, 5), (67, 5)])
def test_step_and_jacobians_fp32(which, N, B):
    """The fp32 entry points (isls_user_model_step_tab_f32, isls_linearize_f32) with a shared and a per-trajectory table."""
    rng = np.random.default_rng(N + B)
    src, mk, W = (tm.LTV, tm.ltv_table, 16) if which == "ltv" else (tm.CAR, tm.car_table, 2)
    x, u = rng.standard_normal((B, N, 4)), rng.standard_normal((B, N, 2))
    for tab in (mk(rng, N), mk(rng, N, B)):
        mdl = models.Custom(4, 2, [0.0], src, table=tab)
        rows = np.broadcast_to(tab, (B, N, W))
        if which == "ltv":
            ref, (Ar, Br) = tm.ltv_step(x, u, rows), tm.ltv_AB(rows)
        else:
            ref, (Ar, Br) = tm.car_step(x, u, rows), tm.car_AB(x, u, rows)
        e = Engine(B, N, 4, 2, dtype=torch.float32)
        e.set_model(mdl.model_id, mdl.device_params(B if tab.ndim == 3 else None, N))
        e.xhat.copy_(e._t(x)), e.uhat.copy_(e._t(u))
        e.linearize()
        xn = torch.zeros(B * N, 4, dtype=torch.float32, device=e.device)
        e.kern.user_model_step_tab(mdl.model_id, e.model_par, e.xhat.reshape(B * N, 4), e.uhat.reshape(B * N, 2), xn, N, N,
                                   stream=torch.cuda.current_stream().cuda_stream)
        errs = rel(xn.cpu().numpy().reshape(B, N, 4), ref), rel(e.A.cpu().numpy(), Ar), rel(e.Bm.cpu().numpy(), Br)
        print(f"fp32 {which} N={N} B={B} table {tab.shape}: step {errs[0]:.2e} A {errs[1]:.2e} B {errs[2]:.2e}")
        assert max(errs) <= 1e-4


# ---- 2. the line search, bit for bit ---------------------------------------------------------------------------------------------
def _engine(mdl, par, B, N, n, m, rng_seed, box=False, dtype=torch.float64):
    rng = np.random.default_rng(rng_seed)
    e = Engine(B, N, n, m, dtype=dtype)
    e.set_model(mdl.model_id, par)
    e.set_quadratic_cost(rng.standard_normal((1, n)), np.eye(n)[None], np.zeros(N, dtype=np.int32), 0.01)
    e.K.copy_(e._t(0.05 * rng.standard_normal((B, N, m, n))))
    e.k.copy_(e._t(0.1 * rng.standard_normal((B, N, m))))
    e.set_nominal(0.3 * rng.standard_normal((B, N, n)), 0.1 * rng.standard_normal((B, N, m)))
    if box:
        e.set_admm(rho_u=1.0, u_box=(-0.2, 0.2))
    return e


@pytest.mark.parametrize("L", [1, 20, 40])
@pytest.mark.parametrize("N", [2, 5, 100])
@pytest.mark.parametrize("n, m", [(4, 2), (6, 3), (9, 3)])
@pytest.mark.parametrize("W", [1, 3, 16])
def test_line_search_bitwise_against_the_params_form(n, m, W, N, L):
    """One case per shape of the search (the first case of a pair and width pays its two run-time compiles); B = 1, 5, 65,
    with and without the fused update, inside."""
    c = tm.generic_consts(W)
    plain = models.Custom(n, m, c, tm.generic_source(n, m, W, False))
    tabm = models.Custom(n, m, [0.0], tm.generic_source(n, m, W, True), table=np.tile(c, (N, 1)))
    for B in (1, 5, 65):
        win = None                                           # the winners of the plain line search of this shape
        for fused in (False, True):
            for miss in ((False, True) if (N, L, B) == (100, 20, 65) else (False,)):
                out = []
                for mdl, par in ((plain, c), (tabm, tabm.device_params(B, N))):
                    e = _engine(mdl, par, B, N, n, m, 7, box=fused)
                    ca = torch.zeros(B, L, dtype=e.dtype, device=e.device)
                    if miss:                                 # predict the candidate behind the winner: every trajectory replays
                        e.best.copy_(torch.as_tensor((win + 1) % L, device=e.device))
                    if fused:
                        e.linearize(), e.expand()
                        e.build_outer(L, 2)
                        e.run_outer()
                        extra = [e.zu, e.lu, e.res]
                    else:
                        e.rollout(L, cost_all=ca)
                        extra = [ca]
                    out.append([t.cpu().numpy().copy() for t in [e.xx, e.xu, e.cost_new, e.best] + extra])
                for p, q in zip(*out):
                    assert np.array_equal(p, q, equal_nan=True), (N, L, B, fused, miss)
                if not fused and not miss:
                    win = out[0][3].copy()
                if miss and not fused:                           # the replay path gave the winners of the recorded path
                    assert np.array_equal(out[0][3], win) and np.array_equal(out[1][3], win)


# ---- 3. time-varying rows against the numpy rollout -------------------------------------------------------------------------------
def _search_against_numpy(e, step, tab, L, cost, tol, miss=False, what=""):
    """One line search over alphas[:L] on the engine as it stands against the numpy candidates: every candidate's cost, the
    arg-min (on inputs without a tie: asserted) and the winner's states and controls.  miss: `best` is preset to the candidate
    behind the reference's winner, so every trajectory misses its prediction and replays the winner."""
    B = e.B
    K, k, xh, uh = (t.double().cpu().numpy() for t in (e.K, e.k, e.xhat, e.uhat))
    alphas = e.alphas.double().cpu().numpy()[:L]
    def clear(ref):                                                 # the two best costs of a trajectory differ by more than 1e-6
        srt = np.sort(ref, axis=1)
        return (srt[:, 1] - srt[:, 0]) > 1e-6 * np.abs(srt[:, 0])
    for _ in range(6):
        # the inputs are made so that no arg-min can flip: a feed-forward that points uphill leaves the least cost among the
        # smallest, nearly equal steps -- such a trajectory gets its k turned round and lengthened until its winner stands clear
        xs, us = tm.candidates(step, tab, xh, uh, K, k, alphas)
        ref = cost(xs, us)                                          # [B, L]
        if clear(ref).all():
            break
        k[~clear(ref)] *= -3.0
        e.k.copy_(e._t(k))
    assert clear(ref).all()
    win = ref.argmin(1)
    if miss:
        e.best.copy_(torch.as_tensor(((win + 1) % L).astype(np.int32), device=e.device))
    ca = torch.zeros(B, L, dtype=e.dtype, device=e.device)
    e.rollout(L, cost_all=ca)
    rows = np.arange(B)
    errs = (rel(ca.cpu().numpy(), ref), rel(e.cost_new.cpu().numpy(), ref[rows, win]), rel(e.xx.cpu().numpy(), xs[rows, win]),
            rel(e.xu.cpu().numpy(), us[rows, win]))
    print(f"{what} L={L} miss={miss}: cost_all {errs[0]:.2e} cost_new {errs[1]:.2e} x {errs[2]:.2e} u {errs[3]:.2e}; best {win.tolist()}")
    assert max(errs) <= tol
    assert np.array_equal(e.best.cpu().numpy(), win)


def _quadratic(e):
    z, r = e.ztab.double().cpu().numpy()[0], 0.01
    return lambda xs, us: ((xs - z) ** 2).sum((-1, -2)) + r * (us ** 2).sum((-1, -2))


@pytest.mark.parametrize("miss", [False, True], ids=["recorded", "replayed"])
@pytest.mark.parametrize("switch", [0, "N-2"])
def test_line_search_time_varying_against_numpy(switch, miss):
    N, B, L, n, m = 12, 5, 20, 4, 2
    rng = np.random.default_rng(11)
    tab = tm.ltv_table(rng, N, B)
    ts = 0 if switch == 0 else N - 2
    tab[:, ts] *= -3.0                                              # a mode switch at one step
    mdl = models.Custom(n, m, [0.0], tm.LTV, table=tab)
    e = _engine(mdl, mdl.device_params(B, N), B, N, n, m, 5)
    _search_against_numpy(e, tm.ltv_step, tab, L, _quadratic(e), 1e-10, miss=miss, what=f"ltv switch at {ts}")


@pytest.mark.parametrize("miss", [False, True], ids=["recorded", "replayed"])
@pytest.mark.parametrize("n, m, W, N, L, B, shared", [(9, 3, 3, 100, 40, 5, False),     # the two-wave variants, the steady-state loop
                                                      (9, 3, 16, 5, 20, 65, True),      # a wide row, a partial last wavefront
                                                      (6, 3, 16, 100, 20, 5, False),
                                                      (4, 2, 1, 2, 20, 65, False)])     # the tail loop alone
def test_line_search_with_rows_that_differ_at_every_pair(n, m, W, N, L, B, shared, miss):
    """Rows that differ from step to step (and from trajectory to trajectory) where the bitwise grid above has constant ones: which
    row a step receives -- the ring index, the side record's parity, the clamped tail, the per-lane row of the replay -- shows."""
    rng = np.random.default_rng(n * N + L)
    tab = tm.generic_table(rng, N, W, None if shared else B) * (0.2 if N == 100 else 1.0)   # (a hundred steps: no blow-up)
    tab[..., N - 2, :] *= -2.0
    mdl = models.Custom(n, m, [0.0], tm.generic_source(n, m, W, True), table=tab)
    e = _engine(mdl, mdl.device_params(B, N), B, N, n, m, 5)
    _search_against_numpy(e, tm.generic_step(n, m, W), tab, L, _quadratic(e), 1e-10, miss=miss, what=f"({n},{m}) W={W} N={N} B={B}")


def test_line_search_fp32_against_numpy():
    N, B, L, n, m = 12, 5, 20, 4, 2
    rng = np.random.default_rng(12)
    tab = tm.ltv_table(rng, N, B)
    mdl = models.Custom(n, m, [0.0], tm.LTV, table=tab)
    e = _engine(mdl, mdl.device_params(B, N), B, N, n, m, 5, dtype=torch.float32)
    K, k, xh, uh = (t.double().cpu().numpy() for t in (e.K, e.k, e.xhat, e.uhat))
    xs, us = tm.candidates(tm.ltv_step, tab, xh, uh, K, k, e.alphas.double().cpu().numpy()[:L])
    ref = _quadratic(e)(xs, us)
    ca = torch.zeros(B, L, dtype=e.dtype, device=e.device)
    e.rollout(L, cost_all=ca)
    b = e.best.cpu().numpy()
    rows = np.arange(B)
    errs = rel(ca.cpu().numpy(), ref), rel(e.xx.cpu().numpy(), xs[rows, b]), rel(ref[rows, b], ref.min(1))
    print(f"fp32 line search: cost_all {errs[0]:.2e} x of the pick {errs[1]:.2e} the pick's cost against the least {errs[2]:.2e}")
    assert max(errs) <= 1e-4


# ---- 4. a model table and a cost table at once --------------------------------------------------------------------------------------
U_STD = 1e-2


def test_model_table_with_a_cost_table_and_set_table_on_each():
    """Two rings and two side records in one kernel: the LTV model (a table per trajectory, 16 words) under the tracking cost (a
    shared table, 8 words), every candidate against numpy; then set_table on the model alone and on the cost alone -- each
    reaches the device, neither disturbs the other -- and once more with a replayed winner."""
    N, B, L = 12, 5, 20
    rng = np.random.default_rng(21)
    mtab, ctab = tm.ltv_table(rng, N, B), tc.make_table(rng, N, 4, None, terminal=5.0)
    q = iSLS(4, 2, N, batch=B)
    mdl = models.Custom(4, 2, [0.0], tm.LTV, table=mtab)
    cst = costs.Custom(4, 2, [U_STD], tc.tracking_source(4, 2), table=ctab)
    q.forward_model, q.cost_function = mdl, cst
    u = 0.1 * rng.standard_normal((B, N, 2))
    x = np.zeros((B, N, 4))
    x[:, 0] = rng.standard_normal((B, 4))
    for t in range(N - 1):
        x[:, t + 1] = tm.ltv_step(x[:, t], u[:, t], mtab[:, t])
    q.nominal_values = (x, u)
    e = q.engine
    e.K.copy_(e._t(0.05 * rng.standard_normal((B, N, 2, 4))))
    e.k.copy_(e._t(0.1 * rng.standard_normal((B, N, 2))))
    cost = lambda c: (lambda xs, us: tc.tracking_numpy(xs, us, c, U_STD)[0])      # noqa: E731
    assert rel(q.cost, cost(ctab)(x, u)) <= 1e-10
    _search_against_numpy(e, tm.ltv_step, mtab, L, cost(ctab), 1e-10, what="both tables")
    ptr = e.model_par.data_ptr(), e.cost_tab.data_ptr()
    mtab2 = tm.ltv_table(rng, N, B)
    mdl.set_table(mtab2)
    q.cost                                                           # any entry point looks for new tables; this one runs nothing else
    assert np.array_equal(e.model_table.cpu().numpy(), mtab2) and np.array_equal(e.cost_tab.cpu().numpy(), ctab)
    _search_against_numpy(e, tm.ltv_step, mtab2, L, cost(ctab), 1e-10, what="both tables, the model's replaced")
    ctab2 = tc.make_table(rng, N, 4, None, terminal=2.0)
    cst.set_table(ctab2)
    assert rel(q.cost, cost(ctab2)(x, u)) <= 1e-10
    assert np.array_equal(e.model_table.cpu().numpy(), mtab2) and np.array_equal(e.cost_tab.cpu().numpy(), ctab2)
    _search_against_numpy(e, tm.ltv_step, mtab2, L, cost(ctab2), 1e-10, miss=True, what="both tables, the cost's replaced")
    assert ptr == (e.model_par.data_ptr(), e.cost_tab.data_ptr())   # copied INTO the buffers the engine holds


# ---- 5. the class surface against the host route -----------------------------------------------------------------------------------
def _problem(B, N, tab, seed=2, host=False):
    """The LTV model under a quadratic cost from a nominal rolled out with numpy.  host: the same model as numpy callables, the
    route the line search takes through the host (isls/hostpath.py) -- it steps every candidate once per step, in order, so a
    counter tells the callable its step; the table must be shared by the batch."""
    rng = np.random.default_rng(seed)
    q = iSLS(4, 2, N, batch=B)
    mdl = None
    if host:
        calls = [0]

        def f(x, u):
            t = calls[0] % N
            calls[0] += 1
            return tm.ltv_step(x, u, tab[t])
        q.forward_model = f
    else:
        mdl = models.Custom(4, 2, [0.0], tm.LTV, table=tab)
        q.forward_model = mdl
    q.set_quadratic_cost(rng.standard_normal((1, 4)), np.eye(4)[None], np.zeros(N, dtype=np.int32), 0.1)
    x0 = rng.standard_normal((B, 4))
    u = np.zeros((B, N, 2))
    x = np.zeros((B, N, 4))
    rows = np.broadcast_to(tab, (B, N, 16))
    x[:, 0] = x0
    for t in range(N - 1):
        x[:, t + 1] = tm.ltv_step(x[:, t], u[:, t], rows[:, t])
    q.reset()
    q.nominal_values = (x, u)
    return q, (calls if host else mdl)                             # (host: the callable's call counter)


@pytest.mark.parametrize("how", ["solve", "ilqr_admm"])
def test_class_surface_equals_the_host_route(how):
    """solve (3 iterations) and ilqr_admm (2 outer x 3 ADMM, a box on u) with the table model against the same problem with
    forward_model and get_AB as numpy callables: x_nom, u_nom and the cost log."""
    N, B = 20, 3
    tab = tm.ltv_table(np.random.default_rng(0), N)
    d, _ = _problem(B, N, tab)
    h, calls = _problem(B, N, tab, host=True)
    get_AB = lambda x, u: tm.ltv_AB(tab)                            # noqa: E731
    if how == "solve":
        d.solve(max_iter=3, max_line_search_iter=20)
        h.solve(get_AB, max_iter=3, max_line_search_iter=20)
    else:
        kw = dict(project_u=Box(-0.3, 0.3), rho_u=1.0, max_iter=2, max_admm_iter=3, max_line_search_iter=20, tol=0.0)
        d.ilqr_admm(**kw)
        h.ilqr_admm(get_AB, **kw)
    # the counter is the callable's clock: it holds only while the host route steps all candidates once per step and calls the
    # model for nothing else -- whole horizons, and at least one line search per iteration, or the comparison means nothing
    assert calls[0] % N == 0 and calls[0] >= 2 * N, calls
    cd, ch = np.array(d.cost_log, dtype=np.float64), np.array(h.cost_log, dtype=np.float64)
    assert cd.shape == ch.shape and cd.shape[0] >= 3
    errs = rel(d.x_nom, h.x_nom), rel(d.u_nom, h.u_nom), rel(cd, ch)
    print(f"{how}: x_nom {errs[0]:.2e} u_nom {errs[1]:.2e} cost log {errs[2]:.2e}; costs {cd[0].tolist()} -> {cd[-1].tolist()}")
    assert max(errs) <= 1e-10
    assert (cd[-1] < cd[0]).all()


def test_set_table_between_two_solver_calls():
    N, B = 20, 3
    rng = np.random.default_rng(0)
    tab = tm.ltv_table(rng, N)
    q, mdl = _problem(B, N, tab)
    q.solve(max_iter=3)
    ptr = q.engine.model_par.data_ptr()
    new = tm.ltv_table(rng, N)
    mdl.set_table(new)
    q.ilqr_admm(max_iter=2, max_admm_iter=3, project_u=Box(-1.0, 1.0), rho_u=1.0)
    assert q.engine.model_par.data_ptr() == ptr
    assert np.array_equal(q.engine.model_table.cpu().numpy(), new)
    x, u = q.x_nom, q.u_nom                                         # the new nominal is the model's own rollout with the new rows
    for t in range(N - 1):
        assert rel(x[:, t + 1], tm.ltv_step(x[:, t], u[:, t], new[t])) <= 1e-10


# ---- 6. mpc --------------------------------------------------------------------------------------------------------------------
J, LS = 3, 20


def _hand_loop(q, world, T):
    """The loop of iSLS.mpc driven from the host on the same kernels in the same order: ilqr_admm(max_iter=1), the window copied
    into the model's buffer, Kernels.mpc_step with the plant's buffer [par | world row s], Engine.nominal_rewritten."""
    e = q.engine
    B, N = e.B, e.N
    W = e.model_tab_w
    MP = e.model_par.shape[-1] - N * W
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=e.dtype, device=e.device)   # noqa: E731
    xl, ul, cl = np.zeros((B, T + 1, e.n)), np.zeros((B, T, e.m)), np.zeros((B, T))
    il = np.zeros((B, T), dtype=np.int32)
    for s in range(T):
        q.ilqr_admm(max_iter=1, max_admm_iter=J, max_line_search_iter=LS, tol=1e-3, project_u=Box(-1.0, 1.0), rho_u=1.0)
        cl[:, s], il[:, s] = e.cost.cpu().numpy(), e.admm_iters.cpu().numpy()
        plant = torch.cat([e.model_par[:, :MP], dev(world[:, s])], dim=-1).contiguous()
        e.model_table.copy_(dev(world[:, s + 1:s + 1 + N]))
        xm, ua, xn = (torch.zeros(B, d, dtype=e.dtype, device=e.device) for d in (e.n, e.m, e.n))
        e.kern.mpc_step(e.model, e.model_par, e.xhat, e.uhat, K=e.K, plant_par=plant, step=s, x_meas_out=xm, u_out=ua, x_next_out=xn,
                        stream=torch.cuda.current_stream().cuda_stream)
        e.nominal_rewritten()
        xl[:, s], ul[:, s], xl[:, s + 1] = xm.cpu().numpy(), ua.cpu().numpy(), xn.cpu().numpy()
    return xl, ul, cl, il


@pytest.mark.parametrize("future", [False, True], ids=["held", "future"])
def test_mpc_equals_the_hand_driven_loop_and_the_plant_table_is_the_truth(future):
    N, B, T = 8, 5, 5
    rng = np.random.default_rng(4)
    tab = tm.ltv_table(rng, N, B)
    fut = tm.ltv_table(rng, T, B) if future else None
    world = np.concatenate([tab, fut if future else np.repeat(tab[:, -1:], T, axis=1)], axis=1)
    kw = dict(project_u=Box(-1.0, 1.0), rho_u=1.0, max_admm_iter=J, max_line_search_iter=LS, tol=1e-3, model_table_future=fut)
    q, mdl = _problem(B, N, tab)
    r = q.mpc(T, **kw)
    assert np.array_equal(mdl.table, world[:, T:T + N])             # the object's table is the last window
    assert np.array_equal(q.engine.model_table.cpu().numpy(), world[:, T:T + N])
    # bit for bit the hand-driven loop: the solver and the re-roll of step s read world rows s .. and s + 1 .., the plant row s
    q2, _ = _problem(B, N, tab)
    xl, ul, cl, il = _hand_loop(q2, world, T)
    print(f"mpc future={future}: max |dx| {np.max(np.abs(r.x - xl)):.2e} |du| {np.max(np.abs(r.u - ul)):.2e} "
          f"|dcost| {np.max(np.abs(r.cost - cl)):.2e} admm iters {r.admm_iters.tolist()}")
    assert np.array_equal(r.admm_iters, il)
    assert np.array_equal(r.x, xl) and np.array_equal(r.u, ul) and np.array_equal(r.cost, cl)
    assert np.array_equal(q.x_nom, q2.x_nom) and np.array_equal(q.u_nom, q2.u_nom) and np.array_equal(q.K, q2.K)
    # the plant stepped with world row s
    for s in range(T):
        assert rel(r.x[:, s + 1], tm.ltv_step(r.x[:, s], r.u[:, s], world[:, s])) <= 1e-10
    # a truth that differs from the forecast in row 2: the measured states part ways exactly from step 3 on
    truth = world[:, :T].copy()
    truth[:, 2] += 0.05
    q3, _ = _problem(B, N, tab)
    r3 = q3.mpc(T, plant_table=truth, **kw)
    assert np.array_equal(r3.x[:, :3], r.x[:, :3]) and np.array_equal(r3.u[:, :3], r.u[:, :3])
    assert (np.abs(r3.x[:, 3] - r.x[:, 3]).max(axis=1) > 0).all()
    for s in range(T):
        assert rel(r3.x[:, s + 1], tm.ltv_step(r3.x[:, s], r3.u[:, s], truth[:, s])) <= 1e-10


def test_mpc_refuses_futures_per_trajectory_for_a_shared_table():
    N, B, T = 8, 3, 2
    rng = np.random.default_rng(5)
    q, _ = _problem(B, N, tm.ltv_table(rng, N))
    with pytest.raises(ValueError, match="shared by the batch"):
        q.mpc(T, model_table_future=tm.ltv_table(rng, T, B))
    # per-trajectory parameters with a shared table: the engine's window is per trajectory, the object's table is not
    q2 = iSLS(4, 2, N, batch=B)
    q2.forward_model = models.Custom(4, 2, np.zeros((B, 1)), tm.LTV, table=tm.ltv_table(rng, N))
    q2.set_quadratic_cost(np.zeros((1, 4)), np.eye(4)[None], np.zeros(N, dtype=np.int32), 0.1)
    q2.nominal_values = (np.zeros((B, N, 4)), np.zeros((B, N, 2)))
    with pytest.raises(ValueError, match="shared by the batch"):
        q2.mpc(T, model_table_future=tm.ltv_table(rng, T, B))


# ---- 7. sample_nominal -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feedback", [None, True], ids=["open_loop", "closed_loop"])
def test_sample_nominal_costs_of_every_sample_against_numpy(feedback):
    N, B, S, sigma, seed = 5, 2, 64, 0.1, 3
    rng = np.random.default_rng(9)
    tab = tm.ltv_table(rng, N, B)
    q, _ = _problem(B, N, tab)
    u = 0.2 * rng.standard_normal((B, N, 2))
    x = np.zeros((B, N, 4))
    x[:, 0] = q.x_nom[:, 0]
    for t in range(N - 1):
        x[:, t + 1] = tm.ltv_step(x[:, t], u[:, t], tab[:, t])
    q.nominal_values = (x, u)
    z = q.engine.ztab.cpu().numpy()[0]
    r = q.sample_nominal(samples=S, sigma=sigma, seed=seed, feedback=feedback, return_costs=True)
    eps = draws(seed, B, S, N, 2, sigma)
    K = q.K if feedback else None                                   # feedback=True leaves the gains of its backward pass in K
    xs, us = tm.sample_rollouts(tm.ltv_step, tab, x, u, eps, K=K)
    ref = ((xs - z) ** 2).sum((-1, -2)) + 0.1 * (us ** 2).sum((-1, -2))            # [B, S]
    print(f"sample_nominal feedback={feedback}: costs {rel(r.costs, ref):.2e}; |K| {0.0 if K is None else np.abs(K).max():.2e}; "
          f"spread of the reference {ref.min():.3e} .. {ref.max():.3e}")
    assert r.costs.shape == (B, S)
    assert rel(r.costs, ref) <= 1e-10
    assert feedback is None or np.abs(K).max() > 1e-3               # the closed loop is one
    assert rel(r.cost_before, ref[:, 0]) <= 1e-10 and rel(r.cost_best_sample[:, 0], ref.min(1)) <= 1e-10
    assert (r.cost_after <= r.cost_before).all()
    xn, un = q.x_nom, q.u_nom                                       # the new nominal is a rollout of the table model
    for t in range(N - 1):
        assert rel(xn[:, t + 1], tm.ltv_step(xn[:, t], un[:, t], tab[:, t])) <= 1e-10


# ---- the entry points that do not serve such a model ---------------------------------------------------------------------------------
def test_refusing_entry_points():
    N, B = 6, 2
    q, _ = _problem(B, N, tm.ltv_table(np.random.default_rng(1), N))
    K, k = np.zeros((N, 2, 4)), np.zeros((N, 2))
    with pytest.raises(capi.IslsError, match="fold the schedule"):
        q.monte_carlo(K, k, samples=4)
    with pytest.raises(capi.IslsError, match="fold the schedule"):
        q.get_trajectory_sls(np.zeros((2, 4)), np.zeros((N * 2, N * 4)), np.zeros(N * 2))
    with pytest.raises(capi.IslsError, match="fold the schedule"):
        q.isls_admm(1)
    with pytest.raises(capi.IslsError, match="fold the schedule"):
        q.iterate_once_batch()
    with pytest.raises(capi.IslsError, match="fold the schedule"):
        q.solve(method='batch', max_iter=1)
