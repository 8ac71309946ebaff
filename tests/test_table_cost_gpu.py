"""User costs with a per-step table (isls.costs.Custom(..., table=)) on the device.

The exact comparator everywhere is the built-in via-point cost with one via point per step (n_via = N, seq = arange(N)), which
tests/table_costs.py restates as a table cost: value and expansion against it and against numpy, the line search against
ISLS_COST_VIA in every loop form of the search (tail only, first steady-state trip, longer), with a shared and a per-trajectory
table, with the fused ADMM update and with a mispredicted winner, and bit for bit against the same constants read from `params`
at the row widths that take one and two loads per lane; then the class surface (solve, ilqr_admm), set_table against a
fresh object, and __call__ / get_Cs against numpy.  Every row of every table is distinct and the last row is the heavy one, so a
step off by one, a wrong clamp at N - 1 or a wrong batch stride shows."""
import numpy as np
import pytest
import torch

from test_isls_api import rel

import table_costs as tc

pytestmark = pytest.mark.gpu

U_STD = 0.02
TOL = {np.float64: 1e-10, np.float32: 1e-4, torch.float64: 1e-10, torch.float32: 1e-4}


def custom(n, m, table):
    from isls import costs
    return costs.Custom(n, m, [U_STD], tc.tracking_source(n, m), table=table)


# ---- value and expansion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_trajectory"])
@pytest.mark.parametrize("n, m, N", [(4, 2, 5), (9, 3, 6)])
def test_value_and_expansion_against_numpy_and_the_via_point_cost(n, m, N, shared):
    """(4, 2) at N = 5: three steps per workgroup, the last one partial; (9, 3) at N = 6: 78 pairs, four steps per workgroup, the
    last one partial.  B = 3 with trajectory 1 switched off: its arrays keep their sentinel.  Non-zero Qr, Rr."""
    from isls import _capi as capi
    from isls.engine import kernels
    B = 3
    rng = np.random.default_rng(10 * n + N)
    x, u = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
    tab = tc.make_table(rng, N, n, None if shared else B)
    Qr, Rr = rng.normal(size=(1, n, n)), rng.normal(size=(1, m, m))
    cost, g, H = tc.tracking_numpy(x, u, tab, U_STD)
    H[..., :n, :n] += 2 * Qr
    H[..., n:, n:] += 2 * Rr
    ref = dict(Cxx=H[..., :n, :n], Cuu=H[..., n:, n:], Cux=H[..., n:, :n], c0x=g[..., :n], c0u=g[..., n:], cost=cost)
    zs, Qs, seq = tc.via_tables(tab, n)
    cst = custom(n, m, tab)
    kern, dev = kernels(), torch.device("cuda")
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    on = active.bool().cpu().numpy()
    for dt in (torch.float64, torch.float32):
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)   # noqa: E731
        capi.user_cost_load(cst.cost_model, -1, dt)
        shapes = dict(Cxx=(B, N, n, n), Cuu=(B, N, m, m), Cux=(B, N, m, n), c0x=(B, N, n), c0u=(B, N, m), cost=(B,))
        out = {k: torch.full(sh, 7.0, dtype=dt, device=dev) for k, sh in shapes.items()}
        via = {k: torch.full(sh, 7.0, dtype=dt, device=dev) for k, sh in shapes.items() if k != "Cux"}
        zero = torch.zeros(1, n, n, dtype=dt, device=dev)
        exp = capi.Kernels.expand_args(zero, zero[0, :1], torch.zeros(N, dtype=torch.int32, device=dev), 0.0, out["c0x"], out["c0u"],
                                       xhat=t(x), uhat=t(u), Cxx=out["Cxx"], Cuu=out["Cuu"], Qr=t(Qr), Rr=t(Rr), cost=out["cost"],
                                       active=active, cost_model=cst.cost_model, cost_par=t([U_STD]), cost_tab=t(tab))
        assert exp.nvia == tc.width(n) and exp.ztab_sb == (0 if shared else N * tc.width(n))
        kern.user_cost_expand(exp, out["Cux"], "f64" if dt == torch.float64 else "f32")
        kern.expand_quadratic(t(Qs), t(zs), torch.as_tensor(seq, device=dev), U_STD, via["c0x"], via["c0u"], xhat=t(x), uhat=t(u),
                              Cxx=via["Cxx"], Cuu=via["Cuu"], Qr=t(Qr), Rr=t(Rr), cost=via["cost"], active=active)
        val = torch.full((B,), 7.0, dtype=dt, device=dev)      # the value alone, every trajectory (no mask at this entry)
        kern.user_cost_value(cst.cost_model, t([U_STD]), t(x), t(u), val, tab=t(tab))
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
        for k, v in res.items():
            assert (v[~on] == 7.0).all(), k                    # the inactive trajectory: left untouched
        for k, r in ref.items():
            e_np = rel(res[k][on], r[on])
            e_via = rel(res[k][on], via[k].cpu().numpy().astype(np.float64)[on]) if k in via else 0.0
            print(f"table ({n},{m}) N={N} {'shared' if shared else 'per-b'} {dt} {k}: numpy {e_np:.2e} via {e_via:.2e}")
            assert e_np < TOL[dt] and e_via < TOL[dt], k
        assert float(out["Cux"][on].abs().max()) == 0.0
        assert rel(val.cpu().numpy().astype(np.float64), cost) < TOL[dt]


# ---- line search ---------------------------------------------------------------------------------------------------------------
def car_sides(B, N, shared, dtype, seed):
    """Two iSLS on CarSimple with the same nominal (random controls rolled out): the via-point cost, and its table restatement"""
    from isls import iSLS, models
    rng = np.random.default_rng(seed)
    mdl = models.CarSimple(0.1)
    tab = tc.make_table(rng, N, 4, None if shared else B)
    zs, Qs, seq = tc.via_tables(tab, 4)
    us = 0.3 * rng.normal(size=(B, N, 2))
    xs = np.zeros((B, N, 4))
    xs[:, 0] = rng.normal(size=(B, 4)) * [0.5, 0.5, 0.3, 0.5] + [0, 0, 0, 1.0]
    for t in range(N - 1):
        xs[:, t + 1] = mdl(xs[:, t], us[:, t])
    sides = []
    for table_cost in (False, True):
        s = iSLS(4, 2, N, batch=B, dtype=dtype)
        s.forward_model = mdl
        if table_cost:
            s.cost_function = custom(4, 2, tab)
        else:
            if shared:
                s.set_cost_variables(zs, Qs, seq, U_STD)
            else:                                              # a Q table per trajectory: the engine takes it, the front end's
                s.engine.set_quadratic_cost(zs, Qs, seq, U_STD)   # host-side copies do not
            s.engine.allow_shared_hessian = False              # per-trajectory Cxx / Cuu arrays, as the user cost's
        s.nominal_values = xs, us
        sides.append(s)
    return sides, rng


def compare_searches(eb, ec, ca_b, ca_c, tol, what):
    """cost_all and cost_new within tol; best by value: the candidate each side picked costs the same on the built-in's own scale;
    x_out / u_out within tol wherever the two picked the same candidate (all but near ties)"""
    cb, cc = ca_b.double().cpu().numpy(), ca_c.double().cpu().numpy()
    bb, bc = eb.best.cpu().numpy(), ec.best.cpu().numpy()
    rows = np.arange(cb.shape[0])
    e_all, e_new = rel(cc, cb), rel(ec.cost_new.double().cpu().numpy(), eb.cost_new.double().cpu().numpy())
    e_best = np.abs(cb[rows, bc] - cb[rows, bb]).max() / max(1.0, np.abs(cb).max())
    same = torch.as_tensor(bb == bc, device=eb.best.device)
    e_x, e_u = rel(ec.xx[same].double().cpu().numpy(), eb.xx[same].double().cpu().numpy()), rel(ec.xu[same].double().cpu().numpy(),
                                                                                              eb.xu[same].double().cpu().numpy())
    print(f"{what}: cost_all {e_all:.2e} cost_new {e_new:.2e} best (value) {e_best:.2e} x {e_x:.2e} u {e_u:.2e}; "
          f"{int((~same).sum())} of {len(bb)} picked another candidate; best {bb.tolist()}")
    assert e_all < tol and e_new < tol and e_best < tol and e_x < tol and e_u < tol
    assert int(same.sum()) >= (len(bb) + 1) // 2
    return same


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_trajectory"])
@pytest.mark.parametrize("L, B", [(20, 4), (8, 9)])
@pytest.mark.parametrize("N", [2, 5, 6, 12])
def test_line_search_equals_the_via_point_cost(N, L, B, shared, dtype):
    """isls_rollout_ls_* with the table cost and with ISLS_COST_VIA on the same model, nominal, gains and candidates.  N = 2: the
    tail loop alone; N = 5: the first trip of the steady-state loop (ring depth 2); N = 6, 12: more trips.  L = 20 with B = 4:
    three trajectories per wavefront, the second wavefront partial; L = 8 with B = 9: eight per wavefront.  Then the same two
    through the outer driver with a control box: the fused element-wise ADMM update behind the search."""
    from isls import Box
    from isls import _capi as capi
    tol = TOL[dtype]
    (sb, sc), rng = car_sides(B, N, shared, dtype, seed=100 * N + L)
    eb, ec = sb.engine, sc.engine
    assert ec.cost_tab.shape == ((N, 8) if shared else (B, N, 8))
    assert rel(ec.cost.double().cpu().numpy(), eb.cost.double().cpu().numpy()) < tol
    for e in (eb, ec):                                         # the same gains for both: any will do, the search is what is compared
        e.K.copy_(e._t(0.2 * np.random.default_rng(N).normal(size=(B, N, 2, 4))))
        e.k.copy_(e._t(0.3 * np.random.default_rng(N + 1).normal(size=(B, N, 2))))
    flags = capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST
    ca_b, ca_c = torch.zeros(B, L, dtype=eb.dtype, device=eb.device), torch.zeros(B, L, dtype=eb.dtype, device=eb.device)
    eb.rollout(L, flags=flags, cost_all=ca_b, active=eb.outer_active)
    ec.rollout(L, flags=flags, cost_all=ca_c, active=ec.outer_active)
    torch.cuda.synchronize()
    compare_searches(eb, ec, ca_b, ca_c, tol, f"plain N={N} L={L} B={B}")
    # the outer driver: three ADMM iterations, the fused update and the recorded winner, on the same expansion
    box = Box(np.array([-0.2, -0.2]), np.array([0.2, 0.2]))
    for s in (sb, sc):
        s._setup_admm(False, box, None, np.diag([1e-1, 1e-2]), 1.0)
        s._linearize(None)
        s._expand_regularised(None)
    for k in ("c0x", "c0u", "Cxx", "Cuu"):
        assert rel(getattr(ec, k).double().cpu().numpy(), getattr(eb, k).double().cpu().numpy()) < tol, k
        getattr(ec, k).copy_(getattr(eb, k))
    outs = []
    for e in (eb, ec):
        e.build_outer(L, 3)
        e.run_outer()
        torch.cuda.synchronize()
        outs.append([t.double().cpu().numpy() for t in (e.xx, e.xu, e.cost_new, e.zu, e.lu, e.res)])
    for name, a, b in zip(("xx", "xu", "cost_new", "zu", "lu", "res"), *outs):
        print(f"outer driver N={N} L={L} B={B} {name}: {rel(b, a):.2e}")
        assert rel(b, a) < tol, name
    assert (eb.admm_iters == ec.admm_iters).all()


def test_line_search_with_a_mispredicted_winner():
    """`best` preset to the last candidate, which loses: every trajectory that accepts a step missed its prediction, so the whole
    wavefront replays the winner with the row staging present.  N = 12, L = 20, B = 4, a table per trajectory."""
    from isls import _capi as capi
    B, N, L = 4, 12, 20
    (sb, sc), _ = car_sides(B, N, False, np.float64, seed=77)
    eb, ec = sb.engine, sc.engine
    sb._linearize(None)
    sb._expand()
    eb.gain(active=eb.outer_active)
    eb.feedforward(active=eb.outer_active)
    for k in ("K", "k"):
        getattr(ec, k).copy_(getattr(eb, k))
    ca_b, ca_c = torch.zeros(B, L, dtype=eb.dtype, device=eb.device), torch.zeros(B, L, dtype=eb.dtype, device=eb.device)
    flags = capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST
    for e, ca in ((eb, ca_b), (ec, ca_c)):
        e.best.fill_(L - 1)
        e.rollout(L, flags=flags, cost_all=ca, active=e.outer_active)
    torch.cuda.synchronize()
    same = compare_searches(eb, ec, ca_b, ca_c, 1e-10, "mispredicted winner")
    missed = same & (ec.best != L - 1) & ((ec.status & capi.ST_LS_REJECT) == 0)
    assert int(missed.sum()) >= 1
    assert not torch.equal(ec.xx[missed], ec.xhat[missed])     # the winner, not the nominal handed back


@pytest.mark.parametrize("n, m, W, MW", [(4, 2, 1, 0), (4, 2, 9, 0), (4, 2, 16, 0), (9, 3, 1, 0), (9, 3, 9, 0), (9, 3, 16, 0), (4, 2, 9, 16)])
def test_line_search_bitwise_against_the_params_form(n, m, W, MW):
    """A cost whose W constants come from a table that repeats them in every row against the same cost reading them from `params`:
    the same arithmetic, so the line search gives the same bits, fp64 -- the same words reach `stage`, nothing more: every row
    is the same, so which step or trajectory a row belongs to is what the comparisons above see, not this one.  W = 9 and 16 take
    two loads per lane in an 8-lane slot (L = 1), W = 9 leaves the second one partly past the row's end; N = 2: the tail loop
    alone, N = 5: the first steady-state trip; B = 5: a partial last wavefront at L = 20.  MW = 16: a table model of that width
    under the table cost, against both in `params` -- side records of unequal widths holding different constants.  A case's time
    is its two run-time compiles (one program per form; about 15 s at (9, 3))."""
    import table_models as tm
    from isls import costs, models
    from isls.engine import Engine
    B, c, mc = 5, tc.generic_consts(W), tm.generic_consts(MW)
    for N in (2, 5):
        sides = []
        for table in (False, True):
            rows = (lambda v: np.tile(v, (N, 1))) if table else (lambda v: None)
            cst = costs.Custom(n, m, [0.0] if table else c, tc.generic_source(n, m, W, table), table=rows(c))
            if MW:
                mdl = models.Custom(n, m, [0.0] if table else mc, tm.generic_source(n, m, MW, table), table=rows(mc))
                sides.append((mdl.model_id, mdl.device_params(B, N), cst))
            else:
                mdl = models.CarSimple(0.1) if n == 4 else models.Planar3R(0.05)
                sides.append((mdl.model_id, mdl.params(), cst))
        for L in (1, 20):
            out = []
            for model_id, par, cst in sides:
                rng = np.random.default_rng(7)
                e = Engine(B, N, n, m)
                e.set_model(model_id, par)
                e.set_cost_model(cst.cost_model, cst.params(), table=cst.table)
                e.K.copy_(e._t(0.05 * rng.standard_normal((B, N, m, n))))
                e.k.copy_(e._t(0.1 * rng.standard_normal((B, N, m))))
                e.set_nominal(0.3 * rng.standard_normal((B, N, n)), 0.1 * rng.standard_normal((B, N, m)))
                ca = torch.zeros(B, L, dtype=e.dtype, device=e.device)
                e.rollout(L, cost_all=ca)
                out.append([t.cpu().numpy().copy() for t in (e.xx, e.xu, e.cost_new, e.best, ca)])
            assert np.isfinite(out[0][4]).all() and (out[0][4] > 0).all()
            for name, p, q in zip(("xx", "xu", "cost_new", "best", "cost_all"), *out):
                assert np.array_equal(p, q), (N, L, name)


# ---- class surface -------------------------------------------------------------------------------------------------------------
def class_sides(which, B=5, N=12, seed=3, perturb=0.0):
    """(via-point iSLS, table-cost iSLS, table) on the 3-D double integrator (models.LTI, (6, 3)) or on CarSimple, with a nominal
    of small random controls; perturb: relative size of a perturbation of the via-point side's inputs"""
    from isls import iSLS, models
    rng = np.random.default_rng(seed)
    if which == "lti":
        n, m, dt = 6, 3, 0.1
        A = np.eye(6)
        A[:3, 3:] = dt * np.eye(3)
        Bm = np.vstack([0.5 * dt * dt * np.eye(3), dt * np.eye(3)])
        mdl = models.LTI(A, Bm)
    else:
        n, m = 4, 2
        mdl = models.CarSimple(0.1)
    tab = tc.make_table(rng, N, n, B, terminal=5.0, shared_weights=True)   # per-trajectory references, one weight table
    us = 0.1 * rng.normal(size=(B, N, m))
    xs = np.zeros((B, N, n))
    xs[:, 0] = 0.3 * rng.normal(size=(B, n)) + (np.array([0, 0, 0, 1.0]) if which == "car" else 0.0)
    for t in range(N - 1):
        xs[:, t + 1] = mdl(xs[:, t], us[:, t])
    sides = []
    for table_cost in (False, True):
        s = iSLS(n, m, N, batch=B)
        s.forward_model = mdl
        if table_cost:
            s.cost_function = custom(n, m, tab)
        else:
            p = 1.0 + perturb * np.random.default_rng(seed + 1).uniform(-1, 1, size=tab.shape)
            p[..., tab.shape[-1] // 2:] = p[:1, :, tab.shape[-1] // 2:]      # (one weight table for the batch, as unperturbed)
            s.set_cost_variables(*tc.via_tables(tab * p, n), U_STD)
        s.nominal_values = xs, us
        sides.append(s)
    return sides[0], sides[1], tab


def run_class(s, how):
    from isls import Box
    if how == "solve":
        s.solve(max_iter=2, max_line_search_iter=15)
    else:
        s.ilqr_admm(project_u=Box(np.array([-0.3] * s.u_dim), np.array([0.3] * s.u_dim)), max_iter=2, max_admm_iter=3,
                    max_line_search_iter=15, rho_u=np.eye(s.u_dim) * 0.1)
    torch.cuda.synchronize()
    return dict(x_nom=s.x_nom.copy(), u_nom=s.u_nom.copy(), cost_log=np.array(s.cost_log, dtype=np.float64), status=s.status.copy())


@pytest.mark.parametrize("how", ["solve", "ilqr_admm"])
@pytest.mark.parametrize("which", ["lti", "car"])
def test_class_surface_equals_set_cost_variables(which, how):
    """Two outer iterations of solve, and of ilqr_admm(project_u=Box, max_admm_iter=3), B = 5, N = 12: the table cost against
    set_cost_variables on the same via points.  The fp64 rule (1e-10) first; a case beyond it is held to max(1e-10, 10 x what the
    built-in run itself moves when its tables are perturbed by 1e-15).
    Observed on MI355X: every case is inside the fp64 rule -- x_nom, u_nom and the cost logs differ by 8e-16 at most (lti / solve;
    the other three cases give the same x_nom and u_nom bit for bit), and the built-in run itself moves 3e-15 at most under the
    perturbation.  `status` is equal wherever it is decided by more than rounding: the second `solve` iteration of the linear-
    quadratic problem improves on the first by nothing, so its acceptance bit is set by the last bit of two equal costs (the
    built-in run flips it under the 1e-15 perturbation as well) and is left out there."""
    sv, st, _ = class_sides(which)
    a, b = run_class(sv, how), run_class(st, how)
    sp, _, _ = class_sides(which, perturb=1e-15)
    c = run_class(sp, how)                                     # the built-in run again, its tables perturbed by 1e-15
    errs = {k: rel(b[k], a[k]) for k in ("x_nom", "u_nom", "cost_log")}
    moved = max(rel(c[k], a[k]) for k in errs)
    # a status bit the built-in run itself flips under that perturbation is rounding (the second iteration of the LQ problem
    # improves on the first by nothing: its acceptance test is decided in the last bit); every other one is compared
    stable = a["status"] == c["status"]
    if which == "lti" and how == "solve":                      # at the optimum after one iteration: the last step changed nothing
        log = a["cost_log"]
        stable &= np.abs(log[-1] - log[-2]) > 1e-12 * np.maximum(1.0, np.abs(log[-1]))
    print(f"class surface {which} {how}:", {k: f"{v:.2e}" for k, v in errs.items()}, f"built-in under 1e-15: {moved:.2e};",
          "status", a["status"].tolist(), b["status"].tolist(), "stable", stable.tolist())
    assert (a["status"] == b["status"])[stable].all() and a["cost_log"].shape == b["cost_log"].shape
    bound = 1e-10 if max(errs.values()) < 1e-10 else max(1e-10, 10 * moved)
    assert max(errs.values()) < bound, (errs, bound)


def test_set_table_equals_a_fresh_object():
    """After a solve the reference is shifted with set_table and the same object solves again from the first nominal: bit for bit
    what a fresh iSLS built on the new table gives, with nothing compiled and the device table where it was."""
    from isls import _capi as capi
    sv, st, tab = class_sides("car", seed=9)
    x0, u0 = st.x_nom.copy(), st.u_nom.copy()
    cost = st._cost_function
    st.solve(max_iter=2, max_line_search_iter=15)
    first = st.x_nom.copy()
    ptr, log_len, programs = st.engine.cost_tab.data_ptr(), len(capi.user_cost_log(cost.cost_model)), len(capi._USER_COST.ids)
    new = tab.copy()
    new[..., :4] += 0.25                                       # the reference moves, the weights stay
    cost.set_table(new)
    assert (cost.table == new).all()
    st.reset()
    st.nominal_values = x0, u0
    st.solve(max_iter=2, max_line_search_iter=15)
    torch.cuda.synchronize()
    assert st.engine.cost_tab.data_ptr() == ptr and torch.equal(st.engine.cost_tab.cpu(), torch.as_tensor(new))
    assert len(capi.user_cost_log(cost.cost_model)) == log_len and len(capi._USER_COST.ids) == programs
    from isls import iSLS
    fresh = iSLS(4, 2, st.N, batch=st.batch)
    fresh.forward_model = st.forward_model
    fresh.cost_function = custom(4, 2, new)
    assert fresh._cost_function.cost_model == cost.cost_model
    fresh.nominal_values = x0, u0
    fresh.solve(max_iter=2, max_line_search_iter=15)
    torch.cuda.synchronize()
    assert np.abs(st.x_nom - first).max() > 1e-3               # the new reference changed the solution ...
    for k in ("x_nom", "u_nom", "cost"):                       # ... into the fresh object's, bit for bit
        assert np.array_equal(getattr(st, k), getattr(fresh, k)), k
    assert np.array_equal(np.array(st.cost_log), np.array(fresh.cost_log))
    # a changed table without a new nominal: the next call still sees it (the nominal's cost is evaluated again)
    cost.set_table(tab)
    c_back = st.cost
    want, _, _ = tc.tracking_numpy(st.x_nom, st.u_nom, tab, U_STD)
    assert rel(c_back, want) < 1e-10 and st.engine.cost_tab.data_ptr() == ptr


def test_call_and_get_Cs_with_a_table():
    rng = np.random.default_rng(4)
    B, N, n, m = 3, 7, 4, 2
    x, u = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
    for tab in (tc.make_table(rng, N, n), tc.make_table(rng, N, n, B)):
        cst = custom(n, m, tab)
        val, g, H = tc.tracking_numpy(x, u, tab, U_STD)
        c = cst(x, u)
        cs, Cs = cst.get_Cs(x, u)
        print("table __call__ / get_Cs", tab.shape, rel(c, val), rel(cs, g), rel(Cs, H))
        assert c.shape == (B,) and rel(c, val) < 1e-10 and rel(cs, g) < 1e-10 and rel(Cs, H) < 1e-10
        if tab.ndim == 2:                                      # one trajectory, the reference's shapes
            c1, (cs1, Cs1) = cst(x[1], u[1]), cst.get_Cs(x[1], u[1])
            assert rel(c1, val[1]) < 1e-10 and cs1.shape == (N, n + m) and rel(cs1, g[1]) < 1e-10 and rel(Cs1, H[1]) < 1e-10
        cst.set_table(2.0 * tab)                               # the host copy is what these evaluate with
        val2, _, _ = tc.tracking_numpy(x, u, 2.0 * tab, U_STD)
        assert rel(cst(x, u), val2) < 1e-10
        cst.set_table(tab)
