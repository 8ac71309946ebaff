"""GPU tests of the moving constraint sets (per-row set parameters, ISLS_SET_ROW_PAR / ISLS_SET_ROW_B;
project_rows_moving_kernel, csrc/project.hip): direct primitives bit for bit against the per-problem form, the iterated forms against
the numpy host route of ConvexSets (which tests/test_moving_sets_host.py pins to the reference), constant tables against the
shared-operand instance, ilqr_admm on the device against its host route, and iSLS.mpc following the sets through time against a
host-driven loop.  Bounds: 1e-10 (fp64) / 1e-4 (fp32) max-abs as tests/test_hip_kernels.py uses for the same algorithms against
the oracle; 1e-12 relative for ilqr_admm as test_ilqr_admm_host_projection_path (tests/test_isls_api.py)."""
import importlib

import numpy as np
import pytest
import torch

import isls_problems as P
from isls import _capi as capi

pj = importlib.import_module("isls.projections")               # (the package attribute of that name is the reference's dict)
pytestmark = pytest.mark.gpu
TOL = {np.float64: 1e-10, np.float32: 1e-4}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(y, sets, **kw):
    """isls_project_rows on the device: numpy in (operands of the dtype of y), (output, iters) out"""
    from dual import hip_kernels
    cast = lambda v: dev(v.astype(y.dtype) if v.dtype.kind == "f" else v)   # noqa: E731
    dsets = [{k: (cast(v) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sets]
    nxt = kw.pop("next_stage", None)
    yd, od, itd = dev(y), dev(np.zeros_like(y)), dev(np.full(y.shape[0], -1, dtype=np.int32))
    if "row_mask" in kw:
        kw["row_mask"] = dev(kw["row_mask"])
    if nxt is not None:                                         # (sets, kwargs) of a second stage, in place on the output
        nsets = [{k: (cast(v) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in nxt[0]]
        kw["next_stage"] = capi.Kernels.project_args(od, od, nsets, **nxt[1])
    hip_kernels().project_rows(yd, od, dsets, iters=itd, **kw)
    torch.cuda.synchronize()
    return od.cpu().numpy(), itd.cpu().numpy()


def chain_on_device(cs, y, dtype=np.float64, **kw):
    """a ConvexSets (all stages, its window) on the rows y [P, R, dim] through Kernels.project_args_chain; the output starts as
    a copy of the rows: the library writes the coordinate block of the sets only"""
    from dual import hip_kernels
    yd, od, itd = dev(y.astype(dtype)), dev(y.astype(dtype)), dev(np.full(y.shape[0], -1, dtype=np.int32))
    wrap = lambda a: dev(a.astype(dtype) if a.dtype.kind == "f" else a)   # noqa: E731
    a = capi.Kernels.project_args_chain(yd, od, cs.stages(), wrap=wrap, iters=itd, **kw)
    hip_kernels()._call("project_rows", "f64" if dtype == np.float64 else "f32", a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return od.cpu().numpy(), itd.cpu().numpy()


@pytest.fixture(scope="module")
def g(golden):
    return golden("g15_moving_sets.npz")


# ---- 1. direct primitives: a per-row table over [P, R] == the per-problem form over [P*R, 1], bit for bit ---------------------
def _direct_tables(kind, d, n, rng):
    """n parameter blocks of a primitive acting on rows of dimension d"""
    u = lambda *s: rng.uniform(0.1, 1.0, size=s)                # noqa: E731
    if kind == capi.SET_BOX:
        lo = -u(n, d)
        return np.concatenate([lo, lo + 2 * u(n, d) * u(n, d)], axis=1)
    if kind == capi.SET_SHELL:
        l = 0.5 * u(n, 1)
        return np.concatenate([l, l + u(n, 1), rng.standard_normal((n, d))], axis=1)
    if kind == capi.SET_LINEAR:
        return np.concatenate([-u(n, 1), u(n, 1), rng.standard_normal((n, d))], axis=1)
    if kind == capi.SET_SQUARE:
        W = np.eye(d) + 0.2 * rng.standard_normal((n, d, d))
        return np.concatenate([np.full((n, 1), d), 0.5 * u(n, 1), 1.0 + u(n, 1), 0.3 * rng.standard_normal((n, d)), W.reshape(n, -1),
                               np.linalg.inv(W).reshape(n, -1)], axis=1)
    q = d - 1                                                   # SET_MULTILINEAR: q rows of M
    return np.concatenate([np.full((n, 1), q), -u(n, q), u(n, q), rng.standard_normal((n, q * d))], axis=1)


CASES = [(capi.SET_BOX, 1), (capi.SET_BOX, 2), (capi.SET_BOX, 3), (capi.SET_BOX, 4), (capi.SET_SHELL, 2), (capi.SET_SHELL, 3),
         (capi.SET_LINEAR, 2), (capi.SET_LINEAR, 3), (capi.SET_SQUARE, 2), (capi.SET_SQUARE, 3), (capi.SET_MULTILINEAR, 2),
         (capi.SET_MULTILINEAR, 3)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("R", [1, 65, 257, 513])
def test_direct_primitives_bit_for_bit(g, R, dtype):
    """R: a single row, a partial second wavefront, the 512-thread and the 1024-thread instance.  The tables have exactly R
    rows (the lanes beyond R must not read past them)."""
    rng = np.random.default_rng(R)
    Pn = 3
    for kind, d in CASES:
        y = (1.5 * rng.standard_normal((Pn, R, d))).astype(dtype)
        for per_problem in (False, True):
            tab = _direct_tables(kind, d, Pn * R if per_problem else R, rng).astype(dtype)
            tab = tab.reshape(Pn, R, -1) if per_problem else tab
            got, _ = run(y, [dict(kind=kind, dim=d, par=tab, par_rows=True)])
            flat = np.ascontiguousarray(np.broadcast_to(tab, (Pn, R, tab.shape[-1]))).reshape(Pn * R, -1)
            want, _ = run(y.reshape(Pn * R, 1, d), [dict(kind=kind, dim=d, par=flat)])       # today's per-problem operands
            assert np.array_equal(got, want.reshape(Pn, R, d)), (kind, d, per_problem)
            assert not np.array_equal(got, y)                                                # ... and something was projected
    # the fixture's per-row box: the reference's project_bound with broadcast bounds
    if R == 1 and dtype == np.float64:
        got, _ = run(g["c_x0"][None], [dict(kind=capi.SET_BOX, dim=3, par=np.concatenate([g["c_lo"], g["c_hi"]], axis=1), par_rows=True)])
        assert np.array_equal(got[0], g["c_y"])


# ---- 2. iterated forms against the host route ------------------------------------------------------------------------------
def _fixture_sets(g, which, lead=0):
    pad = lambda c: np.concatenate([np.full((lead,) + c.shape[1:], 7.0), c])   # noqa: E731
    if which == "a":
        cs = pj.spherical_keepout(2, pad(g["a_centres"]), g["a_radii"], margin=float(g["a_margin"]), upper=float(g["a_upper"]))
        return cs, g["a_x0"], g["a_y"], g["a_iters"][0]
    cs = pj.keepout_rectangles(4, pad(g["b_centres"]), g["b_sizes"], float(g["b_angle"]), margin=float(g["b_margin"]),
                               upper=float(g["b_upper"]))
    return cs, g["b_x0"], g["b_y"], g["b_iters"][0]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("lead", [0, 3], ids=["row0_0", "row0_3"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_fixture_cases_on_device(g, which, lead, dtype):
    """the two-shell chain (ADMM, then Dykstra through `next`) and the moving squares: host route == device, equal iterations
    of the first stage (the only count the library reports), and both == the reference's output; row0 = 3 on a table with
    three leading rows that nobody may read"""
    cs, x0, y_ref, it_ref = _fixture_sets(g, which, lead)
    cs.row0 = lead
    y = np.stack([x0, x0[::-1] * 0.9])                          # two problems: the fixture's rows and another order
    got, it = chain_on_device(cs, y, dtype)
    host = np.stack([cs(y[p].astype(dtype).astype(np.float64).reshape(-1)).reshape(x0.shape) for p in range(1)])
    print(f"{which} lead {lead} {dtype.__name__}: |dev - host| {np.max(np.abs(got[0] - host[0])):.2e} |dev - ref| "
          f"{np.max(np.abs(got[0] - y_ref)):.2e} iters {it.tolist()} host {cs.last_iters} ref {it_ref}")
    assert it[0] == cs.last_iters == it_ref
    assert np.max(np.abs(got[0] - host[0])) < TOL[dtype] and np.max(np.abs(got[0] - y_ref)) < TOL[dtype]
    host1 = cs(y[1].astype(dtype).astype(np.float64).reshape(-1)).reshape(x0.shape)
    assert it[1] == cs.last_iters and np.max(np.abs(got[1] - host1)) < TOL[dtype]


def _random_case(rng, Pn=3, R=65, lead=0):
    """two moving shells + a moving slab on rows of dimension 3 (the sets act on the first two coordinates), per-problem tables"""
    t = np.arange(R + lead)[:, None]
    c = np.stack([np.stack([rng.uniform(-1, 1, 2) + t * rng.uniform(-0.02, 0.02, 2) for _ in range(2)], axis=1) for _ in range(Pn)])
    shell = lambda i: np.ascontiguousarray(np.concatenate([np.broadcast_to([0.08, 50.0], (Pn, R + lead, 2)), c[:, :, i]], axis=-1))   # noqa: E731
    slab = np.ascontiguousarray(np.concatenate([np.broadcast_to([-0.5, 0.6], (Pn, R + lead, 2)) + 0.01 * t,
                                                rng.standard_normal((Pn, R + lead, 2))], axis=-1))
    sets = [dict(kind=pj.SET_SHELL, dim=2, A=np.eye(2), b=np.zeros(2), par=shell(0), par_rows=True),
            dict(kind=pj.SET_SHELL, dim=2, A=np.eye(2), b=0.02 * rng.standard_normal((R + lead, 2)), b_rows=True, par=shell(1), par_rows=True),
            dict(kind=pj.SET_LINEAR, dim=2, A=np.eye(2), b=np.zeros(2), par=slab, par_rows=True)]
    return sets, rng.uniform(-1.2, 1.2, size=(Pn, R, 3))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_random_case_mask_chain_and_window(dtype):
    """[P=3, R=65] (a partial second wavefront), per-problem tables, a per-row offset b shared by the problems, a row mask
    (masked rows pass through bit for bit), the ADMM -> Dykstra chain and row0 = 3.  Eight iterations with the threshold out
    of reach, so that the count is the same in both precisions."""
    rng = np.random.default_rng(5)
    Pn, R, lead = 3, 65, 3
    sets, y = _random_case(rng, Pn, R, lead)
    rows = np.flatnonzero(rng.uniform(size=R) < 0.7)
    dyk = pj.ConvexSets(3, (0, 2), [dict(kind=s["kind"], dim=2, par=s["par"], par_rows=True) for s in sets[:2]], max_iter=6, threshold=1e-9,
                        algorithm=pj.ALG_DYKSTRA)
    cs = pj.ConvexSets(3, (0, 2), sets, rho=2.0, max_iter=8, threshold=1e-30, rows=rows, then=dyk, row0=lead)
    assert dyk.row0 == lead
    got, it = chain_on_device(cs, y, dtype)
    yq = y.astype(dtype).astype(np.float64)
    for p in range(Pn):
        one = cs.problem(p)
        host = one(yq[p].reshape(-1)).reshape(R, 3)
        print(f"problem {p} {dtype.__name__}: |dev - host| {np.max(np.abs(got[p] - host)):.2e} iters {it[p]} host {one.last_iters}")
        assert it[p] == one.last_iters == 8                    # (the library reports the first stage's count)
        assert np.max(np.abs(got[p] - host)) < TOL[dtype]
    # the first stage alone with its mask: masked rows and the third coordinate pass through bit for bit
    head = pj.ConvexSets(3, (0, 2), sets, rho=2.0, max_iter=8, threshold=1e-30, rows=rows, row0=lead)
    got, it = chain_on_device(head, y, dtype)
    masked = np.setdiff1d(np.arange(R), rows)
    assert np.array_equal(got[:, masked], y.astype(dtype)[:, masked]) and np.array_equal(got[..., 2], y.astype(dtype)[..., 2])
    assert not np.array_equal(got[:, rows, :2], y.astype(dtype)[:, rows, :2])
    for p in range(Pn):
        assert np.max(np.abs(got[p] - head.problem(p)(yq[p].reshape(-1)).reshape(R, 3))) < TOL[dtype]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_per_row_offset_with_project_soc(dtype):
    """ISLS_SET_ROW_B under ISLS_PROJ_ALG_SOC: A y + b_r in the second-order cone with one offset per row"""
    rng = np.random.default_rng(9)
    Pn, R = 3, 65
    A = np.array([[1.0, 0.0], [0.0, 1.0], [0.2, 0.1]])
    b = np.concatenate([0.1 * rng.standard_normal((Pn, R, 2)), 0.5 + rng.uniform(size=(Pn, R, 1))], axis=-1)
    cs = pj.ConvexSets(2, (0, 2), [dict(kind=pj.SET_SOC_UNIT, dim=3, A=A, b=np.ascontiguousarray(b), b_rows=True)], algorithm=pj.ALG_SOC,
                       rho=1.0, max_iter=8, threshold=1e-30)
    y = 3.0 * rng.standard_normal((Pn, R, 2))
    got, it = chain_on_device(cs, y, dtype)
    yq = y.astype(dtype).astype(np.float64)
    for p in range(Pn):
        one = cs.problem(p)
        host = one(yq[p].reshape(-1)).reshape(R, 2)
        assert it[p] == one.last_iters == 8 and np.max(np.abs(got[p] - host)) < TOL[dtype]
    assert np.max(np.abs(got - y.astype(dtype))) > 0.1


# ---- 3. constant rows == the shared-operand instance ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("R", [65, 257, 513])
def test_constant_rows_equal_the_shared_instance(g, R, dtype):
    """the same template body on the same numbers: equal bits and equal iteration counts"""
    rng = np.random.default_rng(R)
    y = np.concatenate([rng.uniform(-0.5, 3.0, size=(3, R, 2)), rng.standard_normal((3, R, 2))], axis=-1)
    cb = g["b_centres"][7]
    for const, shared in ((pj.keepout_rectangles(4, np.broadcast_to(cb, (R, 2, 2)), g["b_sizes"], float(g["b_angle"])),
                           pj.keepout_rectangles(4, cb, g["b_sizes"], float(g["b_angle"]))),
                          (pj.spherical_keepout(4, np.broadcast_to(g["a_centres"][5], (R, 2, 2)), 3 * g["a_radii"], q=2),
                           pj.spherical_keepout(4, g["a_centres"][5], 3 * g["a_radii"], q=2))):
        a, ia = chain_on_device(const, y, dtype)
        b, ib = chain_on_device(shared, y, dtype)
        assert np.array_equal(ia, ib) and ia.min() > 1
        assert np.array_equal(a, b) and not np.array_equal(a, y.astype(dtype))


# ---- 4. ilqr_admm: the device route == the host route -----------------------------------------------------------------------
B, N, T = 3, 20, 3
X0 = np.array([[0.0, 0.0, 0.0, 0.0], [0.1, -0.1, 0.0, 0.0], [-0.1, 0.1, 0.2, 0.0]])   # outside every ball of moving_centres


def di_solver():
    import isls
    from isls import models
    A, Bm = P.double_integrator_AB(2, 2, 0.1)
    s = isls.iSLS(4, 2, N, batch=B)
    s.forward_model = models.LTI(A, Bm)
    zs, Qs, seq = P.via_point_cost(4, N, [1.0, 0.8, 0.0, 0.0], 1e2 * np.eye(4))
    s.set_cost_variables(zs, Qs, seq, 1e-1)
    us = np.zeros((B, N, 2))
    xs = np.stack([P.rollout_open_loop(P.lti_f(A, Bm), X0[b], us[b]) for b in range(B)])
    s.reset()
    s.nominal_values = xs, us
    return s


def moving_centres(rows, per_traj=False):
    """two balls that cross the straight line to the target while the plan runs: [rows, 2, 2], or [B, rows, 2, 2] with
    another start and another velocity of both balls for every trajectory"""
    t = np.arange(rows)[:, None]

    def one(b):
        return np.stack([np.array([0.35 + 0.03 * b, 0.1 - 0.02 * b]) + t * np.array([0.002 * b, 0.012 - 0.001 * b]),
                         np.array([0.8 - 0.02 * b, 0.85]) + t * np.array([-0.006, -0.01 + 0.002 * b])], axis=1)
    return np.stack([one(b) for b in range(B)]) if per_traj else one(0)


def window(c, s, rows=None):
    """rows s .. s + rows (default N) of a table of centres [Rtot, 2, 2] or [B, Rtot, 2, 2]"""
    return c[..., s:s + (N if rows is None else rows), :, :]


TABLES = pytest.mark.parametrize("per_traj", [False, True], ids=["shared_table", "table_per_trajectory"])


def keepout(centres):
    return pj.spherical_keepout(4, centres, [0.12, 0.1], q=2)


ADMM = dict(max_admm_iter=5, max_line_search_iter=20, rho_x=1e1)


@TABLES
def test_ilqr_admm_device_route_equals_host_route(per_traj):
    """x_dim = 4, u_dim = 2, N = 20, batch = 3, a moving spherical_keepout on the positions, centres shared or per trajectory;
    the host route is the same object behind a lambda.  That route projects one trajectory per call and does not say which,
    so with a table per trajectory the lambda serves cs.problem(b) of the trajectory whose initial state the argument's first
    row carries (row 0 of a plan is x0, which lies outside the balls: the projection and the multiplier leave it alone); the
    calls must then have come in the order 0, 1, .., B - 1 of every ADMM iteration (tol = 0: no trajectory stops early),
    behind the few probes by which ilqr_admm looks for a box in a callable."""
    c = moving_centres(N, per_traj)
    cs = keepout(c)
    d, h = di_solver(), di_solver()
    ld = d.ilqr_admm(project_x=cs, max_iter=3, tol=0.0, **ADMM)
    one, served = [cs.problem(b) for b in range(B)] if per_traj else [cs] * B, []

    def host(v):
        served.append(int(np.argmin(np.linalg.norm(X0[:, :2] - np.asarray(v)[:2], axis=1))))
        return one[served[-1]](v)
    lh = h.ilqr_admm(project_x=host, max_iter=3, tol=0.0, **ADMM)
    real = 3 * ADMM["max_admm_iter"] * B
    assert served[-real:] == list(range(B)) * (real // B) and len(served) - real <= 6
    rel = lambda a, b: float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))   # noqa: E731
    print(f"x_nom {rel(d.x_nom, h.x_nom):.2e} u_nom {rel(d.u_nom, h.u_nom):.2e} logs {rel(np.array(ld), np.array(lh)):.2e}")
    assert rel(d.x_nom, h.x_nom) < 1e-12 and rel(d.u_nom, h.u_nom) < 1e-12
    assert np.array(ld).shape == np.array(lh).shape == (5, B, 2) and rel(np.array(ld), np.array(lh)) < 1e-12
    still = di_solver()
    still.ilqr_admm(project_x=keepout(np.repeat(window(c, 0, 1), N, axis=-3)), max_iter=3, tol=0.0, **ADMM)   # row 0 throughout
    assert rel(d.x_nom, still.x_nom) > 1e-4                      # the sets bind, and they move
    if per_traj:                                                 # ... and every trajectory has its own
        shared = di_solver()
        shared.ilqr_admm(project_x=keepout(c[0]), max_iter=3, tol=0.0, **ADMM)
        assert np.array_equal(d.x_nom[0], shared.x_nom[0]) and rel(d.x_nom[1:], shared.x_nom[1:]) > 1e-4


# ---- 5. mpc follows the sets through time -----------------------------------------------------------------------------------
def host_loop(q, steps, sets_at):
    """the loop the parent code allows (tests/test_mpc_gpu.py), with the ConvexSets rebuilt before each ilqr_admm call"""
    e = q.engine
    xl, ul = np.zeros((B, steps + 1, e.n)), np.zeros((B, steps, e.m))
    cl, il = np.zeros((B, steps)), np.zeros((B, steps), dtype=np.int32)
    for s in range(steps):
        q.ilqr_admm(max_iter=2, tol=1e-3, project_x=sets_at(s), **ADMM)
        cl[:, s], il[:, s] = e.cost.cpu().numpy(), e.admm_iters.cpu().numpy()
        xm, ua, xn = (torch.zeros(B, d, dtype=e.dtype, device=e.device) for d in (e.n, e.m, e.n))
        e.kern.mpc_step(e.model, e.model_par, e.xhat, e.uhat, K=e.K, tab=e.cost_tab, step=s, x_meas_out=xm, u_out=ua, x_next_out=xn,
                        stream=torch.cuda.current_stream().cuda_stream)
        e.nominal_rewritten()
        xl[:, s], ul[:, s], xl[:, s + 1] = xm.cpu().numpy(), ua.cpu().numpy(), xn.cpu().numpy()
    return xl, ul, cl, il


def _same(r, ref):
    xl, ul, cl, il = ref
    print(f"max |dx| {np.max(np.abs(r.x - xl)):.2e} |du| {np.max(np.abs(r.u - ul)):.2e} |dcost| {np.max(np.abs(r.cost - cl)):.2e} "
          f"admm iters {r.admm_iters.tolist()} / {il.tolist()}")
    assert np.array_equal(r.admm_iters, il)
    assert np.array_equal(r.x, xl) and np.array_equal(r.u, ul) and np.array_equal(r.cost, cl)


@TABLES
def test_mpc_follows_world_time_sets(per_traj):
    c = moving_centres(N + 2 * T, per_traj)
    cs = keepout(c)
    q = di_solver()
    r = q.mpc(steps=T, iters=2, tol=1e-3, project_x=cs, **ADMM)
    assert cs.row0 == T and cs.then.row0 == T
    ref = host_loop(di_solver(), T, lambda s: keepout(window(c, s)))
    _same(r, ref)
    still = host_loop(di_solver(), T, lambda s: keepout(window(c, 0)))
    assert not np.array_equal(r.x, still[0])                    # the window matters
    # a second call continues from the rows consumed
    r2 = q.mpc(steps=T, iters=2, tol=1e-3, project_x=cs, **ADMM)
    assert cs.row0 == 2 * T
    q2 = di_solver()
    host_loop(q2, T, lambda s: keepout(window(c, s)))
    _same(r2, host_loop(q2, T, lambda s: keepout(window(c, T + s))))
    if per_traj:                                                 # every trajectory follows its own table
        one = host_loop(di_solver(), T, lambda s: keepout(window(c[0], s)))
        assert np.array_equal(r.x[0], one[0][0]) and not np.array_equal(r.x[1:], one[0][1:])


@TABLES
def test_mpc_keeps_horizon_relative_sets(per_traj):
    c = moving_centres(N, per_traj)
    cs = keepout(c)
    r = di_solver().mpc(steps=T, iters=2, tol=1e-3, project_x=cs, **ADMM)
    assert cs.row0 == 0
    _same(r, host_loop(di_solver(), T, lambda s: keepout(c)))


@TABLES
def test_mpc_asks_for_a_padded_table(per_traj):
    for rows in (N + 1, N + T - 1):
        cs = keepout(moving_centres(rows, per_traj))
        with pytest.raises(capi.IslsError, match="pad the table"):
            di_solver().mpc(steps=T, project_x=cs, **ADMM)
        assert cs.row0 == 0
    cs = keepout(moving_centres(N + T, per_traj)).advance(1)      # N + T - 1 rows left
    with pytest.raises(capi.IslsError, match="pad the table"):
        di_solver().mpc(steps=T, project_x=cs, **ADMM)
    with pytest.raises(capi.IslsError, match="pad the table"):    # fewer rows than the horizon: the descriptor refuses
        di_solver().ilqr_admm(project_x=keepout(moving_centres(N - 1, per_traj)), max_iter=1, **ADMM)
