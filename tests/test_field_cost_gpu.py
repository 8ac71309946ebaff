"""A 2-D field for user-written costs (costs.Custom(field=), isls::field) on the GPU: value and expansion against the numpy
reference of tests/field_reference.py, the exact-quadratic field against its closed form (line search, solve_al, sampling, mpc,
gradient), and set_field in place.  fp64 at 1e-10, fp32 at 1e-4: the `rel` rule and the TOL table of test_table_cost_gpu.py."""
import numpy as np
import pytest
import torch

import field_reference as fr
from test_field_cost_host import TWO
from test_isls_api import rel
from test_table_cost_gpu import TOL, compare_searches

pytestmark = pytest.mark.gpu

# origin and spacing are powers of two, unequal per axis: (pos - origin) / spacing is exact for a position put on a sample, so the
# device and the reference pick the same cell there
ORIGIN, SPACING = (-1.0, 0.5), (0.5, 0.25)
W_STAGE = 0.7


def wavy_field(C, nx, ny, seed):
    """a non-polynomial field: sin times exp samples"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.stack([np.sin(0.9 * i + 0.4 * c + rng.uniform(0, 3)) * np.exp(0.11 * j - 0.05 * i) + 0.3 * rng.normal(size=(nx, ny))
                     for c in range(C)])


def query_points(nx, ny, n, m, B, N, seed, on_sample):
    """x [B, N, n], u [B, N, m]: field 0 is read at (x0, x1), field 1 at (x1, 0.5 x0 + u0).  Every grid coordinate is at least
    0.05 of a cell from a cell border, except the one point put exactly on a sample (on_sample).  Trajectory 0 holds the special
    points: on a sample, the last cell (i = n-2), outside on each side, outside on a corner; the others are spread over the grid
    and a cell beyond it."""
    rng = np.random.default_rng(seed)
    frac = lambda lo, hi, size: rng.integers(lo, hi, size=size) + rng.uniform(0.05, 0.95, size=size)   # noqa: E731
    px, py = frac(-1, nx, (B, N)), frac(-1, ny, (B, N))
    px[0], py[0] = [2.37, nx - 1.6, -0.7, nx - 0.4, 1.37, 2.63, nx + 1.3][:N], [1.63, ny - 1.3, 2.37, 1.63, -1.4, ny - 0.7, -2.2][:N]
    if on_sample:
        px[0, 0], py[0, 0] = 2.0, 3.0
    x, u = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
    x[..., 0], x[..., 1] = ORIGIN[0] + px * SPACING[0], ORIGIN[1] + py * SPACING[1]
    u[..., 0] = ORIGIN[1] + frac(-1, ny, (B, N)) * SPACING[1] - 0.5 * x[..., 0]       # the second argument of field 1, likewise
    return x, u


def reference(values, x, u, read=None):
    B, N, n = x.shape
    K = n + u.shape[-1]
    c, g, H = np.zeros((B, N)), np.zeros((B, N, K)), np.zeros((B, N, K, K))
    for b in range(B):
        for t in range(N):
            c[b, t], g[b, t], H[b, t] = fr.stage_reference(values, ORIGIN, SPACING, W_STAGE, x[b, t], u[b, t], read)
    return c.sum(-1), g, H


def distance_to_borders(x, u):
    """the smallest distance, in cells, of a grid coordinate the stage reads from a cell border"""
    ps = [(x[..., 0] - ORIGIN[0]) / SPACING[0], (x[..., 1] - ORIGIN[1]) / SPACING[1], (x[..., 1] - ORIGIN[0]) / SPACING[0],
          (0.5 * x[..., 0] + u[..., 0] - ORIGIN[1]) / SPACING[1]]
    return min(float(np.abs(p - np.round(p)).min()) for p in ps)


def expand_on_device(cost, x, u, dt):
    """(cost [B], gradient [B, N, n+m], Hessian [B, N, n+m, n+m]) by user_cost_expand in precision dt"""
    from isls import _capi as capi
    from isls.engine import kernels
    B, N, n = x.shape
    m, dev = u.shape[-1], torch.device("cuda")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)   # noqa: E731
    cost._push_field()
    capi.user_cost_load(cost.cost_model, -1, dt)
    z = lambda *sh: torch.zeros(*sh, dtype=dt, device=dev)   # noqa: E731
    Cxx, Cuu, Cux, c0x, c0u, val = z(B, N, n, n), z(B, N, m, m), z(B, N, m, n), z(B, N, n), z(B, N, m), z(B)
    zero = z(1, n, n)
    exp = capi.Kernels.expand_args(zero, zero[0, :1], torch.zeros(N, dtype=torch.int32, device=dev), 0.0, c0x, c0u, xhat=t(x), uhat=t(u),
                                   Cxx=Cxx, Cuu=Cuu, cost=val, cost_model=cost.cost_model, cost_par=t(cost.params()))
    kernels().user_cost_expand(exp, Cux, "f64" if dt == torch.float64 else "f32")
    torch.cuda.synchronize()
    g = torch.cat([c0x, c0u], dim=-1).double().cpu().numpy()
    H = torch.cat([torch.cat([Cxx, Cux.transpose(-1, -2)], dim=-1), torch.cat([Cux, Cuu], dim=-1)], dim=-2).double().cpu().numpy()
    return val.double().cpu().numpy(), g, H


# ---- 1, 7: value and expansion against the reference, both precisions --------------------------------------------------------------
@pytest.mark.parametrize("nx, ny, C, n, m, B", [(6, 5, 1, 4, 2, 3), (9, 8, 2, 6, 2, 67), (6, 5, 2, 6, 2, 3), (9, 8, 1, 4, 2, 67)])
def test_value_and_expansion_against_the_reference(nx, ny, C, n, m, B):
    """w field(0, x0, x1)^2 + field(1, x1, 0.5 x0 + u0) on a sin-times-exp field, N = 7: cost(x, u) and get_Cs(x, u) (fp64), and
    the expansion kernel in both precisions.  C = 1: channel 1 is clamped to channel 0 on both sides."""
    from isls import costs
    N = 7
    values = wavy_field(C, nx, ny, seed=nx + C)
    cost = costs.Custom(n, m, [W_STAGE], TWO, field=values if C > 1 else values[0], field_origin=ORIGIN, field_spacing=SPACING)
    for dt in (torch.float64, torch.float32):
        x, u = query_points(nx, ny, n, m, B, N, seed=B + n, on_sample=dt == torch.float64)
        # (x1 is also the x of read 1, half as many cells away from a border there)
        assert distance_to_borders(x[:, 1:], u[:, 1:]) >= 0.02 and (dt == torch.float64 or distance_to_borders(x, u) >= 0.02)
        if dt == torch.float32:                                # the reference at the points the device sees
            x, u = x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
            assert distance_to_borders(x, u) >= 1e-3
        want = reference(values, x, u)
        got = expand_on_device(cost, x, u, dt)
        for name, a, b in zip(("cost", "gradient", "Hessian"), got, want):
            print(f"field {nx}x{ny} C={C} ({n},{m}) B={B} {dt} {name}: {rel(a, b):.2e}")
            assert rel(a, b) < TOL[dt], name
        if dt == torch.float64:                                # the object's own surface
            cs, Cs = cost.get_Cs(x, u)
            assert rel(cost(x, u), want[0]) < 1e-10 and rel(cs, want[1]) < 1e-10 and rel(Cs, want[2]) < 1e-10
            cs0, Cs0 = cost.get_Cs(x[0], u[0])
            assert rel(cs0, want[1][0]) < 1e-10 and rel(Cs0, want[2][0]) < 1e-10


# ---- 2: the quadratic field ---------------------------------------------------------------------------------------------------------
QUADS = ((0.7, -1.3, 0.4, 0.9, -0.6, 1.1), (-0.2, 0.5, 0.8, -0.35, 0.45, 0.25))


def quad(k, x, y):
    a, b, c, d, e, g = k
    return (a + b * x + c * y + d * x * x + e * x * y + g * y * y, np.array([b + 2 * d * x + e * y, c + e * x + 2 * g * y]),
            np.array([[2 * d, e], [e, 2 * g]]))


def test_quadratic_field_has_the_analytic_hessian():
    """Two quadratics sampled on a 9 x 8 grid, points in interior cells (1 <= i <= n-3) for both reads: value, gradient and
    Hessian equal the closed form's -- a wrong f_xy or a dropped f_x d2x term shows here, apart from any interpolation error."""
    from isls import costs
    nx, ny, B, N = 9, 8, 3, 7
    X, Y = np.meshgrid(ORIGIN[0] + SPACING[0] * np.arange(nx), ORIGIN[1] + SPACING[1] * np.arange(ny), indexing="ij")
    values = np.stack([quad(k, X, Y)[0] for k in QUADS])
    rng = np.random.default_rng(5)
    x, u = rng.normal(size=(B, N, 4)), rng.normal(size=(B, N, 2))
    # x1 is a y of read 0 and an x of read 1: y cells 1 .. 5 and x cells 1 .. 6 meet in x1 in [0.75, 2.0)
    x[..., 0] = ORIGIN[0] + rng.uniform(1.05, 6.95, size=(B, N)) * SPACING[0]
    x[..., 1] = rng.uniform(0.76, 1.99, size=(B, N))
    u[..., 0] = ORIGIN[1] + rng.uniform(1.05, 5.95, size=(B, N)) * SPACING[1] - 0.5 * x[..., 0]
    cost = costs.Custom(4, 2, [W_STAGE], TWO, field=values, field_origin=ORIGIN, field_spacing=SPACING)
    want = reference(None, x, u, read=lambda c, px, py: quad(QUADS[c], px, py))
    got = expand_on_device(cost, x, u, torch.float64)
    for name, a, b in zip(("cost", "gradient", "Hessian"), got, want):
        print(f"quadratic field {name}: {rel(a, b):.2e}")
        assert rel(a, b) < 1e-10, name
    assert np.abs(want[2][..., 0, 1]).max() > 1e-3 and np.abs(want[2][..., 4, 0]).min() > 1e-3   # (the cross terms are there)


# ---- the exact-quadratic field cost and its closed-form twin ------------------------------------------------------------------------
# a 33 x 33 grid over [-4, 4]^2 (spacing 0.25: exact): its interior cells cover [-3.75, 3.5]^2, where the car of these tests stays
GRID_N, GRID_O, GRID_S = 33, (-4.0, -4.0), (0.25, 0.25)
BUMP_HEAD = r'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {
    S c = par[0] * (u[0] * u[0] + u[1] * u[1]) + par[1] * BUMP;
    if (t == N - 1) c += par[2] * ((x[0] - par[3]) * (x[0] - par[3]) + (x[1] - par[4]) * (x[1] - par[4]));
    return c;
}
'''
BUMP_FIELD = BUMP_HEAD.replace("BUMP", "isls::field(0, x[0], x[1])")
BUMP_TWIN = BUMP_HEAD.replace("BUMP", "(1.5 - 0.5 * ((x[0] - 0.5) * (x[0] - 0.5) + (x[1] + 0.25) * (x[1] + 0.25)) + 0.25 * x[0] * x[1])")
BUMP_PAR = [0.05, 0.3, 2.0, 1.5, 0.5]
DISC_STAGE = BUMP_HEAD.replace("+ par[1] * BUMP", "")
DISC_FIELD = DISC_STAGE + r'''
template <typename S, typename P>
__device__ void constraint(const S *x, const S *u, const P *par, int t, int N, S *g) { g[0] = par[1] - isls::field(0, x[0], x[1]); }
'''
DISC_TWIN = DISC_STAGE + r'''
template <typename S, typename P>
__device__ void constraint(const S *x, const S *u, const P *par, int t, int N, S *g) {
    g[0] = par[1] - ((x[0] - 0.75) * (x[0] - 0.75) + (x[1] - 0.125) * (x[1] - 0.125));
}
'''
DISC_PAR = [0.05, 0.16, 2.0, 1.5, 0.5]                       # par[1] = r^2: the constraint is on the squared distance, which the field holds exactly


def grid_xy():
    return np.meshgrid(GRID_O[0] + GRID_S[0] * np.arange(GRID_N), GRID_O[1] + GRID_S[1] * np.arange(GRID_N), indexing="ij")


def bump_values(shift=0.0):
    X, Y = grid_xy()
    return 1.5 - 0.5 * ((X - 0.5 - shift) ** 2 + (Y + 0.25) ** 2) + 0.25 * X * Y


# the disc's map: 33 x 33 over [-8, 8]^2 (spacing 0.5), so that thirty steps of the car stay in interior cells, |x|, |y| < 7
DISC_O, DISC_S = (-8.0, -8.0), (0.5, 0.5)


def disc_values():
    X, Y = np.meshgrid(DISC_O[0] + DISC_S[0] * np.arange(GRID_N), DISC_O[1] + DISC_S[1] * np.arange(GRID_N), indexing="ij")
    return (X - 0.75) ** 2 + (Y - 0.125) ** 2


def bump_cost(twin, values=None):
    from isls import costs
    if twin:
        return costs.Custom(4, 2, BUMP_PAR, BUMP_TWIN)
    return costs.Custom(4, 2, BUMP_PAR, BUMP_FIELD, field=bump_values() if values is None else values, field_origin=GRID_O, field_spacing=GRID_S)


def car(cost, B, N, dtype=np.float64, seed=0):
    """an iSLS on CarSimple with `cost` and a nominal of small random controls from near the origin"""
    from isls import iSLS, models
    rng = np.random.default_rng(seed)
    mdl = models.CarSimple(0.1)
    us = 0.3 * rng.normal(size=(B, N, 2))
    xs = np.zeros((B, N, 4))
    xs[:, 0] = rng.normal(size=(B, 4)) * [0.5, 0.5, 0.3, 0.3] + [0, 0, 0, 1.0]
    for t in range(N - 1):
        xs[:, t + 1] = mdl(xs[:, t], us[:, t])
    s = iSLS(4, 2, N, batch=B, dtype=dtype)
    s.forward_model = mdl
    s.cost_function = cost
    s.nominal_values = xs, us
    return s


# ---- 3, 7: the line search ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("L", [5, 20])
@pytest.mark.parametrize("B", [3, 67])
def test_line_search_equals_the_closed_form_twin(B, L, dtype):
    """isls_rollout_ls_* with the field cost and with the same cost in closed form on the same model, nominal, gains and
    candidates, N = 7; then both through the outer driver with a control box (the fused ADMM update behind the search)."""
    from isls import Box
    from isls import _capi as capi
    tol, N = TOL[dtype], 7
    sb, sc = car(bump_cost(True), B, N, dtype, seed=B + L), car(bump_cost(False), B, N, dtype, seed=B + L)
    eb, ec = sb.engine, sc.engine
    assert rel(ec.cost.double().cpu().numpy(), eb.cost.double().cpu().numpy()) < tol
    for e in (eb, ec):
        e.K.copy_(e._t(0.2 * np.random.default_rng(N).normal(size=(B, N, 2, 4))))
        e.k.copy_(e._t(0.3 * np.random.default_rng(N + 1).normal(size=(B, N, 2))))
    flags = capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST
    ca_b, ca_c = torch.zeros(B, L, dtype=eb.dtype, device=eb.device), torch.zeros(B, L, dtype=eb.dtype, device=eb.device)
    eb.rollout(L, flags=flags, cost_all=ca_b, active=eb.outer_active)
    ec.rollout(L, flags=flags, cost_all=ca_c, active=ec.outer_active)
    torch.cuda.synchronize()
    assert float(eb.xx[..., :2].abs().max()) < 3.5             # interior cells
    compare_searches(eb, ec, ca_b, ca_c, tol, f"field plain L={L} B={B}")
    box = Box(np.array([-0.2, -0.2]), np.array([0.2, 0.2]))
    for s in (sb, sc):
        s._setup_admm(False, box, None, np.diag([1e-1, 1e-2]), 1.0)
        s._linearize(None)
        s._expand_regularised(None)
    for k in ("c0x", "c0u", "Cxx", "Cuu", "Cux"):
        assert rel(getattr(ec, k).double().cpu().numpy(), getattr(eb, k).double().cpu().numpy()) < tol, k
        getattr(ec, k).copy_(getattr(eb, k))
    outs = []
    for e in (eb, ec):
        e.build_outer(L, 3)
        e.run_outer()
        torch.cuda.synchronize()
        outs.append([t.double().cpu().numpy() for t in (e.xx, e.xu, e.cost_new, e.zu, e.lu, e.res)])
    for name, a, b in zip(("xx", "xu", "cost_new", "zu", "lu", "res"), *outs):
        print(f"field outer driver L={L} B={B} {name}: {rel(b, a):.2e}")
        assert rel(b, a) < tol, name


# ---- 4: constraint(x, u) and solve_al --------------------------------------------------------------------------------------------------
def disc_run(twin, perturb=0.0):
    from isls import Regularization, costs
    par = np.array(DISC_PAR) * (1.0 + perturb * np.random.default_rng(11).uniform(-1, 1, size=5))
    if twin:
        cost = costs.Custom(4, 2, par, DISC_TWIN, constraints=1)
    else:
        cost = costs.Custom(4, 2, par, DISC_FIELD, constraints=1, field=disc_values(), field_origin=DISC_O, field_spacing=DISC_S)
    s = car(cost, 5, 30, seed=4)
    assert np.abs(s.x_nom[..., :2]).max() < 7.0               # interior cells
    g0 = cost.constraint(s.x_nom, s.u_nom)
    # (the penalty of a keep-out region curves the wrong way: the gain pass is regularised, as in test_constraint_cost_gpu.py)
    res = s.solve_al(max_outer=4, max_iter=8, mu0=1.0, regularization=Regularization())
    torch.cuda.synchronize()
    return dict(g0=g0, viol=res.viol[:, -1].copy(), cost=res.cost.copy(), x_nom=s.x_nom.copy(), u_nom=s.u_nom.copy())


def test_constraint_and_solve_al_equal_the_closed_form_disc():
    """(4, 2) CarSimple, N = 30, B = 5: a keep-out disc as g = r^2 - field with the field sampling the squared distance on a
    33 x 33 grid, against the closed-form disc.  Held to max(1e-10, 10 x what the closed-form run itself moves when its
    parameters are perturbed by 1e-15)."""
    a, b, c = disc_run(True), disc_run(False), disc_run(True, perturb=1e-15)
    assert np.abs(a["x_nom"][..., :2]).max() < 7.0 and a["g0"].shape == (5, 30, 1)
    assert rel(b["g0"], a["g0"]) < 1e-10
    errs = {k: rel(b[k], a[k]) for k in ("viol", "cost", "x_nom", "u_nom")}
    moved = max(rel(c[k], a[k]) for k in errs)
    print("field solve_al:", {k: f"{v:.2e}" for k, v in errs.items()}, f"closed form under 1e-15: {moved:.2e}; viol", a["viol"], b["viol"])
    assert max(errs.values()) < max(1e-10, 10 * moved), (errs, moved)


# ---- 5: set_field ----------------------------------------------------------------------------------------------------------------------
def test_set_field_equals_a_fresh_object():
    from isls import _capi as capi
    first_values, second_values = bump_values(), bump_values(shift=0.75)
    cost = bump_cost(False, first_values)
    s = car(cost, 5, 12, seed=9)
    x0, u0 = s.x_nom.copy(), s.u_nom.copy()

    def solve(q):
        q.reset()
        q.nominal_values = x0, u0
        q.solve(max_iter=2, max_line_search_iter=15)
        torch.cuda.synchronize()
        return q.x_nom.copy(), q.u_nom.copy(), np.array(q.cost, dtype=np.float64).copy()

    first = solve(s)
    ptrs = [capi.user_cost_field_ptr(cost.cost_model, dt) for dt in (np.float64, np.float32)]
    log_len = len(capi.user_cost_log(cost.cost_model))
    assert all(ptrs)
    cost.set_field(second_values)
    assert (cost.field == second_values).all()
    second = solve(s)
    assert [capi.user_cost_field_ptr(cost.cost_model, dt) for dt in (np.float64, np.float32)] == ptrs    # in place
    assert len(capi.user_cost_log(cost.cost_model)) == log_len                                         # nothing compiled
    fresh = solve(car(bump_cost(False, second_values), 5, 12, seed=9))
    assert np.abs(second[0] - first[0]).max() > 1e-3           # the new field changed the solution ...
    for a, b in zip(second, fresh):                            # ... into the fresh object's, bit for bit
        assert np.array_equal(a, b)
    cost.set_field(first_values)
    c_back = np.array(s.cost, dtype=np.float64)                # a changed field without a new nominal: the cost is evaluated again
    assert rel(c_back, bump_cost(True)(s.x_nom, s.u_nom)) < 1e-10
    for a, b in zip(solve(s), first):
        assert np.array_equal(a, b)
    assert [capi.user_cost_field_ptr(cost.cost_model, dt) for dt in (np.float64, np.float32)] == ptrs
    # release_field frees the device copies; the object goes on working from its host copy
    cost.release_field()
    assert capi.user_cost_field_ptr(cost.cost_model) is None
    for a, b in zip(solve(s), first):
        assert np.array_equal(a, b)
    assert capi.user_cost_field_ptr(cost.cost_model) is not None


def test_nan_position_gives_nan():
    """A NaN position reads inside the buffers and stays NaN, value and derivatives; the trajectories next to it are untouched"""
    from isls import costs
    values = wavy_field(2, 6, 5, seed=1)
    cost = costs.Custom(4, 2, [W_STAGE], TWO, field=values, field_origin=ORIGIN, field_spacing=SPACING)
    x, u = query_points(6, 5, 4, 2, 3, 7, seed=2, on_sample=False)
    clean = expand_on_device(cost, x, u, torch.float64)
    x[1, 3, 0] = np.nan
    val, g, H = expand_on_device(cost, x, u, torch.float64)
    assert np.isnan(val[1]) and np.isnan(g[1, 3, 0]) and np.isnan(H[1, 3, 0, 0])
    for a, b in zip((val, g, H), clean):
        assert np.array_equal(a[[0, 2]], b[[0, 2]]) and np.array_equal(a[1, :3], b[1, :3]) if a.ndim > 1 else np.array_equal(a[[0, 2]], b[[0, 2]])
    assert np.isnan(cost(x, u)[1])


def test_launch_without_a_field_set_is_refused():
    """isls_user_cost_value_* of a field cost whose field was never set on the device: ISLS_ERR_ARG before anything is launched"""
    from isls import _capi as capi
    from isls.engine import kernels
    cost = bump_cost(False)
    dev = torch.device("cuda")
    capi.user_cost_load(cost.cost_model, -1, np.float64)       # (loading needs no field)
    x, u, out = torch.zeros(2, 3, 4, dtype=torch.float64, device=dev), torch.zeros(2, 3, 2, dtype=torch.float64, device=dev), torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    par = torch.as_tensor(np.array(BUMP_PAR), device=dev)
    with pytest.raises(capi.IslsError):
        kernels().user_cost_value(cost.cost_model, par, x, u, out)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and capi.user_cost_field_ptr(cost.cost_model) is None
    cost._push_field()                                         # the module was loaded first: it gets the descriptor now
    kernels().user_cost_value(cost.cost_model, par, x, u, out)
    torch.cuda.synchronize()
    assert rel(out.cpu().numpy(), bump_cost(True)(np.zeros((2, 3, 4)), np.zeros((2, 3, 2)))) < 1e-10


# ---- 6: every program of the cost received the descriptor ----------------------------------------------------------------------------
def test_sampling_mpc_and_gradient_equal_the_closed_form_twin():
    """One pass each through sample_nominal(rounds=1, samples=64), mpc(steps=3) and gradient(wrt=("u", "cost_params")) with the
    exact-quadratic field cost and with its closed-form twin: the sampling programs, the pair's and the gradient program."""
    B, N = 5, 12
    outs = []
    for twin in (True, False):
        s = car(bump_cost(twin), B, N, seed=21)
        s.sample_nominal(samples=64, rounds=1, sigma=0.2, seed=3)
        torch.cuda.synchronize()
        o = dict(sample_x=s.x_nom.copy(), sample_u=s.u_nom.copy())
        g = s.gradient(wrt=("u", "cost_params"))
        o.update(grad_cost=g.cost.copy(), grad_u=g.u.copy(), grad_par=g.cost_params.copy())
        r = s.mpc(3, iters=1, max_admm_iter=2)
        torch.cuda.synchronize()
        o.update(mpc_x=np.array(r.x), mpc_u=np.array(r.u), mpc_cost=np.array(r.cost))
        assert np.abs(o["mpc_x"][..., :2]).max() < 3.5 and np.abs(o["sample_x"][..., :2]).max() < 3.5
        outs.append(o)
    for k in outs[0]:
        print(f"field {k}: {rel(outs[1][k], outs[0][k]):.2e}")
        assert rel(outs[1][k], outs[0][k]) < 1e-10, k
    assert np.abs(outs[0]["grad_par"][:, 1]).min() > 1e-3      # (the field's weight matters)
