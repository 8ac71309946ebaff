"""iSLS.gradient without a device: the numpy restatement (grad_reference.py) against central finite differences of its own rollout
cost, the gradient programs of the README's sources through hiprtc, a source outside the contract, the front end's refusals and
the register / scratch table of the sweep kernels."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

from isls import _capi as capi
from isls import costs, gradient, models

import al_reference as al
import grad_reference as gr
import table_models as tm
import user_models as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the README's tracking cost at (6, 2): par = [w_u, w_x], row = [x_ref (6) | u_ref (2)]
TRACK = r'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, const P *row, int t, int N) {
    S c = S(0);
    for (int i = 0; i < 6; ++i) c += par[1] * (x[i] - row[i]) * (x[i] - row[i]);
    for (int r = 0; r < 2; ++r) c += par[0] * (u[r] - row[6 + r]) * (u[r] - row[6 + r]);
    return c;
}'''
# the README's quadrotor in wind: QUAD with the horizontal acceleration row[0]
WINDY = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, const P *row, S *xn) {
    const P dt = par[0], mass = par[1], inertia = par[2], arm = par[3], g = par[4];
    const S f = u[0] + u[1], sn = sin(x[2]), cs = cos(x[2]);
    xn[0] = x[0] + dt * x[3]; xn[1] = x[1] + dt * x[4]; xn[2] = x[2] + dt * x[5];
    xn[3] = x[3] + dt * (-f * sn / mass + row[0]);
    xn[4] = x[4] + dt * (f * cs / mass - g);
    xn[5] = x[5] + dt * arm * (u[0] - u[1]) / inertia;
}'''
# inside the contract for S, outside it for P: the mass index comes from a parameter cast to an integer
INT_CAST = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    const int k = (int)par[0];
    xn[0] = x[0] + par[1 + (k & 1)] * x[1];
    xn[1] = x[1] + par[1] * u[0];
}'''


def quad_problem(rng, N, B=None):
    """A hovering quadrotor pushed about: J and its gradient entries are O(1) - O(100)"""
    lead = () if B is None else (B,)
    u = 4.9 + 0.5 * rng.standard_normal(lead + (N, 2))
    x0 = 0.3 * rng.standard_normal(lead + (6,))
    tab = np.concatenate([0.3 * rng.standard_normal(lead + (N, 6)), 4.9 + 0.2 * rng.standard_normal(lead + (N, 2))], axis=-1)
    return x0, u, tab


def fd(fun, v, scale=None):
    """central differences of the scalar fun at v, h = 1e-6 max(1, |v_j|)"""
    v = np.asarray(v, dtype=np.float64)
    g = np.zeros(v.size)
    for j in range(v.size):
        h = 1e-6 * max(1.0, abs(v.flat[j]))
        p, q = v.copy().reshape(-1), v.copy().reshape(-1)
        p[j] += h
        q[j] -= h
        g[j] = (fun(p.reshape(v.shape)) - fun(q.reshape(v.shape))) / (2 * h)
    return g.reshape(v.shape)


def close(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300), (np.abs(a - b).max(), np.abs(b).max())


@pytest.mark.parametrize("which", ["quad_track", "windy_al"])
def test_restatement_against_finite_differences(which):
    """grad_reference against central differences of its own rollout cost, every entry of every array: bound 1e-5 of the array's
    largest entry (rounding eps J / h and truncation both stay below 1e-6 of it at these scales)"""
    rng = np.random.default_rng(5)
    N = 6
    x0, u, ctab = quad_problem(rng, N)
    mpar = um.QUAD_PAR.copy()
    if which == "quad_track":
        f, c, cpar, mtab = gr.quad_f, gr.track_cost, np.array([0.05, 2.0]), None
    else:
        W, K = 1, 2
        lam, mu = 0.5 * rng.random((N, K)), 3.0
        f, c, cpar, mtab = gr.windy_f, gr.al_cost(W, K, lam, mu), al.PAR.copy(), 0.5 * rng.standard_normal((N, 1))
        ctab = 0.2 * rng.standard_normal((N, W))
    x = gr.rollout(f, x0, u, mpar, mtab)
    g = gr.gradient(f, c, x, u, mpar, cpar, mtab, ctab)
    J = lambda **kw: float(gr.total_cost(f, c, **{**dict(x0=x0, u=u, mpar=mpar, cpar=cpar, mtab=mtab, ctab=ctab), **kw}))   # noqa: E731
    assert abs(g["cost"] - J()) <= 1e-12 * abs(J())
    pairs = [("u", fd(lambda v: J(u=v), u)), ("x0", fd(lambda v: J(x0=v), x0)), ("model_params", fd(lambda v: J(mpar=v), mpar)),
             ("cost_params", fd(lambda v: J(cpar=v), cpar)), ("cost_table", fd(lambda v: J(ctab=v), ctab))]
    if mtab is not None:
        pairs.append(("model_table", fd(lambda v: J(mtab=v), mtab)))
        assert (g["model_table"][N - 1] == 0).all()
    for name, ref in pairs:
        ok, figs = close(g[name], ref, 1e-5)
        print(which, name, "max |restatement - fd|, max |fd|:", figs)
        assert ok, (name, figs)
    assert np.array_equal(g["x0"], g["costate"][0])


def test_gradient_programs_build_for_the_readme_sources():
    """quadrotor model, its tracking cost and the constraint cost: the gradient programs compile for fp64 and fp32, and the
    sources' own programs are what they were (the same code object before and after)"""
    quad = models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
    before = quad.code()
    for dtype in (np.float64, np.float32):
        capi.user_model_grad_build(quad.model_id, dtype)
    assert quad.code() == before
    N = 5
    track = costs.Custom(6, 2, [0.05, 2.0], TRACK, table=np.zeros((N, 8)))
    keep = costs.Custom(6, 2, al.PAR, al.full_source(6, 2, 1, 2), table=np.zeros((N, 1)), constraints=2)
    for c in (track, keep):
        before = c.code()
        capi.user_cost_grad_build(c.cost_model, np.float64)
        assert c.code() == before
    windy = models.Custom(6, 2, um.QUAD_PAR, WINDY, table=np.zeros((N, 1)))
    capi.user_model_grad_build(windy.model_id, np.float64)
    ltv = models.Custom(4, 2, [], tm.LTV, table=np.zeros((N, 16)))
    capi.user_model_grad_build(ltv.model_id, np.float64)


def test_a_source_outside_the_contract_for_P_keeps_working_and_fails_the_gradient_build():
    lib = capi.library()
    uid = ctypes.c_int32(-1)
    rc = lib.isls_user_model_create(INT_CAST.encode(), 2, 1, 3, ctypes.byref(uid))
    assert rc == capi.OK and uid.value >= capi.MODEL_USER_BASE
    assert lib.isls_user_model_grad_build(uid.value, capi.DTYPE_F64) == capi.ERR_COMPILE
    log = capi.user_model_log(uid.value)
    assert log.strip() and "contract" in log and "error" in log
    with pytest.raises(capi.IslsError, match="contract"):
        capi.user_model_grad_build(uid.value, np.float64)
    assert lib.isls_user_model_grad_build(capi.MODEL_USER_BASE + 10 ** 6, capi.DTYPE_F64) == capi.ERR_ARG
    assert lib.isls_user_cost_grad_build(0, capi.DTYPE_F64) == capi.ERR_ARG
    assert len(capi.user_model_code(uid.value)) > 0          # the model's own program is untouched


def _stub(model, cost=None, host_model=False, host_cost=False):
    return types.SimpleNamespace(_host_model=host_model, _host_cost=host_cost, _forward_model=model, _cost_function=cost,
                                 engine=types.SimpleNamespace(model=None if host_model else 0))


def test_front_end_refusals_come_before_any_launch():
    """gradient._check is all that runs ahead of the first launch: no device is touched here"""
    lti = models.LTI(np.eye(2), np.ones((2, 1)))
    quad = models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
    no_table = costs.Custom(6, 2, [0.05, 2.0, 1.0], "template <typename S, typename P>\n__device__ S stage(const S *x, const S *u, "
                            "const P *par, int t, int N) { return par[0] * u[0] * u[0] + par[1] * x[0] * x[0] + par[2] * x[1] * x[1]; }")
    with pytest.raises(capi.IslsError, match="unknown wrt"):
        gradient._check(_stub(lti), ("u", "x1"))
    with pytest.raises(capi.IslsError, match="models.Custom"):
        gradient._check(_stub(lti), ("model_params",))
    with pytest.raises(capi.IslsError, match="no table"):
        gradient._check(_stub(quad, no_table), ("cost_table",))
    with pytest.raises(capi.IslsError, match="no table"):
        gradient._check(_stub(quad, no_table), ("model_table",))
    with pytest.raises(capi.IslsError, match="costs.Custom"):
        gradient._check(_stub(quad, None), ("cost_params",))
    with pytest.raises(capi.IslsError, match="callable"):
        gradient._check(_stub(lambda x, u: x, host_model=True), ("u",))
    with pytest.raises(capi.IslsError, match="callable"):
        gradient._check(_stub(quad, lambda x, u: 0.0, host_cost=True), ("u",))
    assert gradient._check(_stub(quad, no_table), ("u", "x0", "model_params", "cost_params")) == (quad, no_table)


def test_entry_points_validate_their_arguments_without_a_device():
    lib = capi.load_hip_library()
    for sfx in ("f64", "f32"):
        fn = getattr(lib, f"isls_adjoint_sweep_{sfx}")
        fn.restype = ctypes.c_int
        assert fn(None, None) == capi.ERR_ARG
        a = capi.AdjointArgs(B=1, N=3, n=2, m=1)
        assert fn(ctypes.byref(a), None) == capi.ERR_ARG     # NULL arrays
        for noun in ("model", "cost"):
            g = getattr(lib, f"isls_user_{noun}_grad_{sfx}")
            g.restype = ctypes.c_int
            assert g(None, None) == capi.ERR_ARG
            assert g(ctypes.byref(capi.UserGradArgs(B=1, N=3, n=2, m=1, id=0)), None) == capi.ERR_ARG


def test_sweep_kernels_use_no_scratch():
    """tools/scan_kernels.py on the built library: one instantiation of adjoint_sweep_kernel per pair of families.def and dtype,
    the run-time-dimension form per dtype, none with scratch memory or spills, single-wavefront workgroups"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from scan_kernels import kernel_table
    tab = {k: v for k, v in kernel_table().items() if "adjoint_sweep" in k}
    assert len(tab) == 2 * len(capi.supported_dims()) + 2, sorted(tab)
    bad = {k: (v["scratch"], v["spill"]) for k, v in tab.items() if v["scratch"] or v["spill"]}
    assert not bad, bad
    assert all(v["wg"] == 64 for v in tab.values())
