"""CPU-side checks of the moving constraint sets (per-row set parameters: ConvexSets par_rows / b_rows, ISLS_SET_ROW_PAR /
ISLS_SET_ROW_B of include/isls_hip.h): the numpy host route of ConvexSets against outputs of the reference's own functions with
closures over per-row parameters (tests/golden/g15_moving_sets.npz, written by tests/golden/make_moving_sets.py), at 1e-10 as the
reference comparisons of tests/test_projections.py; the window bookkeeping (row0, advance, total_rows); constant tables against
the shared form; the refusals of the library (returned before anything touches a device) and of the Python surface.
(iSLS.mpc needs a device: its padding error is checked in tests/test_moving_sets_gpu.py, the descriptor's own here.)"""
import ctypes
import importlib

import numpy as np
import pytest

from isls import _capi as capi

pj = importlib.import_module("isls.projections")               # (the package attribute of that name is the reference's dict)

TOL = 1e-10
Z = 0x1000                                                     # a pointer that is never followed: the errors come first


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - b)) / max(1.0, float(np.max(np.abs(b)))))


@pytest.fixture(scope="module")
def g(golden):
    return golden("g15_moving_sets.npz")


def shells(g, lead=0):
    c = np.concatenate([np.full((lead,) + g["a_centres"].shape[1:], 7.0), g["a_centres"]])   # `lead` rows nobody may read
    return pj.spherical_keepout(2, c, g["a_radii"], margin=float(g["a_margin"]), upper=float(g["a_upper"]))


def squares(g, lead=0):
    c = np.concatenate([np.full((lead,) + g["b_centres"].shape[1:], 7.0), g["b_centres"]])
    return pj.keepout_rectangles(4, c, g["b_sizes"], float(g["b_angle"]), margin=float(g["b_margin"]), upper=float(g["b_upper"]))


# ---- the host route is the reference's closures --------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 3], ids=["row0_0", "row0_3"])
def test_host_route_reproduces_the_reference(g, lead):
    cs = shells(g, lead)
    cs.row0 = lead
    assert cs.then.row0 == lead and cs.total_rows == 24 + lead
    y = cs(g["a_x0"].reshape(-1)).reshape(24, 2)
    assert rel(y, g["a_y"]) < TOL
    assert [cs.last_iters, cs.then.last_iters] == g["a_iters"].tolist()
    head = pj.ConvexSets(2, (0, 2), cs.sets, rho=cs.rho, max_iter=cs.max_iter, threshold=cs.threshold, row0=lead)   # first stage alone
    assert rel(head(g["a_x0"].reshape(-1)).reshape(24, 2), g["a_y_admm"]) < TOL
    sq = squares(g, lead).advance(lead)
    assert rel(sq(g["b_x0"].reshape(-1)).reshape(24, 4), g["b_y"]) < TOL and sq.last_iters == int(g["b_iters"][0])
    lo, hi = (np.concatenate([np.zeros((lead, 3)), g[k]]) for k in ("c_lo", "c_hi"))
    box = dict(kind=pj.SET_BOX, dim=3, par=np.concatenate([lo, hi], axis=1), par_rows=True)
    assert np.array_equal(pj.ConvexSets._primitive(box, np.arange(lead, lead + 24))(g["c_x0"]), g["c_y"])
    if lead:                                                    # the window matters: from row 0 the padding rows are applied
        assert rel(shells(g, lead)(g["a_x0"].reshape(-1)).reshape(24, 2), g["a_y"]) > 1e-3


def test_window_bookkeeping(g):
    cs = shells(g)
    assert cs.per_row and cs.row0 == 0 and cs.total_rows == 24
    assert cs.advance() is cs and cs.row0 == 1 and cs.then.row0 == 1
    cs.advance(4)
    assert (cs.row0, cs.then.row0) == (5, 5)
    short = cs(g["a_x0"][:19].reshape(-1))                      # 19 rows from row 5: the table's last
    assert short.shape == (38,)
    with pytest.raises(ValueError, match="rows 5 .. 25"):
        cs(g["a_x0"][:20].reshape(-1))
    with pytest.raises(ValueError):
        cs.row0 = -1
    fixed = pj.spherical_keepout(2, g["a_centres"][0], g["a_radii"])
    assert not fixed.per_row and fixed.total_rows is None and fixed.advance(2).row0 == 2
    uneven = pj.ConvexSets(2, (0, 2), cs.sets, then=shells(g, 1).then)
    with pytest.raises(ValueError, match="same number of rows"):
        uneven.total_rows
    per_problem = pj.spherical_keepout(2, np.stack([g["a_centres"], g["a_centres"] + 0.1]), g["a_radii"])
    assert per_problem.total_rows == 24 and per_problem.sets[0]["par"].shape == (2, 24, 4)
    with pytest.raises(ValueError, match="problem"):
        per_problem(g["a_x0"].reshape(-1))
    assert rel(per_problem.problem(0)(g["a_x0"].reshape(-1)).reshape(24, 2), g["a_y"]) < TOL
    with pytest.raises(ValueError, match="centres"):
        pj.spherical_keepout(2, np.zeros((2, 3)), [0.1, 0.1])


def test_constant_rows_equal_the_shared_form(g):
    rng = np.random.default_rng(0)
    x = g["a_x0"].reshape(-1)
    c0 = g["a_centres"][5]
    const = pj.spherical_keepout(2, np.broadcast_to(c0, (24, 2, 2)), g["a_radii"])
    shared = pj.spherical_keepout(2, c0, g["a_radii"])
    assert np.array_equal(const(x), shared(x)) and (const.last_iters, const.then.last_iters) == (shared.last_iters, shared.then.last_iters)
    xb, cb = g["b_x0"].reshape(-1), g["b_centres"][7]
    const = pj.keepout_rectangles(4, np.broadcast_to(cb, (24, 2, 2)), g["b_sizes"], float(g["b_angle"]))
    shared = pj.keepout_rectangles(4, cb, g["b_sizes"], float(g["b_angle"]))
    assert np.array_equal(const(xb), shared(xb)) and const.last_iters == shared.last_iters
    # every primitive with a table, and the per-row offset b
    par = {pj.SET_BOX: [-0.3, -0.2, 0.4, 0.5], pj.SET_LINEAR: [-0.1, 0.2, 0.6, -0.8], pj.SET_QUADRATIC: [0.02, 0.3],
           pj.SET_MULTILINEAR: [1, -0.1, 0.2, 0.6, -0.8]}
    y = rng.standard_normal((24, 2))
    for kind, p in par.items():
        p, b = np.array(p, dtype=np.float64), np.array([0.05, -0.02])
        one = pj.ConvexSets(2, (0, 2), [dict(kind=kind, dim=2, A=np.eye(2), b=b, par=p)], rho=2.0, max_iter=20)
        rows = pj.ConvexSets(2, (0, 2), [dict(kind=kind, dim=2, A=np.eye(2), b=np.tile(b, (24, 1)), b_rows=True, par=np.tile(p, (24, 1)),
                                              par_rows=True)], rho=2.0, max_iter=20)
        assert np.array_equal(one(y.reshape(-1)), rows(y.reshape(-1))) and one.last_iters == rows.last_iters, kind
    A, b = np.array([[1.0, 0.0], [0.0, 1.0], [0.2, 0.1]]), np.array([0.0, 0.0, 1.0])
    one = pj.ConvexSets(2, (0, 2), [dict(kind=pj.SET_SOC_UNIT, dim=3, A=A, b=b)], algorithm=pj.ALG_SOC, max_iter=30)
    rows = pj.ConvexSets(2, (0, 2), [dict(kind=pj.SET_SOC_UNIT, dim=3, A=A, b=np.tile(b, (24, 1)), b_rows=True)], algorithm=pj.ALG_SOC,
                         max_iter=30)
    assert np.array_equal(one(3 * y.reshape(-1)), rows(3 * y.reshape(-1))) and one.last_iters == rows.last_iters > 1


def test_per_row_offset_is_each_rows_own():
    """b_rows: three iterations with no stop rule in reach (threshold 0) of all rows together == of each row alone with its b"""
    rng = np.random.default_rng(1)
    y, b = rng.standard_normal((6, 2)), 0.3 * rng.standard_normal((6, 2))
    mk = lambda bb, rows: pj.ConvexSets(2, (0, 2), [dict(kind=pj.SET_BOX, dim=2, A=np.array([[1.0, 0.3], [0.0, 1.0]]), b=bb,   # noqa: E731
                                                         b_rows=rows, par=np.array([-0.2, -0.2, 0.2, 0.2]))], rho=1.5, max_iter=3, threshold=0.0)
    joint = mk(b, True)
    out = joint(y.reshape(-1)).reshape(6, 2)
    assert joint.last_iters == 3
    for r in range(6):
        alone = mk(b[r], False)
        assert rel(alone(y[r]), out[r]) < 1e-13 and alone.last_iters == 3


# ---- the library's refusals, before anything touches a device ------------------------------------------------------------------
def _call(sfx, kind, algorithm=capi.ALG_ADMM, A=Z, b=Z, par=Z, dim=2, P=0):
    lib = capi.load_hip_library()
    a = capi.ProjectArgs(P=P, R=8, d=2, nsets=1, max_iter=5, algorithm=algorithm, rho=1.0, threshold=1e-3, y_in=Z, y_out=Z)
    a.sets[0].kind, a.sets[0].dim, a.sets[0].A, a.sets[0].b, a.sets[0].par = kind, dim, A, b, par
    fn = getattr(lib, f"isls_project_rows_{sfx}")
    fn.restype = ctypes.c_int
    return fn(ctypes.byref(a), None)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_library_refusals(sfx):
    lib = capi.load_hip_library()
    assert lib.isls_version() == capi.ABI_VERSION == 107
    RP, RB = capi.SET_ROW_PAR, capi.SET_ROW_B
    assert (RP, RB) == (0x100, 0x200)
    # accepted (no problem in the block: every check runs, nothing is launched)
    for kind in (capi.SET_BOX, capi.SET_SQUARE, capi.SET_LINEAR, capi.SET_QUADRATIC, capi.SET_SHELL, capi.SET_MULTILINEAR):
        assert _call(sfx, kind | RP) == capi.OK and _call(sfx, kind | RP | RB) == capi.OK
        assert _call(sfx, kind | RP, A=None, b=None) == capi.OK                          # direct form
        assert _call(sfx, kind | RP, algorithm=capi.ALG_DYKSTRA) == capi.OK
    assert _call(sfx, capi.SET_SOC_UNIT | RB, par=None, dim=3) == capi.OK
    assert _call(sfx, capi.SET_SOC_UNIT | RB, algorithm=capi.ALG_SOC, par=None, dim=3) == capi.OK
    # refused
    assert _call(sfx, capi.SET_SOC_UNIT | RP, dim=3) == capi.ERR_ARG                     # no parameters to move
    assert _call(sfx, capi.SET_SOC_UNIT | RP | RB, algorithm=capi.ALG_SOC, dim=3) == capi.ERR_ARG
    assert _call(sfx, capi.SET_BOX | RB, A=None) == capi.ERR_ARG                         # direct form: b unused
    assert _call(sfx, capi.SET_BOX | RB, algorithm=capi.ALG_DYKSTRA) == capi.ERR_ARG     # Dykstra: b unused
    assert _call(sfx, capi.SET_BOX | RP, par=None) == capi.ERR_ARG
    assert _call(sfx, RP) == capi.ERR_UNSUPPORTED and _call(sfx, 8 | RP) == capi.ERR_UNSUPPORTED   # the flags are masked first
    assert _call(sfx, capi.SET_BOX | 0x400) == capi.ERR_UNSUPPORTED                      # a flag nobody defined
    # isls_sls_admm: its rows are not time steps
    k = capi.Kernels(lib)
    z = lambda *s: np.zeros(s, dtype=np.float64 if sfx == "f64" else np.float32)         # noqa: E731
    sets = [dict(kind=capi.SET_BOX, dim=2, A=z(2, 2), b=z(2), par=z(8, 4), par_rows=True)]
    with pytest.raises(capi.IslsError, match=rf"-> {capi.ERR_UNSUPPORTED}\b"):
        k.sls_admm(z(8, 8), z(0, 8, 2), z(8), sets, z(0, 8, 2))
    sets = [dict(kind=capi.SET_BOX, dim=2, A=z(2, 2), b=z(8, 2), b_rows=True, par=z(4))]
    with pytest.raises(capi.IslsError, match=rf"-> {capi.ERR_UNSUPPORTED}\b"):
        k.sls_admm(z(8, 8), z(0, 8, 2), z(8), sets, z(0, 8, 2))


# ---- the descriptor ------------------------------------------------------------------------------------------------------------
def test_descriptor_flags_strides_and_window():
    P, R = 3, 8
    y = np.zeros((P, R, 2))
    par, b = np.zeros((12, 4)), np.zeros((P, 12, 2))
    a = capi.Kernels.project_args(y, y, [dict(kind=capi.SET_SHELL, dim=2, A=np.eye(2), b=b, b_rows=True, par=par, par_rows=True)], row0=3)
    c = a.sets[0]
    assert c.kind == capi.SET_SHELL | capi.SET_ROW_PAR | capi.SET_ROW_B and (c.par_sp, c.b_sp, c.A_sp) == (0, 12 * 2, 0)
    assert c.par == par.ctypes.data + 3 * 4 * 8 and c.b == b.ctypes.data + 3 * 2 * 8
    nxt = capi.Kernels.project_args(y, y, [dict(kind=capi.SET_SHELL, dim=2, par=par, par_rows=True)], algorithm=capi.ALG_DYKSTRA)
    a = capi.Kernels.project_args(y, y, [dict(kind=capi.SET_SHELL, dim=2, A=np.eye(2), b=np.zeros(2), par=par, par_rows=True)], next_stage=nxt)
    assert capi.Kernels.project_args_per_row(a)
    assert capi.Kernels.project_args_set_row0(a, 4) is a                                 # ... every stage of the chain
    assert a.sets[0].par == nxt.sets[0].par == par.ctypes.data + 4 * 4 * 8 and a.sets[0].b_sp == 0
    with pytest.raises(capi.IslsError, match="pad the table"):
        capi.Kernels.project_args_set_row0(a, 5)                                         # rows 5 .. 13 of 12
    assert a.sets[0].par == par.ctypes.data + 4 * 4 * 8                                  # ... and nothing moved
    plain = capi.Kernels.project_args(y, y, [dict(kind=capi.SET_SHELL, dim=2, A=np.eye(2), b=np.zeros(2), par=np.zeros((P, 4)))])
    assert plain.sets[0].kind == capi.SET_SHELL and plain.sets[0].par_sp == 4 and not capi.Kernels.project_args_per_row(plain)
    sq = np.zeros((P, 9, 13))
    sq[..., 0] = 2
    a = capi.Kernels.project_args(y, y, [dict(kind=capi.SET_SQUARE, dim=2, A=np.eye(2), b=np.zeros(2), par=sq, par_rows=True)], row0=1)
    assert a.sets[0].par_sp == 9 * 13 and a.sets[0].par == sq.ctypes.data + 13 * 8


def test_descriptor_refusals():
    y = np.zeros((3, 8, 2))
    mk = lambda **st: capi.Kernels.project_args(y, y, [dict(dict(kind=capi.SET_SHELL, dim=2, A=np.eye(2), b=np.zeros(2)), **st)])   # noqa: E731
    with pytest.raises(ValueError, match=r"\[Rtot, 4\]"):
        mk(par=np.zeros((8, 5)), par_rows=True)                                          # the block width of a shell is 2 + dim
    with pytest.raises(ValueError, match=r"\[3, Rtot, 4\]"):
        mk(par=np.zeros((2, 8, 4)), par_rows=True)                                       # not one table per problem
    with pytest.raises(ValueError, match=r"\[Rtot, 4\]"):
        mk(par=np.zeros(4), par_rows=True)
    with pytest.raises(ValueError, match="C-contiguous"):
        mk(par=np.zeros((4, 8)).T, par_rows=True)
    with pytest.raises(capi.IslsError, match="pad the table"):
        mk(par=np.zeros((7, 4)), par_rows=True)                                          # fewer rows than the call
    with pytest.raises(ValueError, match=r"\[Rtot, 2\]"):
        mk(par=np.zeros(4), b=np.zeros((8, 3)), b_rows=True)
    with pytest.raises(ValueError, match="SET_SOC_UNIT has no parameters"):
        mk(kind=capi.SET_SOC_UNIT, dim=3, A=np.zeros((3, 2)), b=np.zeros(3), par_rows=True)
    with pytest.raises(ValueError, match="b is not used"):
        mk(A=None, par=np.zeros(4), b=np.zeros((8, 2)), b_rows=True)                     # direct form
    with pytest.raises(ValueError, match="b is not used"):
        capi.Kernels.project_args(y, y, [dict(kind=capi.SET_SHELL, dim=2, par=np.zeros(4), b=np.zeros((8, 2)), b_rows=True)],
                                  algorithm=capi.ALG_DYKSTRA)
    sq = np.zeros((8, 13))
    sq[:, 0] = 2
    sq[5, 0] = 1
    with pytest.raises(ValueError, match="same q"):
        mk(kind=capi.SET_SQUARE, par=sq, par_rows=True)
    sq[:, 0] = 2
    with pytest.raises(ValueError, match=r"\[Rtot, 13\]"):
        mk(kind=capi.SET_SQUARE, par=sq[:, :12].copy(), par_rows=True)
    with pytest.raises(ValueError, match="par_rows / b_rows"):
        mk(kind=capi.SET_SHELL | capi.SET_ROW_PAR, par=np.zeros((8, 4)))                 # the flags are the descriptor's to set


def test_sls_routes_refuse_per_row_sets(g):
    from isls import robust
    from isls.sls import SLS
    cs = pj.ConvexSets(2, (0, 2), shells(g).sets)
    with pytest.raises(ValueError, match="ilqr_admm, mpc, ADMM_LQT_DP and project_rows"):
        robust._row_projection(cs, 2)
    for kw in (dict(project_u=cs), dict(project_x=cs)):
        with pytest.raises(ValueError, match="ilqr_admm, mpc, ADMM_LQT_DP and project_rows"):
            SLS.ADMM_SLS(None, **kw)                                                     # refused before anything else is looked at
    assert robust._row_projection(pj.spherical_keepout(2, g["a_centres"][0], g["a_radii"]), 2) is not None
