"""User costs with a per-step table (isls.costs.Custom(..., table=)) on the CPU: they register and compile for gfx950 without a
GPU, the code object of a (cost, model) pair holds the expansion, the value and every roll-out variant of the model's built-in
family with no more scratch than the built-in ones, the table width is part of the registration, what does not fit the contract
is refused before anything is launched, the argument blocks keep their layout, and the numpy derivatives the GPU tests compare
against agree with central differences."""
import ctypes
import os
import sys

import numpy as np
import pytest

from isls import _capi as capi
from isls import costs, models

import table_costs as tc
import user_costs as uc
import user_models as um
from test_user_model_host import kernels_of, rollout_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_kernels  # noqa: E402

sys.path.pop(0)


@pytest.fixture(scope="module")
def library_table():
    return scan_kernels.kernel_table(scan_kernels.DEFAULT_LIB)


def table_cost(n, m, N=6, B=None, seed=0):
    tab = tc.make_table(np.random.default_rng(seed), N, n, B)
    return costs.Custom(n, m, [0.01], tc.tracking_source(n, m), table=tab)


def pair(which):
    """(model, n, m, template id of the model in the pair's program, built-in family to compare with)"""
    if which == "car":
        return models.CarSimple(0.1), 4, 2, capi.MODEL_CAR, capi.MODEL_CAR
    if which == "arm":
        return models.Planar3R(0.05), 9, 3, capi.MODEL_ARM3R, capi.MODEL_ARM3R
    return models.Custom(6, 2, um.QUAD_PAR, um.QUAD), 6, 2, 99, capi.MODEL_LTI


@pytest.mark.parametrize("which", ["car", "arm", "quad"])
@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_code_object_of_a_table_cost_holds_every_kernel(library_table, which, dtype, T):
    """W = 8, 8 and 12 words per step: the row's ring and side records leave the variant set and the scratch bound of
    test_code_object_holds_every_kernel as they are."""
    mdl, n, m, tid, builtin = pair(which)
    cost = table_cost(n, m)
    assert cost.cost_model >= capi.COST_USER_BASE and capi.user_cost_n_tab(cost.cost_model) == tc.width(n)
    code = cost.code(mdl, dtype)
    assert code[:4] == b"\x7fELF"
    ks = kernels_of(code)
    exp = ks[f"_ZN4isls18user_expand_kernelI{T}Li{n}ELi{m}EEEvNS_8UserExpPIT_EE"]
    assert any(k.startswith(f"_ZN4isls22user_cost_value_kernelI{T}Li{n}ELi{m}E") for k in ks)
    mine = rollout_variants(ks, T, n, m, tid)
    ref = rollout_variants(library_table, T, n, m, builtin)
    assert ref and set(mine) == set(ref), (sorted(mine), sorted(ref))
    for jo, k in mine.items():
        r = library_table[ref[jo]]
        print(which, T, jo, "scratch", ks[k][".private_segment_fixed_size"], "built-in", r["scratch"], "vgpr", ks[k].get(".vgpr_count"))
        assert ks[k][".private_segment_fixed_size"] <= r["scratch"], (k, ks[k][".private_segment_fixed_size"], r)
    assert exp[".private_segment_fixed_size"] == 0 and exp.get(".vgpr_spill_count", 0) == 0, exp


def test_the_table_width_is_part_of_the_registration():
    src = uc.fresh(tc.tracking_source(4, 2))
    plain_before = costs.Custom(4, 2, uc.COUPLED_PAR, uc.coupled_source(4, 2)).cost_model
    a = costs.Custom(4, 2, [0.01], src, table=np.ones((5, 8)))
    b = costs.Custom(4, 2, [0.01], src, table=np.ones((5, 9)))
    c = costs.Custom(4, 2, [0.01], src, table=np.ones((3, 7, 8)))      # another N, per trajectory: the same program
    assert a.cost_model != b.cost_model and a.cost_model == c.cost_model
    assert capi.user_cost_n_tab(a.cost_model) == 8 and capi.user_cost_n_tab(b.cost_model) == 9
    # a cost without a table: the id it had, the key it had, no table
    again = costs.Custom(4, 2, uc.COUPLED_PAR, uc.coupled_source(4, 2))
    assert again.cost_model == plain_before and capi.user_cost_n_tab(plain_before) == 0 and again.table is None
    assert (uc.coupled_source(4, 2), 4, 2, uc.COUPLED_PAR.size) in capi._USER_COST.ids
    lib, cid = capi.load_hip_library(), ctypes.c_int32(-1)
    assert lib.isls_user_cost_n_tab(5) == capi.ERR_ARG and lib.isls_user_cost_n_tab(1 << 20) == capi.ERR_ARG
    assert capi.USER_MAX_TAB == 16


FIVE = "template <typename S, typename P>\n__device__ S stage(const S *x, const S *u, const P *par, int t, int N) { return x[0] * u[1]; }"
SIX = ("template <typename S, typename P>\n__device__ S stage(const S *x, const S *u, const P *par, const P *row, int t, int N) "
       "{ return x[0] * row[0]; }")


def test_refusals_of_the_front_end():
    with pytest.raises(capi.IslsError, match="at most 16 words"):
        costs.Custom(4, 2, [0.1], SIX, table=np.zeros((5, 17)))
    with pytest.raises(ValueError):
        costs.Custom(4, 2, [0.1], SIX, table=np.zeros(5))
    # the five-argument form with a table, the six-argument form without: compile errors, the log in the message
    with pytest.raises(capi.IslsError, match=r"compile failed\n(.|\n)*error: no matching function for call to 'stage'"):
        costs.Custom(4, 2, [0.1], uc.fresh(FIVE), table=np.zeros((5, 2)))
    with pytest.raises(capi.IslsError, match=r"compile failed\n(.|\n)*error: no matching function for call to 'stage'"):
        costs.Custom(4, 2, [0.1], uc.fresh(SIX))
    c = costs.Custom(4, 2, [0.1], SIX, table=np.zeros((5, 2)))
    assert c.table.shape == (5, 2)
    for bad in (np.zeros((6, 2)), np.zeros((5, 3)), np.zeros((1, 5, 2))):
        with pytest.raises(ValueError, match="set_table"):
            c.set_table(bad)
    c.set_table(np.ones((5, 2)))
    assert (c.table == 1.0).all()
    with pytest.raises(ValueError, match="without a table"):
        costs.Custom(4, 2, [0.1], FIVE).set_table(np.ones((5, 2)))
    # x of another horizon, a per-trajectory table against another number of trajectories: refused before the device is touched
    with pytest.raises(ValueError, match="5 steps"):
        c(np.zeros((6, 4)), np.zeros((6, 2)))
    cb = costs.Custom(4, 2, [0.1], SIX, table=np.zeros((3, 5, 2)))
    with pytest.raises(ValueError, match=r"per-trajectory table \[3, N, W\]"):
        cb(np.zeros((2, 5, 4)), np.zeros((2, 5, 2)))


def test_refusals_of_the_library():
    """Validation comes before anything is compiled for a pair, loaded or launched, and needs no GPU: every call here is refused."""
    lib, cid = capi.load_hip_library(), ctypes.c_int32(-1)
    src = uc.fresh(SIX).encode()
    assert lib.isls_user_cost_create_tab(src, 4, 2, 1, 17, ctypes.byref(cid)) == capi.ERR_UNSUPPORTED
    assert lib.isls_user_cost_create_tab(src, 4, 2, 1, -1, ctypes.byref(cid)) == capi.ERR_UNSUPPORTED
    assert lib.isls_user_cost_create_tab(src, 4, 2, 1, 3, ctypes.byref(cid)) == capi.OK
    uid, B, N, W = cid.value, 2, 5, 3
    assert lib.isls_user_cost_n_tab(uid) == 3
    buf = np.zeros(B * N * 16)                                 # never read: every call below stops at its arguments
    p = ctypes.c_void_p(buf.ctypes.data)
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    value, value_tab = lib.isls_user_cost_value_f64, lib.isls_user_cost_value_tab_f64
    assert value(i32(uid), i32(B), i32(N), p, i64(0), p, p, p, None) == capi.ERR_ARG               # the entry without a table
    assert value_tab(i32(uid), i32(B), i32(N), p, i64(0), None, i64(0), p, p, p, None) == capi.ERR_ARG
    assert value_tab(i32(uid), i32(B), i32(N), p, i64(0), p, i64(W), p, p, p, None) == capi.ERR_ARG
    assert value_tab(i32(uid), i32(B), i32(N), p, i64(0), p, i64(N * W + 1), p, p, p, None) == capi.ERR_ARG
    for sfx in ("f64", "f32"):
        expand = getattr(lib, f"isls_user_cost_expand_{sfx}")
        rollout = getattr(lib, f"isls_rollout_ls_{sfx}")
        for ztab, sb, nvia in ((None, 0, W), (buf.ctypes.data, 0, W + 1), (buf.ctypes.data, 0, 1), (buf.ctypes.data, W, W),
                               (buf.ctypes.data, N * W - 1, W)):
            e = capi.ExpandArgs(B=B, N=N, n=4, m=2, nvia=nvia, ztab=ztab, ztab_sb=sb, c0x=buf.ctypes.data, c0u=buf.ctypes.data,
                                cost_model=uid, cost_par=buf.ctypes.data)
            assert expand(ctypes.byref(e), None, None) == capi.ERR_ARG, (sfx, ztab, sb, nvia)
            r = capi.RolloutArgs(B=B, N=N, n=4, m=2, L=8, model=capi.MODEL_CAR, nvia=nvia, ztab=ztab, ztab_sb=sb, cost_model=uid,
                                 cost_par=buf.ctypes.data)
            for k in ("model_par", "K", "k", "xhat", "uhat", "alphas", "x_out", "u_out"):
                setattr(r, k, buf.ctypes.data)
            assert rollout(ctypes.byref(r), None) == capi.ERR_ARG, (sfx, ztab, sb, nvia)


def test_argument_blocks_keep_their_layout_with_the_table():
    """The table travels in ztab / ztab_sb / nvia: sizes, the neighbours of the cost fields and the version are what
    test_argument_blocks_keep_their_layout asserts."""
    for S in (capi.RolloutArgs, capi.ExpandArgs):
        assert S.cost_par_sb.offset == S.cost_model.offset + 4 and S.cost_par.offset == S.cost_model.offset + 8
        assert S.ztab_sb.offset == S.ztab.offset + 8
    assert ctypes.sizeof(capi.RolloutArgs) == 312 and ctypes.sizeof(capi.ExpandArgs) == 208
    assert capi.load_hip_library().isls_version() == 107 == capi.ABI_VERSION


@pytest.mark.parametrize("n, m", [(4, 2), (6, 3), (9, 3)])
def test_numpy_derivatives_of_the_tracking_cost(n, m):
    """The hand-written gradient and Hessian agree with central differences of the numpy value (a table per trajectory), every row
    of every trajectory is distinct, and the terminal row is the heavy one."""
    rng = np.random.default_rng(n + m)
    B, N, h = 3, 5, 1e-5
    x, u = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
    tab = tc.make_table(rng, N, n, B)
    assert tab.shape == (B, N, tc.width(n)) and len(np.unique(tab.reshape(B * N, -1), axis=0)) == B * N
    nz = tc.nz_of(n)
    assert (tab[:, -1, nz:].min(-1) > 5 * tab[:, :-1, nz:].max((-1, -2))).all()
    _, g, H = tc.tracking_numpy(x, u, tab, 0.02)
    assert np.abs(H - np.swapaxes(H, -1, -2)).max() == 0.0
    w = np.concatenate([x, u], axis=-1)
    for k in range(n + m):
        for bb in range(B):
            for t in range(N):
                wp, wm = w.copy(), w.copy()
                wp[bb, t, k] += h
                wm[bb, t, k] -= h
                vp, gp, _ = tc.tracking_numpy(wp[..., :n], wp[..., n:], tab, 0.02)
                vm, gm, _ = tc.tracking_numpy(wm[..., :n], wm[..., n:], tab, 0.02)
                assert abs((vp[bb] - vm[bb]) / (2 * h) - g[bb, t, k]) < 1e-7 * max(1.0, abs(g[bb, t, k]))
                assert np.abs((gp[bb, t] - gm[bb, t]) / (2 * h) - H[bb, t, k]).max() < 1e-7 * max(1.0, np.abs(H[bb, t]).max())
    # the shared form and a stack of candidates against a per-trajectory table
    v1, _, _ = tc.tracking_numpy(x[0], u[0], tab[0], 0.02)
    vL, _, _ = tc.tracking_numpy(np.stack([x, x], axis=1), np.stack([u, u], axis=1), tab, 0.02)
    v, _, _ = tc.tracking_numpy(x, u, tab, 0.02)
    assert v1 == v[0] and vL.shape == (B, 2) and (vL[:, 1] == v).all()
