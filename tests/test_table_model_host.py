"""User models with a per-step table (isls.models.Custom(..., table=)) on the CPU: they register and compile for gfx950 without a
GPU, the model's code object holds every roll-out variant of the launch plan with no more scratch than the built-in family's, the
table width is part of the registration, what does not fit the contract is refused before anything is launched, and the argument
blocks keep their layout."""
import ctypes
import os
import sys

import numpy as np
import pytest

from isls import _capi as capi
from isls import costs, models

import table_models as tm
import user_costs as uc
from test_user_model_host import kernels_of, rollout_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_kernels  # noqa: E402

sys.path.pop(0)


@pytest.fixture(scope="module")
def library_table():
    return scan_kernels.kernel_table(scan_kernels.DEFAULT_LIB)


# (n, m, W, built-in family to compare with): the widest row at every pair
PAIRS = [(4, 2, 16, capi.MODEL_CAR), (6, 3, 16, capi.MODEL_LTI), (9, 3, 16, capi.MODEL_ARM3R)]


@pytest.mark.parametrize("n, m, W, builtin", PAIRS)
@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_code_object_of_a_table_model_holds_every_kernel(library_table, n, m, W, builtin, dtype, T):
    mdl = models.Custom(n, m, [0.0], tm.generic_source(n, m, W, True), table=np.tile(tm.generic_consts(W), (5, 1)))
    assert mdl.model_id >= capi.MODEL_USER_BASE and capi.user_model_n_tab(mdl.model_id) == W
    code = mdl.code(dtype)
    assert code[:4] == b"\x7fELF"
    ks = kernels_of(code)
    assert any(k.startswith(f"_ZN4isls20user_step_tab_kernelI{T}Li{n}ELi{m}E") for k in ks)
    assert any(k.startswith(f"_ZN4isls21user_linearize_kernelI{T}Li{n}ELi{m}E") for k in ks)
    mine = rollout_variants(ks, T, n, m, 99)
    ref = rollout_variants(library_table, T, n, m, builtin)
    assert ref and set(mine) == set(ref), (sorted(mine), sorted(ref))
    for jo, k in mine.items():
        r = library_table[ref[jo]]
        print(n, m, W, T, jo, "scratch", ks[k][".private_segment_fixed_size"], "built-in", r["scratch"], "vgpr", ks[k].get(".vgpr_count"))
        assert ks[k][".private_segment_fixed_size"] <= r["scratch"], (k, ks[k][".private_segment_fixed_size"], r)


def test_the_table_width_is_part_of_the_registration():
    src = uc.fresh(tm.generic_source(4, 2, 3, True))
    a = models.Custom(4, 2, [0.1], src, table=np.ones((5, 3)))
    b = models.Custom(4, 2, [0.1], src, table=np.ones((5, 4)))
    c = models.Custom(4, 2, [0.1], src, table=np.ones((3, 7, 3)))      # another N, per trajectory: the same program
    assert a.model_id != b.model_id and a.model_id == c.model_id
    assert capi.user_model_n_tab(a.model_id) == 3 and capi.user_model_n_tab(b.model_id) == 4
    plain = models.Custom(4, 2, tm.generic_consts(3), tm.generic_source(4, 2, 3, False))
    assert capi.user_model_n_tab(plain.model_id) == 0 and plain.table is None and plain.n_tab == 0
    assert capi.user_model_n_tab(capi.MODEL_CAR) == 0
    lib = capi.load_hip_library()
    assert lib.isls_user_model_n_tab(5) == capi.ERR_ARG and lib.isls_user_model_n_tab(1 << 20) == capi.ERR_ARG
    # the layout the device reads
    assert np.array_equal(a.device_params(None, 5), np.concatenate([[0.1], np.ones(15)]))
    assert c.device_params(3, 7).shape == (3, 1 + 21)


FOUR = "template <typename S, typename P>\n__device__ void step(const S *x, const S *u, const P *par, S *xn) { for (int i = 0; i < 4; ++i) xn[i] = x[i]; }"
FIVE = ("template <typename S, typename P>\n__device__ void step(const S *x, const S *u, const P *par, const P *row, S *xn) "
        "{ for (int i = 0; i < 4; ++i) xn[i] = x[i] * row[0]; }")


def test_refusals_of_the_front_end():
    with pytest.raises(capi.IslsError, match="at most 16 words"):
        models.Custom(4, 2, [0.1], FIVE, table=np.zeros((5, 17)))
    with pytest.raises(ValueError):
        models.Custom(4, 2, [0.1], FIVE, table=np.zeros((5, 0)))
    with pytest.raises(capi.IslsError, match=r"compile failed\n(.|\n)*error: no matching function for call to 'step'"):
        models.Custom(4, 2, [0.1], uc.fresh(FOUR), table=np.zeros((5, 2)))
    with pytest.raises(capi.IslsError, match=r"compile failed\n(.|\n)*error: no matching function for call to 'step'"):
        models.Custom(4, 2, [0.1], uc.fresh(FIVE))
    with pytest.raises(ValueError, match="one row and one table per trajectory"):
        models.Custom(4, 2, np.zeros((3, 1)), FIVE, table=np.zeros((2, 5, 2)))
    c = models.Custom(4, 2, [0.1], FIVE, table=np.zeros((5, 2)))
    for bad in (np.zeros((6, 2)), np.zeros((5, 3)), np.zeros((1, 5, 2))):
        with pytest.raises(ValueError, match="set_table"):
            c.set_table(bad)
    c.set_table(np.ones((5, 2)))
    assert (c.table == 1.0).all()
    with pytest.raises(ValueError, match="without a table"):
        models.Custom(4, 2, [0.1], FOUR).set_table(np.ones((5, 2)))
    # single rows without t=, a table of another horizon, another batch: refused before the device is touched
    with pytest.raises(ValueError, match="single rows need t="):
        c(np.zeros(4), np.zeros(2))
    with pytest.raises(ValueError, match="single rows need t="):
        c(np.zeros((6, 4)), np.zeros((6, 2)))
    with pytest.raises(ValueError, match="single rows need t="):
        c.get_AB(np.zeros((6, 4)), np.zeros((6, 2)))
    with pytest.raises(ValueError, match=r"steps in \[0, 5\)"):
        c(np.zeros(4), np.zeros(2), t=5)
    with pytest.raises(ValueError, match="horizon 6"):
        c.device_params(None, 6)
    cb = models.Custom(4, 2, [0.1], FIVE, table=np.zeros((3, 5, 2)))
    with pytest.raises(ValueError, match="the batch has 2"):
        cb.device_params(2, 5)


def test_refusals_of_the_library():
    """Validation comes before anything is compiled for a pair, loaded or launched, and needs no GPU: every call here is refused."""
    lib = capi.load_hip_library()
    mdl = models.Custom(4, 2, [0.1], FIVE, table=np.zeros((5, 2)))
    P, W, N, B = 1, 2, 5, 3
    dummy = ctypes.create_string_buffer(4096)
    ptr = ctypes.addressof(dummy)
    for sb, par, want in ((P, ptr, capi.ERR_ARG), (P + N * W + 1, ptr, capi.ERR_ARG), (N * W, ptr, capi.ERR_ARG), (0, None, capi.ERR_ARG)):
        a = capi.LinearizeArgs()
        a.B, a.N, a.n, a.m, a.model = B, N, 4, 2, mdl.model_id
        a.model_par, a.model_par_sb = par, sb
        a.xhat = a.uhat = a.A = a.Bm = ptr
        assert lib.isls_linearize_f64(ctypes.byref(a), None) == want, (sb, par)
        r = capi.RolloutArgs()
        r.B, r.N, r.n, r.m, r.L, r.model = B, N, 4, 2, 4, mdl.model_id
        r.model_par, r.model_par_sb = par, sb
        for f in ("K", "k", "xhat", "uhat", "alphas", "Qtab", "ztab", "seq", "x_out", "u_out"):
            setattr(r, f, ptr)
        r.nvia = 1
        assert lib.isls_rollout_ls_f64(ctypes.byref(r), None) == want, (sb, par)
        s = capi.SampleArgs()
        s.B, s.N, s.n, s.m, s.S, s.model = B, N, 4, 2, 8, mdl.model_id
        s.model_par, s.model_par_sb = par, sb
        s.temperature = 1.0
        for f in ("xhat", "uhat", "Qtab", "ztab", "seq", "sigma", "costs"):
            setattr(s, f, ptr)
        assert lib.isls_sample_nominal_f64(ctypes.byref(s), None) == want, (sb, par)
        q = capi.MpcStepArgs()
        q.B, q.N, q.n, q.m, q.model = B, N, 4, 2, mdl.model_id
        q.model_par, q.par_sb = par, sb
        q.xhat = q.uhat = ptr
        assert lib.isls_mpc_step_f64(ctypes.byref(q), None) == want, (sb, par)
    # the plant's buffer must reach row 0
    q = capi.MpcStepArgs()
    q.B, q.N, q.n, q.m, q.model = B, N, 4, 2, mdl.model_id
    q.model_par, q.par_sb, q.plant_par, q.plant_sb = ptr, 0, ptr, P
    q.xhat = q.uhat = ptr
    assert lib.isls_mpc_step_f64(ctypes.byref(q), None) == capi.ERR_ARG
    # the row-wise step: a table model through the entry without a table and the reverse
    plain = models.Custom(4, 2, [0.1], FOUR)
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert lib.isls_user_model_step_f64(i32(mdl.model_id), i32(2), vp(ptr), i64(0), vp(ptr), vp(ptr), vp(ptr), None) == capi.ERR_ARG
    assert lib.isls_user_model_step_tab_f64(i32(plain.model_id), i32(2), i32(1), i32(N), vp(ptr), i64(0), None, vp(ptr), vp(ptr), vp(ptr),
                                            None) == capi.ERR_ARG
    assert lib.isls_user_model_step_tab_f64(i32(mdl.model_id), i32(2), i32(1), i32(N), vp(ptr), i64(P), None, vp(ptr), vp(ptr), vp(ptr),
                                            None) == capi.ERR_ARG
    # not served: the dense closed loop and the Monte-Carlo loop
    d = capi.DenseLoopArgs()
    d.M, d.N, d.n, d.m, d.model = 2, N, 4, 2, mdl.model_id
    for f in ("model_par", "K", "k", "x0", "x_log", "u_log"):
        setattr(d, f, ptr)
    assert lib.isls_dense_closed_loop_f64(ctypes.byref(d), None) == capi.ERR_UNSUPPORTED
    mc = capi.McLoopArgs()
    mc.P, mc.M, mc.N, mc.n, mc.m, mc.model = 2, 4, N, 4, 2, mdl.model_id
    for f in ("model_par", "K", "k", "xhat", "uhat", "x0", "x_log", "u_log"):
        setattr(mc, f, ptr)
    assert lib.isls_mc_closed_loop_f64(ctypes.byref(mc), None) == capi.ERR_UNSUPPORTED
    mc.model = plain.model_id                                  # (the refusal is the table's: the same block with NULL gains is an argument error)
    mc.K = None
    assert lib.isls_mc_closed_loop_f64(ctypes.byref(mc), None) == capi.ERR_ARG


def test_version_and_struct_sizes_stand():
    lib = capi.load_hip_library()
    assert lib.isls_version() == 107 and capi.ABI_VERSION == 107
    # the argument blocks through which a model's parameters travel, at the sizes they had before the table: it rides in the
    # buffer they already name
    pinned = dict(RolloutArgs=312, LinearizeArgs=80, DenseLoopArgs=88, McLoopArgs=376, MpcStepArgs=224, SampleArgs=256, OuterArgs=1176,
                  AdvanceArgs=432, ColumnsIterationArgs=1120, ExpandArgs=208, AdmmArgs=264, GainArgs=224, FfArgs=336)
    assert {k: ctypes.sizeof(getattr(capi, k)) for k in pinned} == pinned
    import test_capi_host as tch
    tch.test_struct_layouts_match_header()                      # ... and the header the library was compiled from says the same
    for name in ("isls_user_model_create_tab", "isls_user_model_n_tab", "isls_user_model_step_tab_f64", "isls_user_model_step_tab_f32"):
        assert hasattr(lib, name) and name in capi.EXPORTED


def test_the_refusal_names_the_alternative_and_spares_a_model_without_a_table():
    """The message alone: an iSLS needs a device, so the entry points themselves (monte_carlo, isls_admm, get_trajectory_sls, the
    batch form) are called in tests/test_table_model_gpu.py::test_refusing_entry_points."""
    from isls import iSLS
    q = iSLS.__new__(iSLS)
    q._host_model, q._forward_model = False, models.Custom(4, 2, [0.1], FIVE, table=np.zeros((5, 2)))
    for what in ("monte_carlo", "isls_admm", "get_trajectory_sls (the dense closed loop)", "the batch form"):
        with pytest.raises(capi.IslsError, match="fold the schedule into"):
            q._refuse_table_model(what)
    q._forward_model = models.Custom(4, 2, [0.1], FOUR)
    q._refuse_table_model("monte_carlo")
