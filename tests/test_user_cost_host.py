"""User-written cost functions (isls.costs.Custom) on the CPU: they compile at run time for gfx950 without a GPU, the code object of
a (cost, model) pair holds the expansion, the value and every roll-out variant of the model's built-in family, those need no more
scratch than the built-in ones, the expansion keeps its hyper-dual numbers in registers, bad sources are refused with a clear
error, and the numpy derivatives the GPU tests compare against agree with central differences."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

from isls import _capi as capi
from isls import costs, models

import al_reference as al
import user_costs as uc
import user_models as um
from test_user_model_host import COST_KERNELS, SAMPLING_KERNELS, assert_kernel_set, kernels_of, rollout_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_kernels  # noqa: E402

sys.path.pop(0)

PH = dict(cu=[0.01, 0.0001], cx=[0.001, 0.001, 0.0, 0.0], px=[0.1, 0.1, 1.0, 1.0], cf=[0.1, 0.1, 1.0, 0.3], pf=[0.01, 0.01, 0.01, 1.0])


@pytest.fixture(scope="module")
def library_table():
    return scan_kernels.kernel_table(scan_kernels.DEFAULT_LIB)


def pair(which):
    """(cost, model or None, n, m, template id of the model in the pair's program, built-in family to compare with)"""
    alone = {"alone_42": (4, 2), "alone_62": (6, 2), "con_42": (4, 2), "con_63": (6, 3)}
    if which in alone:
        n, m = alone[which]
        if which.startswith("con"):
            return costs.Custom(n, m, al.PAR, al.full_source(n, m, 0, 3), constraints=3), None, n, m, None, None
        return costs.Custom(n, m, uc.COUPLED_PAR, uc.coupled_source(n, m)), None, n, m, None, None
    if which == "coupled_car":
        return costs.Custom(4, 2, uc.COUPLED_PAR, uc.coupled_source(4, 2)), models.Custom(4, 2, [0.1], um.CAR), 4, 2, 99, capi.MODEL_CAR
    if which == "phuber_tassa":
        c = costs.Custom(4, 2, uc.phuber_params(PH["cu"], PH["cx"], PH["cf"]), uc.phuber_source(4, 2, PH["px"], PH["pf"]))
        return c, models.TassaCar(0.03), 4, 2, capi.MODEL_TASSA, capi.MODEL_TASSA
    if which == "via_arm":
        return costs.Custom(9, 3, uc.VIA_ARM_PAR, uc.via_arm_source(**uc.VIA_ARM_W)), models.Planar3R(0.05), 9, 3, capi.MODEL_ARM3R, capi.MODEL_ARM3R
    return (costs.Custom(6, 2, uc.COUPLED_PAR, uc.coupled_source(6, 2)), models.Custom(6, 2, um.QUAD_PAR, um.QUAD), 6, 2, 99,
            capi.MODEL_LTI)


@pytest.mark.parametrize("which", ["phuber_tassa", "via_arm", "coupled_quad", "coupled_car", "alone_42", "alone_62", "con_42", "con_63"])
@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_code_object_holds_every_kernel(library_table, which, dtype, T):
    cost, mdl, n, m, tid, builtin = pair(which)
    assert cost.cost_model >= capi.COST_USER_BASE
    code = cost.code(mdl, dtype)
    assert code[:4] == b"\x7fELF"
    ks = kernels_of(code)
    exp = ks[f"_ZN4isls18user_expand_kernelI{T}Li{n}ELi{m}EEEvNS_8UserExpPIT_EE"]
    assert any(k.startswith(f"_ZN4isls22user_cost_value_kernelI{T}Li{n}ELi{m}E") for k in ks)
    mine = rollout_variants(ks, T, n, m, tid)
    ref = rollout_variants(library_table, T, n, m, builtin) if mdl is not None else {}
    assert (ref or mdl is None) and set(mine) == set(ref), (sorted(mine), sorted(ref))
    for jo, k in mine.items():
        r = library_table[ref[jo]]
        assert ks[k][".private_segment_fixed_size"] <= r["scratch"], (k, ks[k][".private_segment_fixed_size"], r)
    assert exp[".private_segment_fixed_size"] == 0 and exp.get(".vgpr_spill_count", 0) == 0, exp
    # and nothing else: the cost's kernels, its multiplier update with constraints only, the sampling round and the roll-outs
    # with a model only, none of a model's own kernels
    con = {"user_constraint_update_kernel"} if which.startswith("con") else set()
    assert_kernel_set(ks, T, n, m, COST_KERNELS | con | (SAMPLING_KERNELS if mdl is not None else set()), len(ref))


@pytest.mark.parametrize("n, m", [(4, 2), (6, 2), (9, 3)])
@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_expansion_stays_in_registers(n, m, dtype, T):
    ks = kernels_of(costs.Custom(n, m, uc.COUPLED_PAR, uc.coupled_source(n, m)).code(None, dtype))
    exp = ks[f"_ZN4isls18user_expand_kernelI{T}Li{n}ELi{m}EEEvNS_8UserExpPIT_EE"]
    assert exp[".private_segment_fixed_size"] == 0 and exp.get(".vgpr_spill_count", 0) == 0, exp


# every operation of the contract on the hyper-dual type (and on S = T), in both precisions
EVERY_OP = r'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {
    S s, c;
    isls::sin_cos(x[0] * 0.5, s, c);
    S a = sin(x[1]) + cos(u[0]) - sqrt(x[2] * x[2] + 1.0) * exp(-x[3]) / (2 + tanh(u[1]));
    a += log(x[0] * x[0] + par[0]) * asin(0.5 * tanh(x[1])) + atan2(x[2], x[3] + 3.0) + atan2(1.0, x[0]) + atan2(x[1], 2.0);
    a -= fabs(u[0]) * isls::py_mod(x[2], 2) + isls::py_mod(x[3], x[0] * x[0] + 1.0) + isls::py_mod(3.0, x[1] * x[1] + 1.0);
    a *= S(1.5);
    a /= (1.0 + s * s + c);
    if (x[0] > 0.0 && 0.0 <= u[1] && x[1] != x[2] && !(x[3] == S(2)) && x[2] < x[3] && x[1] >= -x[1]) a = -a + (+a) * 2.0 - 1;
    return t == N - 1 ? a * a : a;
}
'''


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_operation_of_the_contract_compiles(dtype):
    assert costs.Custom(4, 2, [0.5], EVERY_OP).code(models.CarSimple(0.1), dtype)[:4] == b"\x7fELF"


def test_one_registration_per_source():
    a = costs.Custom(4, 2, uc.COUPLED_PAR, uc.coupled_source(4, 2))
    b = costs.Custom(4, 2, np.tile(uc.COUPLED_PAR, (3, 1)), uc.coupled_source(4, 2))   # per-trajectory parameters: same program
    assert a.cost_model == b.cost_model


def test_a_model_and_a_cost_of_the_same_id_number_are_told_apart():
    """Ids count per kind, so a model and a cost share their number as a matter of course: every lookup goes by kind."""
    warns = uc.coupled_source(4, 2).replace("S c = S(0), d2 = S(0);", "S c = S(0), d2 = S(0);\n    int narrowed = 1.5;")
    mdl, cst = uc.same_id_pair((4, 2, [0.1], um.CAR), (4, 2, uc.COUPLED_PAR, warns))
    uid = mdl.model_id
    assert uid == cst.cost_model
    lib = capi.load_hip_library()
    logs = []
    for fn in (lib.isls_user_model_log, lib.isls_user_cost_log):
        buf = ctypes.create_string_buffer(fn(uid, None, 0) + 1)
        fn(uid, buf, len(buf))
        logs.append(buf.value.decode())
    assert "user_cost:" in logs[1] and "warning" in logs[1] and "warning" not in logs[0]
    assert logs == [capi.user_model_log(uid), capi.user_cost_log(uid)]
    of_model, of_cost, of_pair = kernels_of(mdl.code()), kernels_of(cst.code()), kernels_of(cst.code(mdl))
    has = lambda ks, name: any(k.startswith(f"_ZN4isls{len(name)}{name}I") for k in ks)   # noqa: E731
    assert has(of_model, "user_linearize_kernel") and not has(of_model, "user_expand_kernel")
    assert has(of_cost, "user_expand_kernel") and not has(of_cost, "user_linearize_kernel")
    assert set(rollout_variants(of_pair, "d", 4, 2, 99)) == set(rollout_variants(of_model, "d", 4, 2, 99)) != set()
    assert has(of_pair, "user_expand_kernel") and not has(of_pair, "user_linearize_kernel")
    assert not rollout_variants(of_cost, "d", 4, 2, 99)


def test_one_compile_per_key_under_concurrency():
    """Four threads ask for the same (model, cost) program while a fifth registers models: one compile serves them all (the
    compiler's warning enters the cost's log once per compile), and sources and programs being under one lock, it ends."""
    warns = body("int narrowed = 1.5; return x[0] * u[1] + narrowed;")
    cost = costs.Custom(4, 2, [0.1], uc.fresh(warns))
    after_create = len(capi.user_cost_log(cost.cost_model))
    assert after_create > 0
    car, codes, ids = models.CarSimple(0.1), [None] * 4, []

    def ask(k):
        codes[k] = cost.code(car)

    def register():
        for _ in range(3):
            ids.append(models.Custom(2, 1, [0.1], uc.fresh(um.Z21)).model_id)
    threads = [threading.Thread(target=ask, args=(k,)) for k in range(4)] + [threading.Thread(target=register)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert codes[0][:4] == b"\x7fELF" and all(c == codes[0] for c in codes)
    assert len(set(ids)) == 3
    once = len(capi.user_cost_log(cost.cost_model))
    assert once > after_create                                 # the pair's compile added its warning ...
    assert cost.code(car) == codes[0]
    assert len(capi.user_cost_log(cost.cost_model)) == once    # ... and a fifth, later call compiles nothing
    assert once <= 2 * after_create + 64                       # one more compile's worth of messages, not four


def body(text):
    return "template <typename S, typename P>\n__device__ S stage(const S *x, const S *u, const P *par, int t, int N) { " + text + " }"


def test_syntax_error_carries_the_log():
    with pytest.raises(capi.IslsError, match="error: expected expression"):
        costs.Custom(4, 2, [0.1], body("return x[0] + ;"))


@pytest.mark.parametrize("what", ["return cosh(x[0]);", "int k = (int)x[2]; return x[2] * k;", "return pow(x[2], 2.0);"])
def test_outside_the_contract_is_a_compile_error_with_the_log(what):
    with pytest.raises(capi.IslsError, match=r"compile failed\n(.|\n)*user_cost:\d+:\d+: error:"):
        costs.Custom(4, 2, [0.1], body(what))


@pytest.mark.parametrize("src", ['asm volatile("s_nop 0"); return x[0];', "__asm__(\"s_nop 0\"); return x[0];",
                                 "return x[0] * __builtin_amdgcn_readfirstlane(1);"])
def test_assembly_is_refused(src):
    with pytest.raises(capi.IslsError, match="plain arithmetic"):
        costs.Custom(4, 2, [0.1], body(src))
    lib, cid = capi.load_hip_library(), ctypes.c_int32(-1)     # the library refuses it too, whoever calls it
    assert lib.isls_user_cost_create(body(src).encode(), 4, 2, 1, ctypes.byref(cid)) == capi.ERR_ARG


def test_dimensions_and_parameter_counts_are_refused():
    with pytest.raises(capi.IslsError, match=r"\(5, 2\)"):
        costs.Custom(5, 2, [0.1], body("return x[0];"))
    with pytest.raises(capi.IslsError, match="at most 16"):
        costs.Custom(4, 2, np.zeros(17), body("return x[0];"))
    lib, cid = capi.load_hip_library(), ctypes.c_int32(-1)
    assert lib.isls_user_cost_create(body("return x[0];").encode(), 5, 2, 1, ctypes.byref(cid)) == capi.ERR_UNSUPPORTED
    assert lib.isls_user_cost_create(body("return x[0];").encode(), 4, 2, 17, ctypes.byref(cid)) == capi.ERR_UNSUPPORTED
    # a cost of one pair with a model of another, or with a model its pair has no family for
    c = costs.Custom(4, 2, [0.1], body("return x[0] * u[1];"))
    with pytest.raises(capi.IslsError):
        c.code(models.Planar3R(0.05))
    with pytest.raises(capi.IslsError):
        c.code(models.Custom(6, 2, um.QUAD_PAR, um.QUAD))


def test_argument_blocks_keep_their_layout():
    """The parameter stride took the place of a padding word: sizes and the offsets of the neighbours are what they were."""
    for S in (capi.RolloutArgs, capi.ExpandArgs):
        assert S.cost_par_sb.offset == S.cost_model.offset + 4 and S.cost_par.offset == S.cost_model.offset + 8
    assert ctypes.sizeof(capi.RolloutArgs) == 312 and ctypes.sizeof(capi.ExpandArgs) == 208
    assert capi.load_hip_library().isls_version() == 107


@pytest.mark.parametrize("n, m", [(4, 2), (6, 2), (9, 3)])
def test_numpy_derivatives_of_the_coupled_cost(n, m):
    """The hand-written gradient and Hessian agree with central differences of the numpy value (per-trajectory parameters)."""
    rng = np.random.default_rng(n + m)
    B, N, h = 3, 6, 1e-5
    x, u = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
    par = uc.COUPLED_PAR * (1.0 + 0.1 * rng.normal(size=(B, uc.COUPLED_PAR.size)))
    _, g, H = uc.coupled_numpy(x, u, par)
    assert np.abs(H - np.swapaxes(H, -1, -2)).max() == 0.0
    assert np.abs(H[..., n:, :n]).max() > 0.01 and np.abs(H[..., 0, 1]).max() > 0.01      # x-u cross terms, off-diagonal H_xx
    assert np.abs(H[:, -1, 2, 2] - H[:, 0, 2, 2]).min() > 1.0                               # the terminal term
    w = np.concatenate([x, u], axis=-1)
    for k in range(n + m):
        for bb in range(B):
            for t in range(N):                                 # one entry at a time: the value is a sum over the steps
                wp, wm = w.copy(), w.copy()
                wp[bb, t, k] += h
                wm[bb, t, k] -= h
                vp, gp, _ = uc.coupled_numpy(wp[..., :n], wp[..., n:], par)
                vm, gm, _ = uc.coupled_numpy(wm[..., :n], wm[..., n:], par)
                assert abs((vp[bb] - vm[bb]) / (2 * h) - g[bb, t, k]) < 1e-7 * max(1.0, abs(g[bb, t, k]))
                assert np.abs((gp[bb, t] - gm[bb, t]) / (2 * h) - H[bb, t, k]).max() < 1e-7 * max(1.0, np.abs(H[bb, t]).max())
