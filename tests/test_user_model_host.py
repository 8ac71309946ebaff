"""User-written forward models (isls.models.Custom) on the CPU: they compile at run time for gfx950 without a GPU, their code
objects hold every kernel the launches pick, their roll-out kernels need no more scratch than the built-in family of the same
dimensions, and bad sources are refused with a clear error.  The contract zoo (user_models.ZOO: every operation the dual-number
header offers, over the eight supported (n, m) pairs) compiles in both precisions, and its stored high-precision reference
(tests/golden/g14_*.npz) is what its generator produces."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from isls import _capi as capi
from isls import models

import table_models as tm
import user_models as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_kernels  # noqa: E402

sys.path.pop(0)

RO = re.compile(r"^_ZN4isls14rollout_kernelI([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEvNS_3RoPIT_EE$")
KERNEL = re.compile(r"^_ZN4isls\d+([a-z_]+_kernel)I([df])Li(\d+)ELi(\d+)E")

# the kernels of a run-time compiled program by the kind of its key, the roll-out variants apart
MODEL_KERNELS = {"user_linearize_kernel", "dense_closed_loop_kernel", "user_step_kernel", "mc_closed_loop_kernel", "mpc_step_kernel"}
COST_KERNELS = {"user_expand_kernel", "user_cost_value_kernel"}
SAMPLING_KERNELS = {"sample_cost_kernel", "sample_update_kernel", "sample_cost_fb_kernel", "sample_update_fb_kernel"}


@pytest.fixture(scope="module")
def library_table():
    return scan_kernels.kernel_table(scan_kernels.DEFAULT_LIB)


@pytest.fixture(scope="module")
def car():
    return models.Custom(4, 2, [0.1], um.CAR)


@pytest.fixture(scope="module")
def quad():
    return models.Custom(6, 2, um.QUAD_PAR, um.QUAD)


@pytest.fixture(scope="module")
def car_tab():
    return models.Custom(4, 2, [0.0], tm.generic_source(4, 2, 16, True), table=np.tile(tm.generic_consts(16), (5, 1)))


@pytest.fixture(scope="module")
def lti_tab():
    return models.Custom(6, 3, [0.0], tm.generic_source(6, 3, 16, True), table=np.tile(tm.generic_consts(16), (5, 1)))


def kernels_of(code):
    md = scan_kernels._metadata(code)
    return {k[".name"]: k for k in md["amdhsa.kernels"]}


def rollout_variants(names, prec, n, m, model):
    """{(JM, OCC): name} of the rollout kernels of one family"""
    out = {}
    for k in names:
        g = RO.match(k)
        if g and g.group(1) == prec and (int(g.group(2)), int(g.group(3)), int(g.group(4))) == (n, m, model):
            out[(int(g.group(5)), int(g.group(6)))] = k
    return out


def assert_kernel_set(ks, prec, n, m, expected, rollouts):
    """The code object holds exactly `expected` (one instantiation each) and `rollouts` roll-out variants, all of (prec, n, m)."""
    found = [KERNEL.match(k) for k in ks]
    assert all(found), sorted(ks)
    assert {(g.group(2), int(g.group(3)), int(g.group(4))) for g in found} == {(prec, n, m)}, sorted(ks)
    base = sorted(g.group(1) for g in found)
    assert base == sorted(list(expected) + ["rollout_kernel"] * rollouts), (base, sorted(expected), rollouts)


@pytest.mark.parametrize("which, n, m, builtin", [("car", 4, 2, capi.MODEL_CAR), ("quad", 6, 2, capi.MODEL_LTI),
                                                  ("car_tab", 4, 2, capi.MODEL_CAR), ("lti_tab", 6, 3, capi.MODEL_LTI)])
@pytest.mark.parametrize("dtype, prec", [(np.float64, "d"), (np.float32, "f")])
def test_code_object_holds_every_kernel(request, library_table, which, n, m, builtin, dtype, prec):
    mdl = request.getfixturevalue(which)
    assert mdl.model_id >= capi.MODEL_USER_BASE
    code = mdl.code(dtype)
    assert code[:4] == b"\x7fELF"
    ks = kernels_of(code)
    T = "d" if prec == "d" else "f"
    assert f"_ZN4isls21user_linearize_kernelI{T}Li{n}ELi{m}EEEvNS_8UserLinPIT_EE" in ks
    assert f"_ZN4isls16user_step_kernelI{T}Li{n}ELi{m}EEEviPKT_lS3_S3_PS1_" in ks
    assert any(k.startswith(f"_ZN4isls24dense_closed_loop_kernelI{T}Li{n}ELi{m}ELi99E") for k in ks)
    # every (JM, OCC) variant the built-in family of these dimensions has, under the user template id
    mine = rollout_variants(ks, prec, n, m, 99)
    ref = rollout_variants(library_table, prec, n, m, builtin)
    assert ref and set(mine) == set(ref), (sorted(mine), sorted(ref))
    for jo, k in mine.items():
        r = library_table[ref[jo]]
        assert ks[k][".private_segment_fixed_size"] <= r["scratch"], (k, ks[k][".private_segment_fixed_size"], r)
    lin = ks[f"_ZN4isls21user_linearize_kernelI{T}Li{n}ELi{m}EEEvNS_8UserLinPIT_EE"]
    assert lin[".private_segment_fixed_size"] == 0 and lin.get(".vgpr_spill_count", 0) == 0
    # and nothing else: a model's own kernels, the sampling round, the table step of a table model only, nothing of a cost
    tab = {"user_step_tab_kernel"} if which.endswith("_tab") else set()
    assert_kernel_set(ks, prec, n, m, MODEL_KERNELS | SAMPLING_KERNELS | tab, len(ref))


def test_arm_compiles_within_the_builtin_scratch(library_table):
    arm = models.Custom(9, 3, [0.05], um.ARM3R)
    ks = kernels_of(arm.code(np.float64))
    mine, ref = rollout_variants(ks, "d", 9, 3, 99), rollout_variants(library_table, "d", 9, 3, capi.MODEL_ARM3R)
    assert set(mine) == set(ref)
    for jo, k in mine.items():
        assert ks[k][".private_segment_fixed_size"] <= library_table[ref[jo]]["scratch"], k
    assert ks["_ZN4isls21user_linearize_kernelIdLi9ELi3EEEvNS_8UserLinPIT_EE"][".private_segment_fixed_size"] == 0


@pytest.fixture(scope="module")
def zoo():
    made = {}

    def get(name):
        if name not in made:
            n, m, src = um.ZOO[name][:3]
            made[name] = models.Custom(n, m, np.zeros(um.NPAR[name]), src)
        return made[name]
    return get


@pytest.mark.parametrize("name", sorted(um.ZOO))
@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_zoo_compiles_in_both_precisions(zoo, name, dtype, T):
    """Every form of the contract builds for S = T (line search, closed loop, step) and S = Dual<T, 1> (linearisation) in fp64
    and fp32 -- for S = float a plain double next to an S (`x * x + 1.0` inside isls::py_mod or isls::sin_cos) is the case that
    used to be ambiguous -- and the linearisation of every supported (n, m) pair keeps its dual numbers in registers."""
    n, m = um.ZOO[name][:2]
    ks = kernels_of(zoo(name).code(dtype))
    lin = ks[f"_ZN4isls21user_linearize_kernelI{T}Li{n}ELi{m}EEEvNS_8UserLinPIT_EE"]
    assert f"_ZN4isls16user_step_kernelI{T}Li{n}ELi{m}EEEviPKT_lS3_S3_PS1_" in ks
    assert any(k.startswith(f"_ZN4isls24dense_closed_loop_kernelI{T}Li{n}ELi{m}ELi99E") for k in ks)
    assert rollout_variants(ks, T, n, m, 99)
    assert lin[".private_segment_fixed_size"] == 0 and lin.get(".vgpr_spill_count", 0) == 0, (name, lin)


def test_zoo_covers_every_supported_pair():
    assert sorted((v[0], v[1]) for v in um.ZOO.values()) == sorted(capi.supported_dims())


def test_contract_fixture_is_what_the_generator_gives(golden):
    """tests/golden/make_ad_contract.py, run again, reproduces every stored array bit for bit: points, parameter rows, 60-digit
    values and central-difference Jacobians, the same-precision CPU baselines, and the sin_cos point set with its 200-bit
    references."""
    pytest.importorskip("mpmath")
    import runpy
    gen = runpy.run_path(os.path.join(ROOT, "tests", "golden", "make_ad_contract.py"))      # leaves no bytecode beside the fixtures
    files = {"g14_ad_contract.npz": gen["contract_arrays"]()}
    files.update({f"g14_sin_cos_{k}.npz": v for k, v in gen["sin_cos_arrays"]().items()})
    for fname, arrs in files.items():
        g = golden(fname)
        assert sorted(g.files) == sorted(arrs), fname
        for k, v in arrs.items():
            assert g[k].dtype == np.asarray(v).dtype and np.array_equal(g[k], v, equal_nan=True), (fname, k)
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", fname)) < 1 << 20


def test_one_compile_per_source():
    a = models.Custom(4, 2, [0.1], um.CAR)
    b = models.Custom(4, 2, np.array([[0.1], [0.2]]), um.CAR)         # per-trajectory parameters: same program
    assert a.model_id == b.model_id


def test_syntax_error_carries_the_log():
    src = "template <typename S, typename P>\n__device__ void step(const S *x, const S *u, const P *par, S *xn) { xn[0] = x[0] + ; }"
    with pytest.raises(capi.IslsError, match="error: expected expression"):
        models.Custom(4, 2, [0.1], src)


def test_unknown_function_for_the_dual_type_is_a_compile_error():
    src = um.CAR.replace("isls::sin_cos(x[2], sn, cs);", "sn = erf(x[2]); cs = x[2];")
    with pytest.raises(capi.IslsError, match="compile failed"):
        models.Custom(4, 2, [0.1], src)


OUTSIDE = {"an integer cast of S": "int k = (int)x[2]; sn = x[2] * k; cs = x[2];",
           "an S where an int is needed": "int k = x[2]; sn = x[2] * k; cs = x[2];",
           "floor": "sn = floor(x[2]); cs = x[2];",
           "pow": "sn = pow(x[2], 2.0); cs = x[2];",
           "atan": "sn = atan(x[2]); cs = x[2];",
           "fmod": "sn = fmod(x[2], 2.0); cs = x[2];"}


@pytest.mark.parametrize("what", sorted(OUTSIDE))
def test_outside_the_contract_is_a_compile_error_with_the_log(what):
    """What the header names as outside the contract (integer casts of S, functions it does not list) compiles for S = T and
    fails for the dual type: the error carries the compiler's log, which points into the user's source."""
    src = um.CAR.replace("isls::sin_cos(x[2], sn, cs);", OUTSIDE[what])
    assert src != um.CAR
    with pytest.raises(capi.IslsError, match=r"compile failed\n(.|\n)*user_model:\d+:\d+: error:"):
        models.Custom(4, 2, [0.1], src)


@pytest.mark.parametrize("src", ['asm volatile("s_nop 0");', "__asm__(\"s_nop 0\");", "xn[0] = __builtin_amdgcn_readfirstlane(1);"])
def test_assembly_is_refused(src):
    body = "template <typename S, typename P>\n__device__ void step(const S *x, const S *u, const P *par, S *xn) { " + src + " }"
    with pytest.raises(capi.IslsError, match="plain arithmetic"):
        models.Custom(4, 2, [0.1], body)
    # the library refuses it too, whoever calls it
    lib, mid = capi.load_hip_library(), ctypes.c_int32(-1)
    assert lib.isls_user_model_create(body.encode(), 4, 2, 1, ctypes.byref(mid)) == capi.ERR_ARG


def test_dimensions_outside_the_fast_pairs_are_refused():
    with pytest.raises(capi.IslsError, match=r"\(5, 2\)"):
        models.Custom(5, 2, [0.1], um.CAR)
    lib, mid = capi.load_hip_library(), ctypes.c_int32(-1)
    assert lib.isls_user_model_create(um.CAR.encode(), 5, 2, 1, ctypes.byref(mid)) == capi.ERR_UNSUPPORTED


def test_too_many_parameters_are_refused():
    with pytest.raises(capi.IslsError, match="at most 16"):
        models.Custom(4, 2, np.zeros(17), um.CAR)
    lib, mid = capi.load_hip_library(), ctypes.c_int32(-1)
    assert lib.isls_user_model_create(um.CAR.encode(), 4, 2, 17, ctypes.byref(mid)) == capi.ERR_UNSUPPORTED
