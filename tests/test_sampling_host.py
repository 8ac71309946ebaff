"""CPU-side checks of the sampling warm start (isls_sample_nominal_*, iSLS.sample_nominal): the exported symbols and the ctypes
mirror, the refusals (all raised before anything touches a device), the run-time compiled programs carry the two kernels without
scratch, the library's instantiations, and the numpy restatement's own invariants."""
import ctypes
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest

import sampling_reference as R
import table_costs as tc
import user_costs as uc
import user_models as um
from isls import _capi as capi
from isls import costs, models, sampling
from isls.isls import iSLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_kernels  # noqa: E402

sys.path.pop(0)


def test_symbols_and_version():
    lib = capi.load_hip_library()
    for s in ("isls_sample_nominal_f64", "isls_sample_nominal_f32"):
        assert hasattr(lib, s), s
        assert s in capi.EXPORTED
    assert lib.isls_version() == 107
    assert hasattr(capi.Kernels, "sample_nominal") and hasattr(iSLS, "sample_nominal")


def test_struct_layout_matches_header():
    """size and every offset of isls_sample_args as gcc lays the header out == the ctypes mirror"""
    fields = [f[0] for f in capi.SampleArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "isls_hip.h"\nint main(){printf("%zu\\n", sizeof(isls_sample_args));' + \
          "".join(f'printf("%zu\\n", offsetof(isls_sample_args, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == ctypes.sizeof(capi.SampleArgs)
    assert got[1:] == [getattr(capi.SampleArgs, f).offset for f in fields]


def _valid():
    """an argument block that passes every check (the pointers are never followed: the errors come first)"""
    p = 0x1000
    return dict(B=3, N=4, n=2, m=1, S=5, model=capi.MODEL_DI, cost_model=capi.COST_VIA, nvia=1, model_par=p, xhat=p, uhat=p, Qtab=p,
                ztab=p, seq=p, sigma=p, costs=p, temperature=1.0)


@pytest.mark.parametrize("change, code", [
    (dict(xhat=None), capi.ERR_ARG), (dict(uhat=None), capi.ERR_ARG), (dict(model_par=None), capi.ERR_ARG),
    (dict(sigma=None), capi.ERR_ARG), (dict(costs=None), capi.ERR_ARG),
    (dict(Qtab=None), capi.ERR_ARG), (dict(ztab=None), capi.ERR_ARG), (dict(seq=None), capi.ERR_ARG),
    (dict(N=0), capi.ERR_ARG), (dict(S=0), capi.ERR_ARG), (dict(S=-4), capi.ERR_ARG), (dict(B=-1), capi.ERR_ARG),
    (dict(n=0), capi.ERR_ARG), (dict(m=0), capi.ERR_ARG),
    (dict(model_par_sb=-1), capi.ERR_ARG), (dict(cost_par_sb=-1), capi.ERR_ARG), (dict(sigma_sb=-1), capi.ERR_ARG),
    (dict(Qtab_sb=-1), capi.ERR_ARG), (dict(ztab_sb=-1), capi.ERR_ARG), (dict(stat_sb=-1), capi.ERR_ARG),
    (dict(temperature=0.0), capi.ERR_ARG), (dict(temperature=-1.0), capi.ERR_ARG), (dict(temperature=float("nan")), capi.ERR_ARG),
    (dict(temperature=float("inf")), capi.ERR_ARG), (dict(phase=3), capi.ERR_ARG), (dict(phase=-1), capi.ERR_ARG),
    (dict(cost_model=capi.COST_USER_BASE + 10 ** 6, cost_par=0x1000), capi.ERR_ARG),   # a cost nobody registered
    (dict(n=5, m=1), capi.ERR_UNSUPPORTED),                                            # no row-per-lane kernels
    (dict(model=capi.MODEL_CAR), capi.ERR_UNSUPPORTED),                                # no car at (2, 1)
    (dict(cost_model=capi.COST_PHUBER, cost_par=0x1000), capi.ERR_UNSUPPORTED),        # pseudo-Huber: the Tassa model's
    (dict(N=1 << 20), capi.ERR_UNSUPPORTED),                                           # u_new [N, m] does not fit the LDS
    (dict(B=1 << 20, S=1 << 20), capi.ERR_UNSUPPORTED),                                # more workgroups than a grid holds
])
def test_argument_errors_without_a_device(change, code):
    lib = capi.load_hip_library()
    for sfx in ("f64", "f32"):
        fn = getattr(lib, f"isls_sample_nominal_{sfx}")
        fn.restype = ctypes.c_int
        a = capi.SampleArgs(**{**_valid(), **change})
        assert fn(ctypes.byref(a), None) == code, (sfx, change)
        assert fn(None, None) == capi.ERR_ARG
    a = capi.SampleArgs(**{**_valid(), "B": 0})                # an empty batch is no error and launches nothing
    assert lib.isls_sample_nominal_f64(ctypes.byref(a), None) == capi.OK


@pytest.mark.parametrize("kw", [
    dict(samples=0), dict(samples=-3), dict(samples=2.5), dict(rounds=0), dict(temperature=0.0), dict(temperature=-1.0),
    dict(temperature=float("nan")), dict(sigma=-0.1), dict(sigma=[0.1, float("inf")]), dict(sigma=[0.1, float("nan")]),
    dict(sigma=[0.1, 0.2, 0.3]), dict(clip_u=(1.0, 0.0)), dict(clip_u=([0.0, 2.0], [1.0, 1.0])), dict(clip_u=(0.0, float("nan"))),
])
def test_refusals_need_no_library(kw):
    args = dict(B=3, m=2, samples=8, sigma=0.5, temperature=1.0, rounds=1, clip_u=None)
    sampling.check_args(**args)                                 # the base case passes
    with pytest.raises(capi.IslsError):
        sampling.check_args(**{**args, **kw})


class _NoLibrary:
    """an engine whose every use is an error: the front end must refuse before it touches one"""
    def __init__(self, **known):
        self.__dict__.update(known)

    def __getattr__(self, name):
        raise AssertionError(f"the engine was used ({name}) before the refusal")


@pytest.mark.parametrize("state, kw", [
    (dict(_host_model=True, _host_cost=False), {}),             # a forward model that is a Python callable
    (dict(_host_model=False, _host_cost=True), {}),             # a cost that is one
    (dict(_host_model=False, _host_cost=False), dict(samples=0)),
    (dict(_host_model=False, _host_cost=False), dict(clip_u=(2.0, 1.0))),
])
def test_front_end_refuses_before_the_engine_is_used(state, kw):
    s = iSLS.__new__(iSLS)
    s.__dict__.update(state, engine=_NoLibrary(model=capi.MODEL_DI), batch=3, x_dim=2, u_dim=1, N=5)
    with pytest.raises(capi.IslsError):
        s.sample_nominal(**kw)


def test_pairs_outside_the_fast_ones_are_refused():
    e = types.SimpleNamespace(model=capi.MODEL_LTI, fast_dims=False, n=5, m=2, B=3)
    with pytest.raises(capi.IslsError, match="row-per-lane"):
        sampling.run(e)


def kernels_of(code):
    return {k[".name"]: k for k in scan_kernels._metadata(code)["amdhsa.kernels"]}


def _sampling_kernels(ks, T, n, m, model):
    out = [k for k in ks if k.startswith(f"_ZN4isls18sample_cost_kernelI{T}Li{n}ELi{m}ELi{model}E")
           or k.startswith(f"_ZN4isls20sample_update_kernelI{T}Li{n}ELi{m}ELi{model}E")]
    assert len(out) == 2, sorted(ks)
    return out


@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_user_programs_hold_the_two_kernels_without_scratch(dtype, T):
    """the program of a Custom model, and of a (model, cost) pair -- the bump cost and a table cost on the quadrotor, the bump on
    the car source and on a built-in model -- compile with sample_cost_kernel and sample_update_kernel, state and draws in registers"""
    car, quad = models.Custom(4, 2, [0.1], um.CAR), models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
    bump6, bump4 = (costs.Custom(n, 2, uc.COUPLED_PAR, uc.coupled_source(n, 2)) for n in (6, 4))
    track = costs.Custom(6, 2, [0.01], tc.tracking_source(6, 2), table=np.zeros((5, tc.width(6))))
    programs = [(car.code(dtype), 4, 99), (quad.code(dtype), 6, 99), (bump6.code(quad, dtype), 6, 99), (track.code(quad, dtype), 6, 99),
                (bump4.code(car, dtype), 4, 99), (bump4.code(models.CarSimple(0.1), dtype), 4, capi.MODEL_CAR)]
    for code, n, model in programs:
        ks = kernels_of(code)
        for k in _sampling_kernels(ks, T, n, 2, model):
            assert ks[k][".private_segment_fixed_size"] == 0 and ks[k].get(".vgpr_spill_count", 0) == 0, (k, ks[k])
    assert not any("sample_" in k for k in kernels_of(bump6.code(None, dtype)))   # a cost alone has no model to roll out


def test_library_kernels_use_no_scratch():
    """every family of families.def in both precisions: state, control, running cost and the generator in registers -- no
    private segment.  (The fp64 update of the 3R arm holds 295 registers and parks 24 of them in the accumulation half of the
    unified file: no memory traffic, one wavefront per SIMD.)"""
    tab = {k: v for k, v in scan_kernels.kernel_table().items() if "sample_cost_kernel" in k or "sample_update_kernel" in k}
    assert len(tab) == 2 * 2 * 14, sorted(tab)
    bad = {k: v["scratch"] for k, v in tab.items() if v["scratch"]}
    assert not bad, bad
    assert not any(v["spill"] for k, v in tab.items() if "sample_cost_kernel" in k)


# ---- the restatement itself --------------------------------------------------------------------------------------------------------
def _di_problem(B=3, N=7, d=1, seed=0):
    rng = np.random.default_rng(seed)
    n = 2 * d
    par = np.array([0.1, 0.005, 0.1])
    zs = np.zeros((2, n))
    zs[1, :d] = 1.0
    Qs = np.zeros((2, n, n))
    Qs[1] = np.diag(rng.uniform(5.0, 10.0, n))
    seq = np.zeros(N, dtype=np.int32)
    seq[-1] = 1
    xhat = np.zeros((B, N, n))
    xhat[:, 0] = rng.uniform(-0.5, 0.5, (B, n))
    uhat = rng.uniform(-0.5, 0.5, (B, N, d))
    step = R.model("di")
    xhat = R.rollout(step, xhat[:, 0], uhat, par)
    return step, par, R.via_cost(zs, Qs, seq, 1e-2), xhat, uhat


@pytest.mark.parametrize("S", [1, 2, 65])
@pytest.mark.parametrize("clip", [None, (-0.3, 0.4)])
def test_reference_never_raises_the_cost(S, clip):
    step, par, cost, xhat, uhat = _di_problem()
    out = R.sample_nominal(step, par, cost, xhat, uhat, 0.5, seed=3, samples=S, rounds=3, clip_u=clip)
    assert np.all(out["cost_after"] <= out["cost_before"])
    assert np.all(np.diff(out["cost_best_sample"], axis=1) <= 0)              # sample 0 of a round is the round before's result
    assert np.allclose(cost(out["xhat"], out["uhat"]), out["cost_after"], rtol=1e-13)
    assert np.all((out["ess"] >= 1 - 1e-12) & (out["ess"] <= S + 1e-9))


@pytest.mark.parametrize("kw", [dict(samples=1, sigma=0.5), dict(samples=33, sigma=0.0)])
def test_reference_keeps_the_nominal_bit_for_bit(kw):
    step, par, cost, xhat, uhat = _di_problem()
    out = R.sample_nominal(step, par, cost, xhat, uhat, seed=5, rounds=2, **kw)
    assert np.array_equal(out["uhat"], uhat) and np.array_equal(out["xhat"], xhat)
    assert np.array_equal(out["cost_after"], out["cost_before"]) and out["took_best"].all()


def test_reference_draws_are_the_generators():
    from mc_reference import normals
    eps = R.draws(7, 2, 3, 4, 5, [[1.0] * 5, [2.0] * 5], problem0=10)
    assert np.all(eps[:, 0] == 0)
    assert np.array_equal(eps[1, 2, 3], 2.0 * normals(7, 11, 2, 3, 5))
