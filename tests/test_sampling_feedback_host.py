"""CPU-side checks of the closed-loop sampling round (isls_sample_nominal_fb_*, iSLS.sample_nominal(feedback=)): the numpy
restatement against the open-loop one, the refusals (all raised before anything touches a device), the exported symbols, and
the new kernels' resources in the built library and in the run-time compiled programs."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

import sampling_fb_reference as F
import sampling_reference as R
import user_costs as uc
import user_models as um
from isls import _capi as capi
from isls import costs, models, sampling
from isls.isls import iSLS
from test_sampling_host import _NoLibrary, _di_problem, _valid, kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_kernels  # noqa: E402

sys.path.pop(0)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, temperature, rounds", [(1, 1.0, 1), (65, 1.0, 2), (200, 0.05, 2)])
def test_zero_gains_without_a_clip_are_the_open_loop_round(S, temperature, rounds):
    """G = 0, no clip: u = uhat + eps, e = eps, and the candidate is the open-loop rollout of uhat + sum w eps"""
    step, par, cost, xhat, uhat = _di_problem()
    G = np.zeros((uhat.shape[1], uhat.shape[2], xhat.shape[2]))
    a = R.sample_nominal(step, par, cost, xhat, uhat, 0.5, seed=3, samples=S, temperature=temperature, rounds=rounds)
    b = F.sample_nominal(step, par, cost, xhat, uhat, G, 0.5, seed=3, samples=S, temperature=temperature, rounds=rounds)
    assert np.array_equal(a["took_best"], b["took_best"])
    for k in ("costs", "xhat", "uhat", "cost_after", "cost_before", "ess"):
        assert rel(b[k], a[k]) < 1e-12, k


def test_restatement_stores_a_consistent_nominal_inside_the_clip():
    step, par, cost, xhat, uhat = _di_problem()
    B, N, m = uhat.shape
    G = -0.5 * np.random.default_rng(1).uniform(0.2, 1.0, (B, N, m, xhat.shape[2]))
    took = []
    for T_ in (1.0, 1e-3):
        out = F.sample_nominal(step, par, cost, xhat, uhat, G, 0.5, seed=4, samples=65, temperature=T_, rounds=2, clip_u=(-0.3, 0.4))
        assert np.all(out["cost_after"] <= out["cost_before"])
        assert rel(R.rollout(step, xhat[:, 0], out["uhat"], par), out["xhat"]) < 1e-13
        assert out["uhat"].min() >= -0.3 and out["uhat"].max() <= 0.4
        assert np.allclose(cost(out["xhat"], out["uhat"]), out["cost_after"], rtol=1e-13)
        took.append(out["took_best"])
    assert np.concatenate(took).any() and not np.concatenate(took).all()      # both branches of step 5


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
ARGS = dict(B=3, m=2, samples=8, sigma=0.5, temperature=1.0, rounds=1, clip_u=None, N=5, n=4)


@pytest.mark.parametrize("fb", [None, False, True, np.zeros((5, 2, 4)), np.zeros((3, 5, 2, 4)), torch.zeros(5, 2, 4),
                                np.zeros((5, 2, 4), dtype=np.float32), np.zeros((5, 2, 4)).tolist()])
def test_feedback_forms_that_pass(fb):
    sampling.check_args(**ARGS, feedback=fb)


def _with(shape, at, value):
    G = np.zeros(shape)
    G[at] = value
    return G


@pytest.mark.parametrize("fb", [
    np.zeros((5, 4, 2)), np.zeros((2, 4)), np.zeros((4, 5, 2, 4)), np.zeros((1, 5, 2, 4)), np.zeros((6, 2, 4)), np.zeros(40), 1.0,
    torch.zeros(5, 4, 2), _with((5, 2, 4), (4, 1, 3), np.nan), _with((3, 5, 2, 4), (2, 0, 0, 0), np.inf),
    torch.full((5, 2, 4), float("nan")), np.zeros((5, 2, 4), dtype=complex), np.full((5, 2, 4), "a"),
])
def test_feedback_refusals_need_no_library(fb):
    with pytest.raises(capi.IslsError):
        sampling.check_args(**ARGS, feedback=fb)
    with pytest.raises(capi.IslsError):
        sampling.check_feedback(fb, 3, 5, 2, 4)


def test_run_refuses_gains_before_the_engine_is_used():
    e = _NoLibrary(model=capi.MODEL_LTI, fast_dims=True, n=4, m=2, B=3, N=5)
    with pytest.raises(capi.IslsError, match="feedback"):
        sampling.run(e, feedback=np.zeros((5, 4, 2)))
    with pytest.raises(capi.IslsError, match="finite"):
        sampling.run(e, feedback=_with((5, 2, 4), (0, 0, 0), np.nan))
    with pytest.raises(capi.IslsError, match="feedback=True"):  # a bare True is the front end's: it hands run the callable
        sampling.run(e, feedback=True)
    e = types.SimpleNamespace(model=capi.MODEL_LTI, fast_dims=False, n=5, m=2, B=3, N=5)
    with pytest.raises(capi.IslsError, match="row-per-lane"):
        sampling.run(e, feedback=lambda: None)


@pytest.mark.parametrize("state, kw", [
    (dict(_host_model=True, _host_cost=False), dict(feedback=True)),             # a forward model that is a Python callable
    (dict(_host_model=False, _host_cost=True), dict(feedback=np.zeros((5, 1, 2)))),
    (dict(_host_model=False, _host_cost=False), dict(feedback=np.zeros((5, 2, 1)))),
    (dict(_host_model=False, _host_cost=False), dict(feedback=np.full((3, 5, 1, 2), np.inf))),
])
def test_front_end_refuses_before_the_engine_is_used(state, kw):
    s = iSLS.__new__(iSLS)
    s.__dict__.update(state, engine=_NoLibrary(model=capi.MODEL_DI), batch=3, x_dim=2, u_dim=1, N=5)
    with pytest.raises(capi.IslsError):
        s.sample_nominal(**kw)


@pytest.mark.parametrize("change, K, K_sb, code", [
    ({}, None, 0, capi.ERR_ARG), ({}, 0x1000, -1, capi.ERR_ARG), (dict(xhat=None), 0x1000, 0, capi.ERR_ARG),
    (dict(S=0), 0x1000, 0, capi.ERR_ARG), (dict(phase=3), 0x1000, 0, capi.ERR_ARG), (dict(temperature=0.0), 0x1000, 8, capi.ERR_ARG),
    (dict(n=5, m=1), 0x1000, 0, capi.ERR_UNSUPPORTED), (dict(model=capi.MODEL_CAR), 0x1000, 0, capi.ERR_UNSUPPORTED),
    (dict(N=1 << 20), 0x1000, 0, capi.ERR_UNSUPPORTED),
    (dict(N=2049), 0x1000, 0, capi.ERR_UNSUPPORTED),           # fp64: N (n + m) = 6147 words > 48 KB; the open-loop N m fits
])
def test_argument_errors_without_a_device(change, K, K_sb, code):
    lib = capi.load_hip_library()
    for sfx in ("f64", "f32"):
        if change.get("N") == 2049 and sfx == "f32":
            continue
        fn = getattr(lib, f"isls_sample_nominal_fb_{sfx}")
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        a = capi.SampleArgs(**{**_valid(), **change})
        assert fn(ctypes.byref(a), K, K_sb, None) == code, (sfx, change)
        assert fn(None, K, K_sb, None) == capi.ERR_ARG
    a = capi.SampleArgs(**{**_valid(), "B": 0})                # an empty batch is no error and launches nothing
    assert fn(ctypes.byref(a), 0x1000, 0, None) == capi.OK


# ---- the built library ------------------------------------------------------------------------------------------------------------
def test_symbols_and_version():
    lib = capi.load_hip_library()
    for s in ("isls_sample_nominal_fb_f64", "isls_sample_nominal_fb_f32"):
        assert hasattr(lib, s), s
        assert s in capi.EXPORTED
    assert lib.isls_version() == 107
    assert hasattr(capi.Kernels, "sample_nominal_fb")


def test_library_kernels_use_no_scratch():
    """every sample_* kernel of the library -- the open-loop pair and the closed-loop pair of every family of families.def in both
    precisions -- has no private segment, and the lane-per-sample kernels spill nothing"""
    tab = {k: v for k, v in scan_kernels.kernel_table().items() if "sample_" in k}
    fb = {k: v for k, v in tab.items() if "sample_cost_fb_kernel" in k or "sample_update_fb_kernel" in k}
    assert fb and len(tab) == 2 * len(fb), sorted(tab)          # one closed-loop kernel beside every open-loop one
    assert {k.replace("21sample_cost_fb_kernel", "18sample_cost_kernel").replace("23sample_update_fb_kernel", "20sample_update_kernel")
            .replace("9SampleFbP", "7SampleP") for k in fb} == set(tab) - set(fb)
    bad = {k: v["scratch"] for k, v in tab.items() if v["scratch"]}
    assert not bad, bad
    assert not any(v["spill"] for k, v in tab.items() if "sample_cost" in k)


@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_user_programs_hold_the_closed_loop_kernels_without_scratch(dtype, T):
    """the program of a Custom model and of a (model, cost) pair carries the closed-loop pair behind the open-loop one"""
    quad = models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
    bump6, bump4 = (costs.Custom(n, 2, uc.COUPLED_PAR, uc.coupled_source(n, 2)) for n in (6, 4))
    for code, n, model in [(quad.code(dtype), 6, 99), (bump6.code(quad, dtype), 6, 99), (bump4.code(models.CarSimple(0.1), dtype), 4, capi.MODEL_CAR)]:
        ks = kernels_of(code)
        mine = [k for k in ks if k.startswith(f"_ZN4isls21sample_cost_fb_kernelI{T}Li{n}ELi2ELi{model}E")
                or k.startswith(f"_ZN4isls23sample_update_fb_kernelI{T}Li{n}ELi2ELi{model}E")]
        assert len(mine) == 2, sorted(ks)
        for k in mine:
            assert ks[k][".private_segment_fixed_size"] == 0 and ks[k].get(".vgpr_spill_count", 0) == 0, (k, ks[k])
    assert not any("sample_" in k for k in kernels_of(bump6.code(None, dtype)))   # a cost alone has no model to roll out
