"""GPU tests of the closed-loop sampling round (iSLS.sample_nominal(feedback=), isls_sample_nominal_fb_*, csrc/sampling.hpp)
against the numpy restatement tests/sampling_fb_reference.py.  The problems, shapes and bounds are those of
tests/test_sampling_gpu.py: B = 3, N in {2, 7} (N = 2: the first horizon where the feedback acts), S in {1, 63, 64, 65, 200},
fp64, rel 1e-9 for a device run against its host restatement.  Gains: uniform in [-0.5, 0.5], no two entries alike."""
import ctypes

import numpy as np
import pytest
import torch

import sampling_fb_reference as F
import sampling_reference as R
from isls import _capi as capi
from test_sampling_gpu import B, DRAW_COST, SIZES, make_ref, rel, rel_costs, solver

pytestmark = pytest.mark.gpu
KINDS = ("di21", "di63", "car", "arm", "quad_bump", "quad_track", "tassa", "sqrt")


def gains(p, per_traj=True, seed=0):
    rng = np.random.default_rng([seed, p["n"], p["N"]])
    G = rng.uniform(-0.5, 0.5, ((p["nb"],) if per_traj else ()) + (p["N"], p["m"], p["n"]))
    assert np.unique(G).size == G.size
    return G


def reference(p, G, **kw):
    return F.sample_nominal(p["step"], p["par"], p["cost"], p["xhat"], p["uhat"], G, kw.pop("sigma", p["sigma"]), **kw)


def clip_of(kind):
    return (4.2, 5.6) if kind.startswith("quad") else (-0.4, 0.5)


# ---- 1. sample costs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_sample_costs_match_the_reference(kind, N):
    p = make_ref(kind, N)
    q = solver(p)
    for k, S in enumerate(SIZES):
        clip = None if k % 2 == 0 else clip_of(kind)
        G = gains(p, per_traj=k % 3 != 0, seed=k)               # shared [N, m, n] and per trajectory [B, N, m, n], with and without a clip
        q.nominal_values = p["xhat"], p["uhat"]
        r = q.sample_nominal(samples=S, sigma=p["sigma"], seed=11 + k, clip_u=clip, return_costs=True, feedback=G)
        ref = reference(p, G, seed=11 + k, samples=S, clip_u=clip)
        err = rel_costs(r.costs, ref["costs"])
        print(f"{kind} N={N} S={S} clip={clip} G{G.shape}: costs rel {err:.2e}")
        assert err < 1e-9
        assert rel(r.cost_before, ref["cost_before"]) < 1e-9 and rel(r.cost_best_sample, ref["cost_best_sample"]) < 1e-9
        assert r.costs.shape == (B, S) and r.took_best.shape == r.ess.shape == (B, 1) and r.took_best.dtype == bool
        assert rel(q.cost, r.cost_after) < 1e-12               # the same terms, summed by the expansion in another order


def test_feedback_changes_the_costs():
    """the gains are not ignored: the same seed in open loop gives other costs from the second step on (N = 2: the last control)"""
    p = make_ref("car", 2)
    q = solver(p)
    a = q.sample_nominal(samples=65, sigma=p["sigma"], seed=3, return_costs=True).costs
    q.nominal_values = p["xhat"], p["uhat"]
    b = q.sample_nominal(samples=65, sigma=p["sigma"], seed=3, return_costs=True, feedback=gains(p)).costs
    assert rel(a[:, 0], b[:, 0]) < 1e-12 and np.median(np.abs(a[:, 1:] - b[:, 1:])) > 1e-6


# ---- 2. every gain entry is read where it belongs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
def test_every_gain_entry_is_read_where_it_belongs(dense):
    """identity LTI (2, 2), N = 2, a cost that is control r of step 1: costs[b, s] = ua_1[r] + G[b, 1, r, :] . eps[s, 0, :] + eps[s, 1, r]"""
    import isls
    from isls import costs, models
    from mc_reference import normals
    N, S, sigma = 2, 65, np.array([[1.0, 0.5], [2.0, 1.5], [0.25, 3.0]])
    b, s = np.meshgrid(np.arange(B), np.arange(S), indexing="ij")
    eps = [sigma[:, None, :] * normals(21, b, s, t, 2) for t in range(N)]
    for e in eps:
        e[:, 0] = 0.0
    rng = np.random.default_rng(5)
    u0 = rng.uniform(-1.0, 1.0, (B, N, 2))
    xs = np.concatenate([np.zeros((B, 1, 2)), u0[:, :1]], axis=1)   # a consistent nominal: x_0 = 0, x_1 = x_0 + u_0
    forms = [rng.uniform(-0.5, 0.5, (B, N, 2, 2))] if dense else []
    if not dense:
        for t in range(N):
            for r in range(2):
                for j in range(2):
                    G = np.zeros((B, N, 2, 2))
                    G[:, t, r, j] = np.array([0.5, -1.5, 2.5])
                    forms.append(G)
    for r in range(2):
        q = isls.iSLS(2, 2, N, batch=B)
        q.forward_model = models.LTI(np.eye(2), np.eye(2))
        q.cost_function = costs.Custom(2, 2, np.eye(4)[2 + r], DRAW_COST)
        for G in forms:
            q.nominal_values = xs, u0
            got = q.sample_nominal(samples=S, sigma=sigma, seed=21, return_costs=True, feedback=G).costs
            ref = u0[:, None, 1, r] + np.einsum("bj,bsj->bs", G[:, 1, r, :], eps[0]) + eps[1][..., r]
            assert np.max(np.abs(got - ref)) < 1e-12


# ---- 3. the updated plan -----------------------------------------------------------------------------------------------------------
# (kind, N, S, temperature, rounds, seed, clip): the seeds were chosen with the restatement alone so that, in every round and
# problem, the arg-min leads the runner-up and the decision of step 5 has a margin, both above 1e-6 relative -- asserted below
PLANS = [
    ("di63", 7, 200, 1.0, 2, 1, False),
    ("di63", 7, 65, 200.0, 1, 1, False),
    ("quad_bump", 7, 200, 0.01, 2, 1, True),
    ("car", 7, 64, 0.03, 1, 1, False),
    ("arm", 7, 65, 0.05, 1, 1, True),
    ("car", 2, 63, 1.0, 1, 2, True),
    # the candidate of step 5 taken by the library's own instantiations (the plans above take it in the run-time compiled program only)
    ("car", 7, 65, 0.01, 1, 1, True),
    ("di63", 7, 200, 0.003, 1, 2, False),
    ("di21", 7, 64, 0.001, 1, 4, False),
]
BUILT_IN_CANDIDATE = PLANS[-3:]


def _plan_reference(kind, N, S, temperature, rounds, seed, clip):
    p = make_ref(kind, N)
    G = gains(p, seed=seed)
    return p, G, reference(p, G, seed=seed, samples=S, temperature=temperature, rounds=rounds, clip_u=clip_of(kind) if clip else None)


@pytest.mark.parametrize("kind, N, S, temperature, rounds, seed, clip", PLANS)
def test_updated_plan_matches_the_reference(kind, N, S, temperature, rounds, seed, clip):
    p, G, ref = _plan_reference(kind, N, S, temperature, rounds, seed, clip)
    assert ref["lead"].min() > 1e-6 and ref["decide"].min() > 1e-6, (ref["lead"], ref["decide"])
    q = solver(p)
    r = q.sample_nominal(samples=S, sigma=p["sigma"], temperature=temperature, rounds=rounds, seed=seed, feedback=G,
                         clip_u=clip_of(kind) if clip else None)
    assert np.array_equal(r.took_best, ref["took_best"])
    assert rel(q.u_nom, ref["uhat"]) < 1e-9 and rel(q.x_nom, ref["xhat"]) < 1e-9
    assert rel(r.cost_after, ref["cost_after"]) < 1e-9 and rel(r.cost_before, ref["cost_before"]) < 1e-9
    assert rel(r.ess, ref["ess"]) < 1e-9 and rel(r.cost_best_sample, ref["cost_best_sample"]) < 1e-9
    assert rel(q.cost, r.cost_after) < 1e-12


def test_both_branches_of_the_selection_are_covered():
    took = [_plan_reference(*plan)[2]["took_best"] for plan in PLANS]
    assert any(t.any() for t in took) and any((~t).any() for t in took)
    for plan in BUILT_IN_CANDIDATE:                             # each of them takes the candidate somewhere
        assert (~_plan_reference(*plan)[2]["took_best"]).any(), plan


# ---- 4. feedback=True --------------------------------------------------------------------------------------------------------------
def _state(q, r):
    return q.x_nom, q.u_nom, r.costs, r.cost_before, r.cost_after, r.ess, r.took_best, r.cost_best_sample, np.asarray(q.cost)


@pytest.mark.parametrize("kind", ["di63", "car", "quad_track"])
def test_feedback_true_is_the_backward_pass_gains(kind):
    p = make_ref(kind, 7)
    q0 = solver(p)
    K0, _ = q0.backward_pass_DP()
    assert K0.shape == (B, 7, p["m"], p["n"]) and np.abs(K0).max() > 1e-3
    kw = dict(samples=65, sigma=p["sigma"], seed=5, return_costs=True)
    a = _state(q0, q0.sample_nominal(feedback=K0, **kw))
    q1 = solver(p)
    b = _state(q1, q1.sample_nominal(feedback=True, **kw))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    # as a device tensor, used in place
    q2 = solver(p)
    c = _state(q2, q2.sample_nominal(feedback=torch.as_tensor(K0, device=q2.engine.device), **kw))
    for u, v in zip(a, c):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("kind", ["di63", "car"])
def test_feedback_true_rounds_are_calls_in_a_row(kind):
    p = make_ref(kind, 7)
    kw = dict(samples=65, sigma=p["sigma"], feedback=True, return_costs=True)
    q0, q1 = solver(p), solver(p)
    r0 = q0.sample_nominal(rounds=2, seed=9, **kw)
    r1a = q1.sample_nominal(rounds=1, seed=9, **kw)
    r1b = q1.sample_nominal(rounds=1, seed=10, **kw)
    assert np.array_equal(q0.x_nom, q1.x_nom) and np.array_equal(q0.u_nom, q1.u_nom) and np.array_equal(q0.K, q1.K)
    assert np.array_equal(r0.costs, r1b.costs) and np.array_equal(r0.cost_after, r1b.cost_after)
    assert np.array_equal(r0.cost_before, r1a.cost_before)
    assert np.array_equal(r0.ess, np.concatenate([r1a.ess, r1b.ess], axis=1))
    assert np.array_equal(r0.took_best, np.concatenate([r1a.took_best, r1b.took_best], axis=1))


BUMP_ON_THE_PATH = np.array([0.05, 0.01, 40.0, 0.0, 0.0, 0.5, 0.01, 0.01, 1.0, 0.5])   # a tall bump where the guess starts


def test_feedback_true_on_an_indefinite_quu_needs_a_regularization():
    import isls
    p = make_ref("quad_bump", 7)
    p["ucost"] = ("bump", BUMP_ON_THE_PATH)
    q = solver(p)
    x0, u0 = q.x_nom.copy(), q.u_nom.copy()
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        q.sample_nominal(samples=65, sigma=p["sigma"], feedback=True)
    assert np.array_equal(q.x_nom, x0) and np.array_equal(q.u_nom, u0)          # before anything is sampled
    r = q.sample_nominal(samples=65, sigma=p["sigma"], feedback=True, regularization=isls.Regularization())
    assert (q.reg_mu > 0).any() and np.isfinite(r.cost_after).all() and np.all(r.cost_after <= r.cost_before)


# ---- 5. invariants on the device ---------------------------------------------------------------------------------------------------
def _consistent(p, q, clip):
    x = R.rollout(p["step"], q.x_nom[:, 0], q.u_nom, p["par"])
    assert rel(q.x_nom, x) < 1e-12
    if clip is not None:
        assert q.u_nom.min() >= clip[0] and q.u_nom.max() <= clip[1]


@pytest.mark.parametrize("kind", ["di63", "quad_bump", "arm"])
def test_cost_never_rises_runs_repeat_and_the_nominal_is_consistent(kind):
    p = make_ref(kind, 7)
    clip = clip_of(kind)
    G = gains(p)
    p["uhat"] = np.clip(p["uhat"], *clip)
    p["xhat"] = R.rollout(p["step"], p["xhat"][:, 0], p["uhat"], p["par"])
    took = []
    # temperature 1: the best sample wins everywhere; 0.01: the candidate wins in several problems and rounds -- by the restatement,
    # with a decision margin of 5e-5 relative or more in every problem and round of the three kinds, so no rounding moves a branch
    for T_ in (1.0, 0.01):
        out = []
        for _ in range(2):
            q = solver(p)
            r = q.sample_nominal(samples=200, sigma=p["sigma"], rounds=3, seed=2, temperature=T_, return_costs=True, feedback=G, clip_u=clip)
            assert np.all(r.cost_after <= r.cost_before)
            _consistent(p, q, clip)
            out.append((q.x_nom, q.u_nom, r.costs, r.cost_after, r.ess, r.took_best, r.cost_best_sample))
        for a, b_ in zip(*out):
            assert np.array_equal(a, b_)
        took.append(out[0][5])
    print(f"{kind}: took_best {[t.tolist() for t in took]}")
    last = np.concatenate([t[:, -1] for t in took])             # the round whose result the checks above have seen
    assert last.any() and (~last).any()                         # the stored nominal of both branches of step 5 was checked


@pytest.mark.parametrize("kind", ["di63", "quad_bump"])
def test_one_sample_or_no_spread_keeps_a_consistent_nominal(kind):
    p = make_ref(kind, 7)
    G = gains(p)
    q = solver(p)
    q.sample_nominal(samples=1, feedback=G)                     # the nominal becomes the device's own rollout of its controls
    assert rel(q.u_nom, p["uhat"]) < 1e-12
    x0, u0 = q.x_nom.copy(), q.u_nom.copy()
    for kw in (dict(samples=1, sigma=0.7), dict(samples=65, sigma=0.0), dict(samples=1, sigma=0.0, rounds=2)):
        r = q.sample_nominal(seed=4, feedback=G, **kw)
        assert rel(q.x_nom, x0) < 1e-13 and rel(q.u_nom, u0) < 1e-13
        assert rel(r.cost_after, r.cost_before) < 1e-13


def _c_round(e, G, costs, x=None, u=None, rows=None, **kw):
    x, u = (e.xhat, e.uhat) if x is None else (x, u)
    ztab = e.ztab if rows is None else e.ztab[rows].contiguous()
    e.kern.sample_nominal_fb(e.model, e.model_par, x, u, e.Qtab, ztab, e.seq, e.u_std, e._t(np.full(3, 0.5)), costs, K=G,
                             stream=torch.cuda.current_stream().cuda_stream, **kw)


def test_inactive_problems_are_left_alone():
    p = make_ref("di63", 7)
    q = solver(p)
    e = q.engine
    x0, u0 = e.xhat.clone(), e.uhat.clone()
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=e.device)
    costs = torch.full((B, 65), -7.0, dtype=e.dtype, device=e.device)
    stats = {k: torch.full((B,), -7.0, dtype=e.dtype, device=e.device) for k in ("cost_before", "cost_after", "cost_best", "ess")}
    stats["took_best"] = torch.full((B,), -7, dtype=torch.int32, device=e.device)
    e.sample_round(e._t(np.full(3, 0.5)), costs, seed=5, active=active, K=e._t(gains(p)), **stats)
    assert torch.equal(e.xhat[1], x0[1]) and torch.equal(e.uhat[1], u0[1]) and bool((costs[1] == -7.0).all())
    assert all(float(v[1]) == -7 for v in stats.values())
    assert not torch.equal(e.uhat[0], u0[0]) and not torch.equal(e.uhat[2], u0[2])
    assert all(float(v[b]) != -7 for v in stats.values() for b in (0, 2))
    assert torch.equal(e.xhat[:, 0], x0[:, 0])                  # xhat_0 is never written


def test_results_do_not_depend_on_the_batch():
    """problems [0, 1, 63, 64, 199] of a B = 200, S = 200 run against a B = 5 run of the same problems gathered (problem_ids),
    and the pair [63, 64] with problem0; gains per trajectory"""
    idx = [0, 1, 63, 64, 199]
    p = make_ref("di63", 7, nb=200)
    q = solver(p)
    e = q.engine
    xs, us = e.xhat.clone(), e.uhat.clone()
    G = e._t(gains(p))
    r = q.sample_nominal(samples=200, sigma=0.5, seed=8, return_costs=True, feedback=G)
    sel = torch.tensor(idx, device=e.device)
    for rows, kw in ((sel, dict(problem_ids=sel.to(torch.int32))), (sel[2:4], dict(problem0=63))):
        nb, at = len(rows), rows.cpu().numpy()
        x, u = xs[rows].contiguous(), us[rows].contiguous()
        costs = torch.zeros(nb, 200, dtype=e.dtype, device=e.device)
        after, ess = (torch.zeros(nb, dtype=e.dtype, device=e.device) for _ in range(2))
        _c_round(e, G[rows].contiguous(), costs, x, u, rows, seed=8, cost_after=after, ess=ess, **kw)
        assert np.array_equal(costs.cpu().numpy(), r.costs[at])
        assert torch.equal(x, e.xhat[rows]) and torch.equal(u, e.uhat[rows])
        assert np.array_equal(after.cpu().numpy(), r.cost_after[at]) and np.array_equal(ess.cpu().numpy(), r.ess[at, 0])


# ---- 6. fp32 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["di63", "car"])
def test_fp32_costs_are_as_good_as_numpy_float32(kind):
    """the criterion of test_sampling_gpu.test_fp32_costs_are_as_good_as_numpy_float32: the device's error against the fp64
    restatement is at most twice that of a float32 numpy evaluation of the same closed loops"""
    p = make_ref(kind, 7)
    G = gains(p)
    q = solver(p, dtype=np.float32)
    r = q.sample_nominal(samples=200, sigma=p["sigma"], seed=6, return_costs=True, feedback=G)
    ref = reference(p, G, seed=6, samples=200)["costs"]
    ref32 = reference(p, G, seed=6, samples=200, dtype=np.float32)["costs"]
    dev_err, np_err = rel(r.costs, ref), rel(ref32, ref)
    print(f"{kind}: fp32 device costs rel {dev_err:.3e}, numpy float32 rel {np_err:.3e}")
    assert dev_err <= 2 * np_err


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_null_gains_and_the_lds_limit_at_the_c_level():
    p = make_ref("di21", 7)
    q = solver(p)
    e = q.engine
    sigma, costs = e._t(np.full(1, 0.5)), torch.full((B, 65), -7.0, dtype=e.dtype, device=e.device)
    a = capi.Kernels.sample_args(e.model, e.model_par, e.xhat, e.uhat, e.Qtab, e.ztab, e.seq, e.u_std, sigma, costs)
    fn = e.kern.lib.isls_sample_nominal_fb_f64
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    x0, u0 = e.xhat.clone(), e.uhat.clone()
    assert fn(ctypes.byref(a), None, 0, None) == capi.ERR_ARG
    G = e._t(gains(p))
    assert fn(ctypes.byref(a), G.data_ptr(), -1, None) == capi.ERR_ARG
    # N (n + m) = 2049 * 3 words of 8 bytes: 24 bytes past the 48 KB; arrays of that horizon, so nothing could be read out of bounds
    N = 2049
    xl, ul = torch.zeros(B, N, 2, dtype=e.dtype, device=e.device), torch.zeros(B, N, 1, dtype=e.dtype, device=e.device)
    seq, Gl = torch.zeros(N, dtype=torch.int32, device=e.device), torch.zeros(N, 1, 2, dtype=e.dtype, device=e.device)
    al = capi.Kernels.sample_args(e.model, e.model_par, xl, ul, e.Qtab, e.ztab, seq, e.u_std, sigma, costs)
    assert fn(ctypes.byref(al), Gl.data_ptr(), 0, None) == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.IslsError, match="-> %d" % capi.ERR_UNSUPPORTED):
        e.kern.sample_nominal_fb(e.model, e.model_par, xl, ul, e.Qtab, e.ztab, seq, e.u_std, sigma, costs, K=Gl)
    torch.cuda.synchronize()
    assert bool((costs == -7.0).all()) and not bool(xl.any()) and not bool(ul.any())      # nothing was launched
    assert torch.equal(e.xhat, x0) and torch.equal(e.uhat, u0)


def test_a_callable_forward_model_is_refused():
    import isls
    q = isls.iSLS(2, 1, 7, batch=B)
    q.forward_model = lambda x, u: x
    for fb in (True, np.zeros((7, 1, 2))):
        with pytest.raises(capi.IslsError, match="runs on the device"):
            q.sample_nominal(samples=8, feedback=fb)
