"""GPU tests of the sampling warm start (iSLS.sample_nominal, isls_sample_nominal_*, csrc/sampling.hpp) against the numpy
restatement tests/sampling_reference.py.  B = 3 unless said, N in {2, 7}, S in {1, 63, 64, 65, 200} (one chunk of 64 lanes, its
edge, several chunks), fp64.  rel = max-abs error over max(1, |ref|_max): 1e-9 for a device run against its host restatement
(tests/test_user_model_gpu.py), 1e-12 absolute for the draws (tests/test_monte_carlo_gpu.py)."""
import numpy as np
import pytest
import torch

import sampling_reference as R
import table_costs as tc
import user_costs as uc
import user_models as um
from isls import _capi as capi

pytestmark = pytest.mark.gpu
B = 3
KINDS = ("di21", "di63", "car", "arm", "quad_bump", "quad_track", "tassa")
SIZES = (1, 63, 64, 65, 200)
SEED_NAN = 1                   # test_nan_samples_get_no_weight: chosen like the seeds of PLANS


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


def rel_costs(got, ref):
    """costs with +inf entries: the same entries are infinite, the others within rel"""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    return rel(np.where(fin, got, 0.0), np.where(fin, ref, 0.0))


# ---- problems: the numpy side (no device) and the solver over it ------------------------------------------------------------------
def _via(rng, nb, N, n, lead, u_std):
    """per-trajectory via points at the middle and the last step, weights on the first `lead` states"""
    zs, Qs = np.zeros((nb, 3, n)), np.zeros((3, n, n))
    zs[:, 1:, :lead] = rng.uniform(-1.0, 1.0, (nb, 2, lead))
    Qs[1, :lead, :lead] = np.diag(rng.uniform(2.0, 5.0, lead))
    Qs[1, 0, lead - 1] = Qs[1, lead - 1, 0] = 0.25 if lead > 1 else Qs[1, 0, 0]
    Qs[2] = np.diag(rng.uniform(5.0, 10.0, n))
    seq = np.zeros(N, dtype=np.int32)
    seq[N // 2], seq[N - 1] = 1, 2
    return zs, Qs, seq, u_std


def make_ref(kind, N, nb=B, seed=0, per_traj=False):
    """dict: n, m, step, par (model), cost, sigma, xhat, uhat and what the solver needs to be set up the same way"""
    rng = np.random.default_rng([seed, KINDS.index(kind) if kind in KINDS else 99, N])
    p = dict(kind=kind, N=N, nb=nb)
    if kind in ("di21", "di63"):
        d, dt = (1, 0.1) if kind == "di21" else (3, 0.05)
        n, m = 2 * d, d
        A, Bm = np.block([[np.eye(d), dt * np.eye(d)], [np.zeros((d, d)), np.eye(d)]]), np.vstack([0.5 * dt * dt * np.eye(d), dt * np.eye(d)])
        p.update(model=("lti", A, Bm), step=R.model("di"), par=np.array([dt, 0.5 * dt * dt, dt]), via=_via(rng, nb, N, n, d, 1e-2))
        x0, u0, sig = rng.uniform(-0.5, 0.5, (nb, n)), 0.3 * rng.standard_normal((nb, N, m)), 0.5
    elif kind == "car":
        n, m = 4, 2
        p.update(model=("car", 0.1), step=R.model("car"), par=np.array([0.1]), via=_via(rng, nb, N, n, 2, 1e-2))
        x0, u0, sig = np.tile([0.0, 0.0, 0.3, 1.0], (nb, 1)) + 0.1 * rng.standard_normal((nb, n)), 0.3 * rng.standard_normal((nb, N, m)), [0.4, 0.6]
    elif kind == "arm":
        n, m = 9, 3
        p.update(model=("arm", 0.05), step=R.model("arm"), par=np.array([0.05]), via=_via(rng, nb, N, n, 3, 1e-3))
        q0 = rng.uniform(0.2, 1.0, (nb, 3))
        c = np.cumsum(q0, axis=1)
        x0 = np.concatenate([q0, 0.1 * rng.standard_normal((nb, 3)), np.cos(c).sum(1, keepdims=True), np.sin(c).sum(1, keepdims=True),
                             np.zeros((nb, 1))], axis=1)
        u0, sig = rng.standard_normal((nb, N, m)), 1.5
    elif kind in ("quad_bump", "quad_track"):
        n, m = 6, 2
        par = np.tile(um.QUAD_PAR, (nb, 1)) * (1 + 0.1 * rng.uniform(-1, 1, (nb, 5))) if per_traj else um.QUAD_PAR.copy()
        p.update(model=("quad", par), step=R.model("quad"), par=par)
        x0 = np.concatenate([rng.uniform(-0.2, 0.2, (nb, 2)), 0.1 * rng.standard_normal((nb, 4))], axis=1)
        u0 = 4.9 + 0.3 * rng.standard_normal((nb, N, m))
        sig = rng.uniform(0.3, 0.9, (nb, m)) if per_traj else [0.5, 0.7]
        if kind == "quad_bump":
            cpar = np.tile(uc.COUPLED_PAR, (nb, 1)) * (1 + 0.2 * rng.uniform(-1, 1, (nb, 10))) if per_traj else uc.COUPLED_PAR.copy()
            p.update(ucost=("bump", cpar), cost=R.coupled_cost(cpar))
        else:
            table = tc.make_table(rng, N, n, nb if per_traj else None, terminal=5.0)
            p.update(ucost=("track", table), cost=R.tracking_cost(table, 1e-2))
    elif kind == "tassa":                                      # the pseudo-Huber cost: five vectors with no two entries alike
        n, m = 4, 2
        ph = (np.array([0.01, 0.02]), np.array([0.01, 0.02, 0.03, 0.04]), np.array([0.1, 0.2, 0.3, 0.4]),
              np.array([0.5, 1.0, 1.5, 2.0]), np.array([0.015, 0.025, 0.035, 0.045]))
        p.update(model=("tassa", 0.1, 2.0), step=R.model("tassa"), par=np.array([0.1, 2.0]), phuber=ph, cost=R.phuber_cost(*ph))
        x0 = np.tile([1.0, 1.0, 4.0, 0.5], (nb, 1)) + 0.1 * rng.standard_normal((nb, n))
        u0, sig = 0.3 * rng.standard_normal((nb, N, m)), [0.3, 0.5]
    elif kind == "sqrt":
        n, m = 2, 1
        p.update(model=("sqrt", np.array([0.1])), step=R.model("sqrt"), par=np.array([0.1]), via=_via(rng, nb, N, n, 2, 1e-2))
        x0, u0, sig = np.tile([0.08, 0.0], (nb, 1)), 0.5 + 0.1 * rng.uniform(size=(nb, N, m)), 1.0
    if "via" in p:
        p["cost"] = R.via_cost(*p["via"])
    p.update(n=n, m=m, sigma=sig, uhat=u0, xhat=R.rollout(p["step"], x0, u0, p["par"]))
    return p


def solver(p, dtype=np.float64):
    import isls
    from isls import costs, models
    n, m, N = p["n"], p["m"], p["N"]
    q = isls.iSLS(n, m, N, batch=p["nb"], dtype=dtype)
    what = p["model"]
    if what[0] == "lti":
        q.forward_model = models.LTI(what[1], what[2])
    elif what[0] == "car":
        q.forward_model = models.CarSimple(what[1])
    elif what[0] == "arm":
        q.forward_model = models.Planar3R(what[1])
    elif what[0] == "quad":
        q.forward_model = models.Custom(6, 2, what[1], um.QUAD)
    elif what[0] == "sqrt":
        q.forward_model = models.Custom(2, 1, what[1], R.SQRT_MODEL)
    elif what[0] == "tassa":
        q.forward_model = models.TassaCar(what[1], what[2])
    if "via" in p:
        q.set_cost_variables(*p["via"])
    elif "phuber" in p:
        q.cost_function = costs.PseudoHuber(*p["phuber"])
    elif p["ucost"][0] == "bump":
        q.cost_function = costs.Custom(6, 2, p["ucost"][1], uc.coupled_source(6, 2))
    else:
        q.cost_function = costs.Custom(6, 2, [1e-2], tc.tracking_source(6, 2), table=p["ucost"][1])
    q.reset()
    q.nominal_values = p["xhat"], p["uhat"]
    return q


def reference(p, **kw):
    return R.sample_nominal(p["step"], p["par"], p["cost"], p["xhat"], p["uhat"], kw.pop("sigma", p["sigma"]), **kw)


# ---- sample costs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_sample_costs_match_the_reference(kind, N):
    p = make_ref(kind, N)
    q = solver(p)
    for k, S in enumerate(SIZES):
        clip = None if k % 2 == 0 else ((4.2, 5.6) if kind.startswith("quad") else (-0.4, 0.5))
        q.nominal_values = p["xhat"], p["uhat"]
        r = q.sample_nominal(samples=S, sigma=p["sigma"], seed=11 + k, clip_u=clip, return_costs=True)
        ref = reference(p, seed=11 + k, samples=S, clip_u=clip)
        err = rel_costs(r.costs, ref["costs"])
        print(f"{kind} N={N} S={S} clip={clip}: costs rel {err:.2e}")
        assert err < 1e-9
        assert rel(r.cost_before, ref["cost_before"]) < 1e-9 and rel(r.cost_best_sample, ref["cost_best_sample"]) < 1e-9
        assert r.costs.shape == (B, S) and r.took_best.shape == r.ess.shape == (B, 1) and r.took_best.dtype == bool
        assert rel(q.cost, r.cost_after) < 1e-12               # the same terms, summed by the expansion in another order


@pytest.mark.parametrize("kind", ["quad_bump", "quad_track"])
def test_per_trajectory_parameters_and_sigma(kind):
    """model_par [B, 5], cost_par [B, 10] or a table per trajectory, sigma [B, m]; clip on and off"""
    p = make_ref(kind, 7, per_traj=True)
    q = solver(p)
    for S, clip in ((65, None), (200, (4.2, [5.6, 5.4]))):
        q.nominal_values = p["xhat"], p["uhat"]
        r = q.sample_nominal(samples=S, sigma=p["sigma"], seed=3, clip_u=clip, return_costs=True)
        ref = reference(p, seed=3, samples=S, clip_u=clip)
        assert rel_costs(r.costs, ref["costs"]) < 1e-9
        rows = ref["costs"] - ref["costs"][0]                   # the trajectories' parameters differ: so do their costs
        assert np.abs(rows[1:]).max() > 1e-3


DRAW_COST = r'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {
    return par[2 * t] * u[0] + par[2 * t + 1] * u[1];
}
'''


def test_drawn_normals_are_the_generators():
    """a cost that is one control of one step makes costs[b, s] = uhat + eps[s, t, r]: every draw of an N = 2, m = 2 problem"""
    import isls
    from isls import costs, models
    from mc_reference import normals
    N, S, sigma = 2, 200, np.array([[1.0, 0.5], [2.0, 1.5], [0.25, 3.0]])
    b, s = np.meshgrid(np.arange(B), np.arange(S), indexing="ij")
    for t in range(N):
        for c in range(2):
            q = isls.iSLS(2, 2, N, batch=B)
            q.forward_model = models.LTI(np.eye(2), np.eye(2))
            q.cost_function = costs.Custom(2, 2, np.eye(4)[2 * t + c], DRAW_COST)
            q.nominal_values = np.zeros((B, N, 2)), np.zeros((B, N, 2))
            r = q.sample_nominal(samples=S, sigma=sigma, seed=21, return_costs=True)
            ref = sigma[:, None, c] * normals(21, b, s, t, 2)[..., c]
            ref[:, 0] = 0.0
            assert np.max(np.abs(r.costs - ref)) < 1e-12


# ---- the updated plan ------------------------------------------------------------------------------------------------------------
# (kind, N, S, temperature, rounds, seed): the seeds were chosen with the reference alone so that, in every round and problem,
# the arg-min leads the runner-up and the decision of step 5 has a margin, both above 1e-6 relative -- asserted below
PLANS = [
    ("di63", 7, 200, 1.0, 2, 1),
    ("di63", 7, 65, 200.0, 1, 1),
    ("quad_bump", 7, 200, 0.01, 2, 1),
    ("car", 7, 64, 0.03, 1, 8),
]


@pytest.mark.parametrize("kind, N, S, temperature, rounds, seed", PLANS)
def test_updated_plan_matches_the_reference(kind, N, S, temperature, rounds, seed):
    p = make_ref(kind, N)
    ref = reference(p, seed=seed, samples=S, temperature=temperature, rounds=rounds)
    assert ref["lead"].min() > 1e-6 and ref["decide"].min() > 1e-6, (ref["lead"], ref["decide"])
    q = solver(p)
    r = q.sample_nominal(samples=S, sigma=p["sigma"], temperature=temperature, rounds=rounds, seed=seed)
    assert np.array_equal(r.took_best, ref["took_best"])
    assert rel(q.u_nom, ref["uhat"]) < 1e-9 and rel(q.x_nom, ref["xhat"]) < 1e-9
    assert rel(r.cost_after, ref["cost_after"]) < 1e-9 and rel(r.cost_before, ref["cost_before"]) < 1e-9
    assert rel(r.ess, ref["ess"]) < 1e-9 and rel(r.cost_best_sample, ref["cost_best_sample"]) < 1e-9
    assert rel(q.cost, r.cost_after) < 1e-12                   # the same terms, summed by the expansion in another order


def test_both_branches_of_the_selection_are_covered():
    took = [reference(make_ref(k, N), seed=sd, samples=S, temperature=T_, rounds=R_)["took_best"] for k, N, S, T_, R_, sd in PLANS]
    assert any(t.any() for t in took) and any((~t).any() for t in took)


# ---- invariants on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["di63", "quad_bump", "arm"])
def test_cost_never_rises_and_runs_repeat(kind):
    p = make_ref(kind, 7)
    out = []
    for _ in range(2):
        q = solver(p)
        r = q.sample_nominal(samples=200, sigma=p["sigma"], rounds=3, seed=2, return_costs=True)
        assert np.all(r.cost_after <= r.cost_before) and np.all(np.diff(r.cost_best_sample, axis=1) <= 0)
        out.append((q.x_nom, q.u_nom, r.costs, r.cost_after, r.ess, r.took_best, r.cost_best_sample))
    for a, b_ in zip(*out):
        assert np.array_equal(a, b_)


@pytest.mark.parametrize("kind", ["di63", "quad_bump"])
def test_one_sample_or_no_spread_keeps_the_nominal(kind):
    """bit for bit, from a nominal that is the device's own rollout of its controls (the first call makes it one)"""
    p = make_ref(kind, 7)
    q = solver(p)
    q.sample_nominal(samples=1)
    assert np.array_equal(q.u_nom, p["uhat"])
    x0, u0 = q.x_nom.copy(), q.u_nom.copy()
    for kw in (dict(samples=1, sigma=0.7), dict(samples=65, sigma=0.0), dict(samples=1, sigma=0.0, rounds=2)):
        r = q.sample_nominal(seed=4, **kw)
        assert np.array_equal(q.x_nom, x0) and np.array_equal(q.u_nom, u0)
        # the two kernels cost the same trajectory with the same sums, contracted as the compiler chose in each: a few ulps
        assert np.all(r.cost_after <= r.cost_before) and rel(r.cost_after, r.cost_before) < 1e-14


def test_inactive_problems_are_left_alone():
    p = make_ref("di63", 7)
    q = solver(p)
    e = q.engine
    x0, u0 = e.xhat.clone(), e.uhat.clone()
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=e.device)
    costs = torch.full((B, 65), -7.0, dtype=e.dtype, device=e.device)
    stats = {k: torch.full((B,), -7.0, dtype=e.dtype, device=e.device) for k in ("cost_before", "cost_after", "cost_best", "ess")}
    stats["took_best"] = torch.full((B,), -7, dtype=torch.int32, device=e.device)
    e.sample_round(e._t(np.full(3, 0.5)), costs, seed=5, active=active, **stats)
    assert torch.equal(e.xhat[1], x0[1]) and torch.equal(e.uhat[1], u0[1]) and bool((costs[1] == -7.0).all())
    assert all(float(v[1]) == -7 for v in stats.values())
    assert not torch.equal(e.uhat[0], u0[0]) and not torch.equal(e.uhat[2], u0[2])
    assert all(float(v[b]) != -7 for v in stats.values() for b in (0, 2))


def test_results_do_not_depend_on_the_batch():
    """problems [0, 1, 63, 64, 199] of a B = 200, S = 200 run (200 x 4 workgroups of the cost kernel) against a B = 5 run of the
    same problems gathered, problem_ids giving each its counter in the large batch -- and the pair [63, 64] with problem0"""
    idx = [0, 1, 63, 64, 199]
    p = make_ref("di63", 7, nb=200)
    q = solver(p)
    e = q.engine
    xs, us = e.xhat.clone(), e.uhat.clone()
    sigma = e._t(np.full(3, 0.5))
    r = q.sample_nominal(samples=200, sigma=0.5, seed=8, return_costs=True)
    sel = torch.tensor(idx, device=e.device)
    for rows, kw in ((sel, dict(problem_ids=sel.to(torch.int32))), (sel[2:4], dict(problem0=63))):
        nb, at = len(rows), rows.cpu().numpy()
        x, u = xs[rows].contiguous(), us[rows].contiguous()
        costs = torch.zeros(nb, 200, dtype=e.dtype, device=e.device)
        after, ess = (torch.zeros(nb, dtype=e.dtype, device=e.device) for _ in range(2))
        e.kern.sample_nominal(e.model, e.model_par, x, u, e.Qtab, e.ztab[rows].contiguous(), e.seq, e.u_std, sigma, costs, seed=8,
                              cost_after=after, ess=ess, stream=torch.cuda.current_stream().cuda_stream, **kw)
        assert np.array_equal(costs.cpu().numpy(), r.costs[at])
        assert torch.equal(x, e.xhat[rows]) and torch.equal(u, e.uhat[rows])
        assert np.array_equal(after.cpu().numpy(), r.cost_after[at]) and np.array_equal(ess.cpu().numpy(), r.ess[at, 0])


# ---- fp32, NaN, end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["di63", "car"])
def test_fp32_costs_are_as_good_as_numpy_float32(kind):
    """two roundings of the same sums, possibly in another order: the device's error against the fp64 reference is at most twice
    that of a float32 numpy evaluation of the same rollouts"""
    p = make_ref(kind, 7)
    q = solver(p, dtype=np.float32)
    r = q.sample_nominal(samples=200, sigma=p["sigma"], seed=6, return_costs=True)
    ref = reference(p, seed=6, samples=200)["costs"]
    ref32 = reference(p, seed=6, samples=200, dtype=np.float32)["costs"]
    dev_err, np_err = rel(r.costs, ref), rel(ref32, ref)
    print(f"{kind}: fp32 device costs rel {dev_err:.3e}, numpy float32 rel {np_err:.3e}")
    assert dev_err <= 2 * np_err


def test_nan_samples_get_no_weight():
    p = make_ref("sqrt", 7)
    ref = reference(p, seed=SEED_NAN, samples=200)
    nan = ~np.isfinite(ref["costs"])
    assert nan.any(axis=1).all() and not nan[:, 0].any()       # every problem has NaN samples; the nominal is finite
    assert ref["lead"].min() > 1e-6 and ref["decide"].min() > 1e-6
    q = solver(p)
    r = q.sample_nominal(samples=200, sigma=p["sigma"], seed=SEED_NAN, return_costs=True)
    assert rel_costs(r.costs, ref["costs"]) < 1e-9 and np.isfinite(r.cost_after).all()
    assert np.array_equal(r.took_best, ref["took_best"]) and rel(r.ess, ref["ess"]) < 1e-9
    assert rel(q.u_nom, ref["uhat"]) < 1e-9 and rel(q.x_nom, ref["xhat"]) < 1e-9 and rel(r.cost_after, ref["cost_after"]) < 1e-9


def test_a_nominal_without_a_finite_cost_raises():
    p = make_ref("sqrt", 7)
    p["xhat"] = p["xhat"].copy()
    p["xhat"][1, 0, 0] = -1.0                                   # problem 1 starts below zero: its own rollout is NaN
    q = solver(p)
    before = q.u_nom.copy()
    with pytest.raises(capi.IslsError, match=r"\[1\]"):
        q.sample_nominal(samples=65, sigma=0.1)
    assert np.array_equal(q.u_nom[1], before[1])


@pytest.mark.parametrize("kind", ["di63", "quad_bump"])
def test_solvers_run_on_the_warm_start(kind):
    from isls import Box
    p = make_ref(kind, 7)
    q = solver(p)
    r = q.sample_nominal(samples=200, sigma=p["sigma"], seed=1)
    assert rel(q.cost, r.cost_after) < 1e-12 and np.array_equal(q.status, np.zeros(B, dtype=np.int32))
    q.solve(max_iter=3)
    print(f"{kind}: status after solve(max_iter=3) {q.status}")
    # a trajectory that has converged ends with ISLS_ST_LS_REJECT: no candidate of its last line search costs less (the linear-
    # quadratic di63 converges in one iteration: seen [4, 4, 0]).  Every other bit -- Quu not PD, a NaN cost, the ladder's end -- is an error
    assert np.array_equal(q.status & ~capi.ST_LS_REJECT, np.zeros(B, dtype=np.int32)) and np.all(q.cost <= r.cost_after * (1 + 1e-12))
    q.sample_nominal(samples=64, sigma=p["sigma"], seed=2)
    lim = (0.0, 9.0) if kind.startswith("quad") else (-2.0, 2.0)
    q.ilqr_admm(project_u=Box(*lim), rho_u=0.1, max_iter=2, max_admm_iter=3)
    assert np.array_equal(q.status, np.zeros(B, dtype=np.int32)) and np.isfinite(q.cost).all()
