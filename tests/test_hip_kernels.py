"""GPU parity, kernel by kernel: every HIP kernel (through the C ABI) against the CPU oracle on identical
seeded inputs, for the four systems of the BASELINE configs.  Tolerance: 1e-10 (fp64) on max-abs error
relative to max(1,|ref|_max) per array; the ill-conditioned arm problem uses the conditioning-aware bound
recorded in its golden file (see tests/test_oracle_golden.py::trace_tols)."""
import numpy as np
import pytest

import isls_problems as P
from helpers import ALPHAS as ALPHAS_
from helpers import OracleDriver, problem_arrays
from isls import _capi as capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dual(oracle):
    from dual import DualKernels, hip_kernels
    return lambda tol=1e-10, ff_nseg=1, ff_record=False, ti_weights=False, ff_lin=False: DualKernels(
        oracle, hip_kernels(), tol=tol, ff_nseg=ff_nseg, ff_record=ff_record, ti_weights=ti_weights, ff_lin=ff_lin)


def _report(dk):
    worst = sorted(dk.max_err.items(), key=lambda kv: -kv[1])[:6]
    print("calls", dk.calls, "worst:", ", ".join(f"{k}={v:.1e}" for k, v in worst))
    worst = sorted(dk.max_err_traj.items(), key=lambda kv: -kv[1])[:6]
    print("  per trajectory:", ", ".join(f"{k}={v:.1e}" for k, v in worst))


@pytest.mark.parametrize("B,ff_nseg", [(1, 1), (7, 1), (23, 1), (7, 4), (23, 5)])
def test_di3d_all_kernels(dual, B, ff_nseg):
    cfg = P.config2(batch=32, N=100, seed=1)
    pa = problem_arrays(cfg, range(B))
    dk = dual(ff_nseg=ff_nseg)
    d = OracleDriver(dk, pa, rho_u=cfg["rho_u"], relax=cfg["relax"])
    d.run(2, 20, 3, 0.0)
    # state box + relaxation + natural stop (freezing of converged trajectories)
    pa["x_lo"] = np.full((100, 6), -np.inf); pa["x_hi"] = np.full((100, 6), np.inf)
    pa["x_lo"][:, 3:6], pa["x_hi"][:, 3:6] = -1.2, 1.2
    d = OracleDriver(dk, pa, rho_x=0.05, rho_u=cfg["rho_u"], project_x=True, relax=1.5)
    d.run(4, 20, 10, 1e-3)
    _report(dk)


def test_di3d_iterate_once_flags(dual):
    cfg = P.config2(batch=16, N=100, seed=2)
    pa = problem_arrays(cfg, range(9))
    dk = dual()
    d = OracleDriver(dk, pa, project_u=False)
    for it in range(3):
        # LQ problem: the first Newton step lands on the optimum, afterwards k ~ 0 and the candidates tie
        # to rounding: the arg-min index / accept bit are then not determined at 1e-16, only the values are
        dk.int_exact = it == 0
        d.linearize_expand()
        d.gain(), d.ff()
        d.rollout(20, flags=capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST, cost_all=np.zeros((9, 20)))
        d.xhat[:], d.uhat[:], d.cost[:] = d.xx, d.xu, d.cost_new
    # forced rejection: no candidate can beat a current cost of -1 -> the nominal must be kept bit-exactly
    d.cost[:] = -1.0
    d.status[:] = 0
    d.linearize_expand()
    d.gain(), d.ff()
    d.rollout(5, flags=capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST)
    assert (d.status & capi.ST_LS_REJECT).all() and np.array_equal(d.xx, d.xhat) and np.array_equal(d.xu, d.uhat)
    _report(dk)


@pytest.mark.parametrize("L", [1, 5, 8, 20, 33, 50])
def test_rollout_candidate_counts(dual, L):
    cfg = P.config2(batch=16, N=100, seed=3)
    pa = problem_arrays(cfg, range(11))
    dk = dual()
    d = OracleDriver(dk, pa, rho_u=cfg["rho_u"])
    d.linearize_expand()
    d.gain(), d.ff()
    d.rollout(L, cost_all=np.zeros((11, L)))
    _report(dk)


def test_double_integrator_model_equals_dense_lti(oracle):
    """ISLS_MODEL_DI (Kronecker-structured evaluation) on the GPU against the dense LTI map of the oracle."""
    import torch
    from dual import hip_kernels
    from isls import models
    cfg = P.config2(batch=16, N=100, seed=5)
    pa = problem_arrays(cfg, range(13))
    d = OracleDriver(oracle, pa, rho_u=cfg["rho_u"])
    d.linearize_expand()
    d.gain(), d.ff()
    cost_all = np.zeros((13, 20))
    d.rollout(20, cost_all=cost_all)                          # oracle, dense LTI
    mdl = models.LTI(cfg["A"], cfg["B"])
    assert mdl.model_id == capi.MODEL_DI
    hip = hip_kernels()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    xx, xu, ca, cn, best = dev(np.zeros_like(d.xx)), dev(np.zeros_like(d.xu)), dev(np.zeros((13, 20))), dev(np.zeros(13)), dev(np.zeros(13, dtype=np.int32))
    hip.rollout_ls(mdl.model_id, dev(mdl.params()), dev(d.K), dev(d.k), dev(d.xhat), dev(d.uhat), dev(ALPHAS_[:20]),
                   dev(pa["Qtab"]), dev(pa["ztab"]), dev(pa["seq"]), pa["u_std"], xx, xu, best=best, cost_new=cn, cost_all=ca,
                   wr=dev(d.wr), zu=dev(d.zu), lu=dev(d.lu), cost_cur=dev(d.cost))
    torch.cuda.synchronize()
    assert np.max(np.abs(ca.cpu().numpy() - cost_all)) / max(1.0, np.abs(cost_all).max()) < 1e-12
    assert np.array_equal(best.cpu().numpy(), d.best)
    assert np.max(np.abs(xx.cpu().numpy() - d.xx)) < 1e-12 and np.max(np.abs(xu.cpu().numpy() - d.xu)) < 1e-12
    # linearisation of the structured model reproduces the dense A, B
    A, Bm = dev(np.zeros_like(d.A)), dev(np.zeros_like(d.Bm))
    hip.linearize(mdl.model_id, dev(mdl.params()), dev(d.xhat), dev(d.uhat), A, Bm)
    torch.cuda.synchronize()
    assert np.array_equal(A.cpu().numpy(), d.A) and np.array_equal(Bm.cpu().numpy(), d.Bm)


@pytest.mark.parametrize("ff_nseg", [1, 4])
def test_arm_all_kernels(dual, golden, ff_nseg):
    g = golden("g4_arm3r.npz")
    sens = max(float(v) for v in g["o2_sens"])
    cfg = P.config3(batch=16, N=100, seed=0)
    pa = problem_arrays(cfg, range(7))
    dk = dual(tol=max(1e-10, 10 * sens), ff_nseg=ff_nseg)
    d = OracleDriver(dk, pa, rho_x=cfg["rho_x"], rho_u=cfg["rho_u"], project_x=True)
    d.run(3, cfg["max_line_search"], cfg["max_admm_iter"], 0.0)
    _report(dk)


@pytest.mark.parametrize("ff_nseg", [1, 8])
def test_car_all_kernels(dual, ff_nseg):
    cfg = P.config4(batch=16, N=200, seed=0)
    pa = problem_arrays(cfg, range(13))
    dk = dual(ff_nseg=ff_nseg)
    d = OracleDriver(dk, pa, rho_x=cfg["rho_x"], rho_u=cfg["rho_u"], project_x=True)
    d.run(3, 20, cfg["max_admm_iter"], 0.0)
    _report(dk)


def test_di1d_sls_inverse_mode(dual):
    """SLS.solve_dp / solve_dp_ff / get_trajectory_dp path (explicit inverse, absolute coordinates)."""
    from helpers import rho_to_weights
    c = P.config1(50)
    N, n, m, B = 50, 2, 1, 3
    dk = dual()
    z = lambda *s: np.zeros(s)   # noqa: E731
    Rr = rho_to_weights(c["rho_u"], N, m)
    Qr = rho_to_weights(0.5, N, n)
    Cxx, Cuu, c0x, c0u = z(B, N, n, n), z(B, N, m, m), z(B, N, n), z(B, N, m)
    dk.expand_quadratic(c["Qs"], c["zs"], c["seq"], c["u_std"], c0x, c0u, Cxx=Cxx, Cuu=Cuu, Qr=Qr, Rr=Rr)
    K, Quu, fac, Qux, k = z(B, N, m, n), z(B, N, m, m), z(B, N, m, m), z(B, N, m, n), z(B, N, m)
    st = np.zeros(B, dtype=np.int32)
    dk.riccati_gain(c["A"], c["B"], Cxx, Cuu, K, Quu, fac, Qux, solve_mode=capi.SOLVE_INV, status=st)
    rng = np.random.default_rng(0)
    zx, zu = rng.standard_normal((B, N, n)), rng.standard_normal((B, N, m))
    lx, lu = 0.1 * rng.standard_normal((B, N, n)), 0.1 * rng.standard_normal((B, N, m))
    dk.riccati_ff(c["A"], c["B"], c0x, c0u, K, Quu, fac, Qux, k, Qr=Qr, Rr=Rr, zx=zx, lx=lx, zu=zu, lu=lu,
                  solve_mode=capi.SOLVE_INV)
    par = np.concatenate([c["A"].ravel(), c["B"].ravel()])
    xx, xu = z(B, N, n), z(B, N, m)
    x0 = rng.standard_normal((B, n)) * 0.1
    dk.rollout_ls(capi.MODEL_LTI, par, K, k, z(B, N, n), z(B, N, m), np.ones(1), c["Qs"], c["zs"], c["seq"],
                  c["u_std"], xx, xu, x0=x0, flags=capi.RO_ABSOLUTE, cost_new=z(B), best=np.zeros(B, dtype=np.int32))
    _report(dk)


@pytest.mark.parametrize("N,nseg", [(2, 4), (3, 2), (4, 3), (10, 4), (33, 16), (100, 3), (100, 7)])
def test_time_parallel_feedforward(dual, N, nseg):
    """isls_ffseg: segmented recursion + stitch against the oracle's sequential feed-forward pass, over horizon /
    segment-count pairs with ragged last segments, frozen trajectories and both solve modes."""
    cfg = P.config2(batch=16, N=N, seed=5)
    pa = problem_arrays(cfg, range(11))
    for mode in (capi.SOLVE_CHOL, capi.SOLVE_INV):
        dk = dual(ff_nseg=nseg)
        d = OracleDriver(dk, pa, rho_x=0.05, rho_u=cfg["rho_u"], project_x=True)
        d.linearize_expand()
        d.admm_active[[2, 5]] = 0
        rng = np.random.default_rng(N)
        for arr in (d.zx, d.zu, d.lx, d.lu):
            arr[:] = 0.3 * rng.standard_normal(arr.shape)
        dk.riccati_gain(d.A, d.Bm, d.Cxx, d.Cuu, d.K, d.Quu, d.fac, d.Qux, solve_mode=mode, status=d.status,
                        active=d.admm_active)
        d.k[:] = 7.0                                            # frozen trajectories must keep this
        dk.riccati_ff(d.A, d.Bm, d.c0x, d.c0u, d.K, d.Quu, d.fac, d.Qux, d.k, Qr=d.Qr, Rr=d.Rr, xhat=d.xhat,
                      uhat=d.uhat, zx=d.zx, lx=d.lx, zu=d.zu, lu=d.lu, solve_mode=mode, active=d.admm_active)
        assert np.all(d.k[[2, 5]] == 7.0)
    _report(dk)


@pytest.mark.parametrize("which,ff_nseg", [("di3d", 1), ("di3d", 3), ("car", 1), ("car", 4), ("arm", 1), ("arm", 3), ("di1d", 2)])
def test_feedforward_on_packed_records(dual, golden, which, ff_nseg):
    """isls_gain_args.rec / isls_ff_args.rec: the gain pass writes [A + B K | B | K | fac] per step and the feed-forward
    passes evaluate v = cx + K'cu + (A + B K)'v, k = -Quu^-1 (cu + B'v) from those records -- against the oracle's
    four-term recursion of the reference (isls.py:285-302), whole ADMM traces, sequential and time-parallel, both solve
    modes (di1d: the SLS inverse mode), frozen trajectories included."""
    if which == "di1d":                                         # SLS layout: shared LTI A, B (stride-0 views), absolute coordinates
        from helpers import rho_to_weights
        c = P.config1(50)
        N, n, m, B = 50, 2, 1, 3
        z = lambda *s_: np.zeros(s_)   # noqa: E731
        Rr, Qr = rho_to_weights(c["rho_u"], N, m), rho_to_weights(0.5, N, n)
        rng = np.random.default_rng(0)
        zx, zu = rng.standard_normal((B, N, n)), rng.standard_normal((B, N, m))
        lx, lu = 0.1 * rng.standard_normal((B, N, n)), 0.1 * rng.standard_normal((B, N, m))
        for mode in (capi.SOLVE_CHOL, capi.SOLVE_INV):
            dk = dual(ff_nseg=ff_nseg, ff_record=True)
            Cxx, Cuu, c0x, c0u = z(B, N, n, n), z(B, N, m, m), z(B, N, n), z(B, N, m)
            dk.expand_quadratic(c["Qs"], c["zs"], c["seq"], c["u_std"], c0x, c0u, Cxx=Cxx, Cuu=Cuu, Qr=Qr, Rr=Rr)
            K, Quu, fac, Qux, k = z(B, N, m, n), z(B, N, m, m), z(B, N, m, m), z(B, N, m, n), z(B, N, m)
            dk.riccati_gain(c["A"], c["B"], Cxx, Cuu, K, Quu, fac, Qux, solve_mode=mode, status=np.zeros(B, dtype=np.int32))
            dk.riccati_ff(c["A"], c["B"], c0x, c0u, K, Quu, fac, Qux, k, Qr=Qr, Rr=Rr, zx=zx, lx=lx, zu=zu, lu=lu, solve_mode=mode)
            assert dk._rec is not None
        _report(dk)
        return
    tol = 1e-10
    if which == "di3d":
        cfg = P.config2(batch=32, N=100, seed=1)
        kw = dict(rho_x=0.05, rho_u=cfg["rho_u"], project_x=True, relax=1.5)
        pa = problem_arrays(cfg, range(13))
        pa["x_lo"] = np.full((100, 6), -np.inf); pa["x_hi"] = np.full((100, 6), np.inf)
        pa["x_lo"][:, 3:6], pa["x_hi"][:, 3:6] = -1.2, 1.2
    elif which == "car":
        cfg = P.config4(batch=8, N=200, seed=0)
        kw = dict(rho_u=cfg["rho_u"])
        pa = problem_arrays(cfg, range(5))
    else:
        cfg = P.config3(batch=2, N=100, seed=0)
        g = golden("g4_arm3r.npz")
        tol = max(1e-10, 10 * float(np.max(g["o2_sens"])))        # conditioning-aware bound of the arm (see module docstring)
        kw = dict(rho_x=cfg["rho_x"], rho_u=cfg["rho_u"], project_x=True)
        pa = problem_arrays(cfg, range(2))
    dk = dual(tol=tol, ff_nseg=ff_nseg, ff_record=True)
    d = OracleDriver(dk, pa, **kw)
    d.run(3, 10, 4, 1e-3 if which == "di3d" else 0.0)
    assert dk._rec is not None
    _report(dk)


@pytest.mark.parametrize("ff_record,ff_nseg", [(False, 1), (True, 1), (True, 3)])
def test_fp32_kernels(dual, ff_record, ff_nseg):
    """fp32 build of every kernel against the fp32 oracle (north star: 1e-4 fp32); the feed-forward pass in its array form
    and on the packed records of the gain pass, sequential and time-parallel."""
    cfg = P.config2(batch=16, N=100, seed=4)
    pa = problem_arrays(cfg, range(10), dtype=np.float32)
    dk = dual(tol=1e-4, ff_record=ff_record, ff_nseg=ff_nseg)
    dk.int_exact = False            # near-ties of the arg-min may flip in fp32
    d = OracleDriver(dk, pa, rho_u=cfg["rho_u"], relax=cfg["relax"], dtype=np.float32)
    d.run(2, 20, 3, 0.0)
    _report(dk)


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-10), ("f32", 1e-4)])
@pytest.mark.parametrize("ff_nseg", [1, 3])
@pytest.mark.parametrize("which", ["di3d_u", "di3d_xu", "car"])
def test_one_handoff_feedforward_on_time_invariant_weights(dual, which, ff_nseg, dtype, tol):
    """riccati_ffrec2_kernel -- the feed-forward pass the headline workload runs: packed records AND time-invariant ADMM
    weights handed over as one [1,d,d] block (time stride 0), as isls.Engine does.  Kernel call by kernel call against the
    oracle's four-term recursion on the tiled weights, sequential (ff_nseg = 1) and time-parallel (prepare + segments +
    stitch), fp64 at 1e-10 and fp32 at the north star's 1e-4; the rollout reads its AL weights from the same one block."""
    f = np.float64 if dtype == "f64" else np.float32
    if which == "car":
        cfg = P.config4(batch=8, N=200, seed=0)
        pa, kw = problem_arrays(cfg, range(6), dtype=f), dict(rho_u=cfg["rho_u"])
    else:
        cfg = P.config2(batch=32, N=100, seed=5)
        pa, kw = problem_arrays(cfg, range(11), dtype=f), dict(rho_u=cfg["rho_u"], relax=cfg["relax"])
        if which == "di3d_xu":
            pa["x_lo"] = np.full((100, 6), -np.inf, dtype=f); pa["x_hi"] = np.full((100, 6), np.inf, dtype=f)
            pa["x_lo"][:, 3:6], pa["x_hi"][:, 3:6] = -1.2, 1.2
            kw = dict(rho_x=0.05, rho_u=cfg["rho_u"], project_x=True, relax=1.5)
    dk = dual(tol=tol, ff_nseg=ff_nseg, ff_record=True, ti_weights=True)
    dk.int_exact = dtype == "f64"                                  # near-ties of the arg-min may flip in fp32
    d = OracleDriver(dk, pa, dtype=f, **kw)
    d.run(2, 20, 4, 0.0)
    assert dk._rec is not None
    _report(dk)


def _di_config(dim, batch, N, seed):
    """config2's problem for a double integrator of another dimension (n = 2 dim, m = dim)"""
    rng = np.random.default_rng(seed)
    n, m, dt = 2 * dim, dim, 0.01
    A, B = P.double_integrator_AB(dim, 2, dt)
    x0, target = np.zeros((batch, n)), np.zeros((batch, n))
    x0[:, :dim] = rng.uniform(-0.5, 0.5, size=(batch, dim))
    target[:, :dim] = rng.uniform(0.5, 1.5, size=(batch, dim))
    zs = np.zeros((batch, 2, n))
    zs[:, 1] = target
    seq = np.zeros(N, dtype=np.int32)
    seq[N - 1] = 1
    return dict(name=f"di{dim}d", n=n, m=m, N=N, dt=dt, A=A, B=B, zs=zs, Qs=np.stack([np.zeros((n, n)), 1e3 * np.eye(n)]), seq=seq,
                u_std=1e-3, x0=x0, u0=np.zeros((batch, N, m)), u_lo=-3.0, u_hi=3.0, rho_u=1e-2, relax=1.0, model=P.MODEL_LTI)


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-10), ("f32", 1e-4)])
@pytest.mark.parametrize("which", ["di1d", "di2d", "di3d_u", "di3d_xu", "arm", "car"])
def test_model_structured_feedforward(dual, golden, which, dtype, tol, ff_nseg=1):
    """isls_gain_args.lin_on / isls_ff_args.lin_on: the gain pass writes the lean records [K | fac | model words] and the record
    pass evaluates (A + B K)'v = A'v + K'(B'v) from the structure of the model whose linearisation A, B are -- double integrators
    of dimension 1, 2, 3 (ISLS_MODEL_DI), the planar arm (ISLS_MODEL_ARM3R, J behind fac) and the car (ISLS_MODEL_CAR, its six
    varying entries behind fac) -- against the oracle's four-term
    recursion on the dense arrays, whole ADMM traces kernel call by kernel call, batch sizes that leave wavefront slots empty,
    both precisions (the arm in fp64 and fp32 at its conditioning-aware bounds, as in the dense-form tests).  Sequential form
    only: the time-parallel one needs the dense records (test_structured_hint_is_refused_where_it_cannot_apply)."""
    f = np.float64 if dtype == "f64" else np.float32
    if which == "arm":
        g = golden("g4_arm3r.npz")
        cfg = P.config3(batch=8, N=100, seed=0)
        amp = max(float(v) for v in g["o2_sens"]) / 1e-15
        tol = max(1e-10, 10 * float(np.max(g["o2_sens"]))) if dtype == "f64" else max(1e-4, 10 * amp * 2.0 ** -24)
        pa, kw = problem_arrays(cfg, range(7), dtype=f), dict(rho_x=cfg["rho_x"], rho_u=cfg["rho_u"], project_x=True)
        steps = (2, cfg["max_line_search"], 4)
    elif which == "car":                                           # ISLS_MODEL_CAR: the six varying entries of A, B behind fac, N = 200
        cfg = P.config4(batch=16, N=200, seed=0)
        pa, kw = problem_arrays(cfg, range(13), dtype=f), dict(rho_x=cfg["rho_x"], rho_u=cfg["rho_u"], project_x=True)
        steps = (2, 20, 3)
    else:
        dim = {"di1d": 1, "di2d": 2}.get(which, 3)
        cfg = _di_config(dim, batch=40, N=100, seed=5)
        nb = {1: 23, 2: 13, 3: 11}[dim]                            # 21 / 10 / 7 trajectories per wavefront: a partly filled last one
        pa, kw = problem_arrays(cfg, range(nb), dtype=f), dict(rho_u=cfg["rho_u"], relax=cfg["relax"])
        if which == "di3d_xu":
            pa["x_lo"] = np.full((100, 6), -np.inf, dtype=f); pa["x_hi"] = np.full((100, 6), np.inf, dtype=f)
            pa["x_lo"][:, 3:6], pa["x_hi"][:, 3:6] = -1.2, 1.2
            kw = dict(rho_x=0.05, rho_u=cfg["rho_u"], project_x=True, relax=1.5)
        steps = (2, 20, 4)
    dk = dual(tol=tol, ff_nseg=ff_nseg, ff_record=True, ti_weights=True, ff_lin=True)
    dk.int_exact = dtype == "f64" and which not in ("arm", "car")  # near-ties of the arg-min may flip in fp32 / on the arm / the car
    d = OracleDriver(dk, pa, dtype=f, **kw)
    d.run(*steps, 0.0)
    assert dk._rec is not None and dk.lin_calls >= steps[0] * steps[2]   # the structured form really ran
    _report(dk)


def test_structured_hint_is_refused_where_it_cannot_apply():
    """The hint selects the lean record layout, so a pass that cannot honour it must fail instead of falling back: a gain pass
    asked for the Quu / fac / Qux arrays, a feed-forward pass with time-varying weights or with time-parallel segments, the
    fused entry with one block hinted and the other not, a model the passes do not know, the array form."""
    import torch
    from dual import hip_kernels
    from isls import models
    hk = hip_kernels()
    B, N, n, m = 5, 12, 6, 3
    A1, B1 = P.double_integrator_AB(3, 2, 0.01)
    par = torch.as_tensor(np.asarray(models.LTI(A1, B1).params())).cuda()
    z = lambda *s_: torch.zeros(*s_, dtype=torch.float64, device="cuda")   # noqa: E731
    A, Bm = z(B, N, n, n), z(B, N, n, m)
    hk.linearize(capi.MODEL_DI, par, z(B, N, n), z(B, N, m), A, Bm)
    Cxx, Cuu = torch.eye(n, dtype=torch.float64, device="cuda").expand(B, N, n, n).contiguous(), torch.eye(m, dtype=torch.float64, device="cuda").expand(B, N, m, m).contiguous()
    K, k, st = z(B, N, m, n), z(B, N, m), torch.zeros(B, dtype=torch.int32, device="cuda")
    rec = z(capi.ff_record_elems(B, N, n, m))
    lin = (capi.MODEL_DI, par)
    G, F = capi.Kernels.gain_args, capi.Kernels.ff_args
    ok_gain = G(A, Bm, Cxx, Cuu, K, None, None, None, status=st, rec=rec, lin=lin)
    hk._call("riccati_gain", "f64", ok_gain, None)                 # the valid form runs
    Rr1, RrN = 0.1 * torch.eye(m, dtype=torch.float64, device="cuda")[None], (0.1 * torch.eye(m, dtype=torch.float64, device="cuda")).expand(N, m, m).contiguous()
    zu, lu, uh, xh = z(B, N, m), z(B, N, m), z(B, N, m), z(B, N, n)
    ff_ok = F(A, Bm, z(B, N, n), z(B, N, m), K, None, None, None, k, Rr=Rr1, xhat=xh, uhat=uh, zu=zu, lu=lu, rec=rec, lin=lin)
    hk._call("riccati_ff", "f64", ff_ok, None)
    torch.cuda.synchronize()
    with pytest.raises(capi.IslsError):                            # arrays requested: the dense form would be needed
        hk._call("riccati_gain", "f64", G(A, Bm, Cxx, Cuu, K, z(B, N, m, m), z(B, N, m, m), z(B, N, m, n), status=st, rec=rec, lin=lin), None)
    with pytest.raises(capi.IslsError):                            # time-varying weights: not the one-hand-off kernel
        hk._call("riccati_ff", "f64", F(A, Bm, z(B, N, n), z(B, N, m), K, None, None, None, k, Rr=RrN, xhat=xh, uhat=uh, zu=zu, lu=lu, rec=rec, lin=lin), None)
    nseg, seg_len = hk.ff_segments(N, 3)
    seg = capi.Kernels.ff_seg(z(B, N, m, n), z(B, nseg, n, n), z(B, nseg, n), seg_len)
    with pytest.raises(capi.IslsError):                            # segments: their operators come from the dense records
        hk._call("riccati_ff", "f64", F(A, Bm, z(B, N, n), z(B, N, m), K, None, None, None, k, Rr=Rr1, xhat=xh, uhat=uh, zu=zu, lu=lu, rec=rec, lin=lin, seg=seg), None)
    with pytest.raises(capi.IslsError):                            # writer hinted, reader not
        hk.riccati_gain_ff(ok_gain, F(A, Bm, z(B, N, n), z(B, N, m), K, None, None, None, k, Rr=Rr1, xhat=xh, uhat=uh, zu=zu, lu=lu, rec=rec), "f64")
    with pytest.raises(capi.IslsError):                            # a model whose structure the passes do not know
        hk._call("riccati_gain", "f64", G(A, Bm, Cxx, Cuu, K, None, None, None, status=st, rec=rec, lin=(capi.MODEL_CAR, par)), None)
    with pytest.raises(ValueError):                                # the hint describes records: not the array form
        F(A, Bm, z(B, N, n), z(B, N, m), K, z(B, N, m, m), z(B, N, m, m), z(B, N, m, n), k, lin=lin)
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["arm", "car", "tassa"])
def test_fp32_kernels_nonlinear_models(dual, golden, which):
    """fp32 build of every kernel on the 3R arm (state + control boxes), the car (N = 200) and the Tassa car (pseudo-Huber
    cost) against the fp32 oracle on identical inputs, kernel call by kernel call.  Tolerance: the north star's 1e-4, except
    where the problem's own conditioning amplifies the last fp32 bit beyond that -- the arm carries weights of 1e6 next
    to 1e-4 (its fp64 trace already moves by 8e-9 under 1e-15 perturbations, golden o2_sens): the same amplification of
    fp32 rounding (6e-8) gives the bound used here."""
    from helpers import tassa_arrays
    f32 = np.float32
    if which == "arm":
        g = golden("g4_arm3r.npz")
        amp = max(float(v) for v in g["o2_sens"]) / 1e-15            # measured amplification of a relative input perturbation
        cfg = P.config3(batch=16, N=100, seed=0)
        dk = dual(tol=max(1e-4, 10 * amp * 2.0 ** -24), ff_nseg=3, ff_record=True)
        dk.int_exact = False
        d = OracleDriver(dk, problem_arrays(cfg, range(5), dtype=f32), rho_x=cfg["rho_x"], rho_u=cfg["rho_u"], project_x=True, dtype=f32)
        d.run(2, cfg["max_line_search"], 4, 0.0)
    elif which == "car":
        cfg = P.config4(batch=16, N=200, seed=0)
        dk = dual(tol=1e-4, ff_nseg=4, ff_record=True)
        dk.int_exact = False
        d = OracleDriver(dk, problem_arrays(cfg, range(6), dtype=f32), rho_x=cfg["rho_x"], rho_u=cfg["rho_u"], project_x=True, dtype=f32)
        d.run(2, 20, 3, 0.0)
    else:
        g = golden("g8_tassa.npz")
        dk = dual(tol=1e-4, ff_nseg=3)
        dk.int_exact = False
        d = OracleDriver(dk, tassa_arrays(g, [0, 1], dtype=f32), rho_u=np.diag([1e-1, 1e-2]), dtype=f32)
        d.run(2, 40, 3, 0.0)
    _report(dk)


def test_car_state_constraint_kernels(dual):
    """ISLS_PROJ_SETS inside the ADMM update (argument kernel + project_rows + update) on the car, kernel by kernel."""
    import sys
    pj = sys.modules["isls.projections"]
    cfg = P.config4(batch=16, N=200, seed=0)
    rho_x = np.zeros((200, 4, 4)); rho_x[:, :2, :2] = 0.1 * np.eye(2)
    cs = pj.keepout_rectangles(4, [[-7.0, -3.0], [-3.0, -7.0]], [[2.0, 1.0], [2.0, 1.0]], -np.pi / 4)
    dk = dual(ff_nseg=4)
    d = OracleDriver(dk, problem_arrays(cfg, range(5)), rho_x=rho_x, project_x=True, project_u=False, x_sets=cs)
    d.run(2, 20, 4, 0.0)
    _report(dk)


def _car_keepout_sets(dtype=np.float64):
    """The two rotated keep-out rectangles of notebooks/Car/Iterative LQR with state constraints.ipynb cell 18 as
    ISLS_SET_SQUARE parameter blocks acting on the position block of a 4-vector (A = I4, b = 0)."""
    a_safe = np.array([[2.5, 1.5], [2.5, 1.5]])
    al = -np.pi / 4
    Rm = np.array([[np.cos(al), -np.sin(al)], [np.sin(al), np.cos(al)]])
    centres = np.array([[-7.0, -3.0], [-3.0, -7.0]])
    sets = []
    for i in range(2):
        W = np.diag(a_safe[i, 0] / a_safe[i]) @ Rm.T
        par = np.concatenate([[2, a_safe[i, 0] / 2, 1e5], centres[i], W.ravel(), np.linalg.inv(W).ravel()]).astype(dtype)
        sets.append(dict(kind=capi.SET_SQUARE, dim=4, A=np.eye(4, dtype=dtype), b=np.zeros(4, dtype=dtype), par=par))
    return sets


def _dual_project(oracle, y, sets, **kw):
    import torch
    from dual import hip_kernels
    hip = hip_kernels()
    P = y.shape[0]
    out_o, it_o = np.zeros_like(y), np.zeros(P, dtype=np.int32)
    oracle.project_rows(y, out_o, sets, iters=it_o, **kw)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    dsets = [{k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in sets]
    yd, od, itd = dev(y), dev(np.zeros_like(y)), dev(np.zeros(P, dtype=np.int32))
    dkw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    hip.project_rows(yd, od, dsets, iters=itd, **dkw)
    torch.cuda.synchronize()
    return out_o, it_o, od.cpu().numpy(), itd.cpu().numpy()


def test_projection_kernels(oracle, golden):
    """isls_project_rows on the device against the oracle: direct primitives, the SOC chance-constraint rows with
    per-problem operands, the car's keep-out rectangles on a coordinate block of strided rows, R > 64 rows."""
    g = golden("g6_projections.npz")
    rng = np.random.default_rng(7)
    # direct primitives (bit-exact: same operations in the same order)
    soc = np.ascontiguousarray(np.stack([g["soc_in"], 0.3 * g["soc_in"]]))
    o, _, h, _ = _dual_project(oracle, soc, [dict(kind=capi.SET_SOC_UNIT, dim=4)])
    assert np.max(np.abs(o - h)) < 1e-15
    sq = rng.standard_normal((3, 130, 2)) * 2
    par = np.concatenate([[2, 1.0, 2.5], [0.2, -0.1], np.eye(2).ravel(), np.eye(2).ravel()])
    o, _, h, _ = _dual_project(oracle, sq, [dict(kind=capi.SET_SQUARE, dim=2, par=par)])
    assert np.max(np.abs(o - h)) < 1e-15
    qd = np.ascontiguousarray(np.stack([g["quad_in"], 2.0 * g["quad_in"]]))
    o, _, h, _ = _dual_project(oracle, qd, [dict(kind=capi.SET_QUADRATIC, dim=3, par=np.array([0.5, 3.0]))])
    assert np.max(np.abs(o - h)) < 1e-14
    lin = np.ascontiguousarray(g["lin_in"][:, None, :])
    par = np.ascontiguousarray(np.concatenate([np.tile([-0.5, 1.0], (50, 1)), g["lin_a"]], axis=1))
    o, _, h, _ = _dual_project(oracle, lin, [dict(kind=capi.SET_LINEAR, dim=3, par=par)])
    assert np.max(np.abs(o - h)) < 1e-14 and np.allclose(h[:, 0], g["lin_out"], atol=1e-13)
    # chance-constraint rows: two SOC images, A_i, b_i differ per problem (variance / bound per problem)
    P, R = 9, 50
    A0 = np.tile(g["setcvx_A0"][None], (P, 1, 1)) * (1 + 0.2 * rng.random((P, 1, 1)))
    A1 = np.tile(g["setcvx_A1"][None], (P, 1, 1)) * (1 + 0.2 * rng.random((P, 1, 1)))
    b0 = np.tile(g["setcvx_b0"][None], (P, 1)) * (1 + 0.3 * rng.random((P, 1)))
    b1 = np.tile(g["setcvx_b1"][None], (P, 1)) * (1 + 0.3 * rng.random((P, 1)))
    sets = [dict(kind=capi.SET_SOC_UNIT, dim=3, A=A0, b=b0), dict(kind=capi.SET_SOC_UNIT, dim=3, A=A1, b=b1)]
    y = rng.standard_normal((P, R, 2)) * np.array([6.0, 30.0])
    act = np.ones(P, dtype=np.int32); act[4] = 0
    o, io, h, ih = _dual_project(oracle, y, sets, rho=10.0, max_iter=100, threshold=1e-3, active=act)
    assert np.array_equal(io, ih) and np.max(np.abs(o - h)) < 1e-10 and np.all(h[4] == 0)
    # keep-out rectangles on the position block of [B, N, 4] state rows, N = 200 rows per problem
    sets = _car_keepout_sets()
    x = rng.standard_normal((5, 200, 4)) * np.array([3.0, 3.0, 1.0, 1.0]) + np.array([-5.0, -5.0, 0, 0])
    o, io, h, ih = _dual_project(oracle, x, sets, rho=10.0, max_iter=15, threshold=1e-3)
    assert np.array_equal(io, ih) and np.max(np.abs(o - h)) < 1e-10
    assert np.max(np.abs(o[..., 2:] - x[..., 2:])) < 1e-12                 # heading / speed untouched
    # fp32
    o, io, h, ih = _dual_project(oracle, x.astype(np.float32), _car_keepout_sets(np.float32), rho=10.0, max_iter=15, threshold=1e-3)
    assert np.max(np.abs(o - h)) < 1e-4


def test_projection_kernels_shells_dykstra_soc_multilinear(oracle, golden):
    """SURVEY 8f-4 on the device: ISLS_SET_SHELL through project_set_convex and through Dykstra (ISLS_PROJ_ALG_DYKSTRA), the
    two chained as the obstacle notebook does (`next`), project_soc with a general affine image (ISLS_PROJ_ALG_SOC),
    project_multilinear (ISLS_SET_MULTILINEAR) and row masks -- against the oracle (same iteration counts, 1e-12) and against
    the outputs of the reference's own functions (golden G6, 1e-10); fp32 against the fp32 oracle at 1e-4."""
    import torch
    from dual import hip_kernels
    g = golden("g6_projections.npz")
    rng = np.random.default_rng(3)
    P_ = 5
    pts = np.ascontiguousarray(np.concatenate([g["shell_in"][None], rng.uniform(0.0, 1.0, size=(P_ - 1, 60, 2))]))

    def shell(dtype=np.float64):
        return [dict(kind=capi.SET_SHELL, dim=2, A=np.eye(2, dtype=dtype), b=np.zeros(2, dtype=dtype),
                     par=np.concatenate([[lo, 1e2], c]).astype(dtype)) for lo, c in zip(g["shell_lowers"], g["shell_centres"])]
    o, io, h, ih = _dual_project(oracle, pts, shell(), rho=1.0, max_iter=5, threshold=1e-2)
    assert np.array_equal(io, ih) and np.max(np.abs(o - h)) < 1e-12 and np.max(np.abs(h[0] - g["shell_admm_out"])) < 1e-10
    o2, io2, h2, ih2 = _dual_project(oracle, h, shell(), max_iter=50, threshold=1e-5, algorithm=capi.ALG_DYKSTRA)
    assert np.array_equal(io2, ih2) and np.max(np.abs(o2 - h2)) < 1e-12 and np.max(np.abs(h2[0] - g["shell_dykstra_out"])) < 1e-10
    # both stages in one call (the `next` chain), as isls.projections.spherical_keepout builds it for the solvers
    hip = hip_kernels()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    import sys
    pj = sys.modules["isls.projections"]
    cs = pj.spherical_keepout(2, g["shell_centres"], [np.sqrt(2 * lo) / 1.1 for lo in g["shell_lowers"]])
    yd = dev(pts)
    desc = capi.Kernels.project_args_chain(yd, yd, cs.stages(), wrap=dev)
    hip._call("project_rows", "f64", desc, None)
    torch.cuda.synchronize()
    assert np.max(np.abs(yd.cpu().numpy() - h2)) < 1e-14
    # general SOC image and the multilinear slab
    soc = [dict(kind=capi.SET_SOC_UNIT, dim=3, A=np.ascontiguousarray(g["gsoc_A"]), b=np.ascontiguousarray(g["gsoc_b"]))]
    zin = np.ascontiguousarray(np.concatenate([g["gsoc_in"][None], 2 * rng.standard_normal((2, 30, 3))]))
    o, io, h, ih = _dual_project(oracle, zin, soc, rho=1.0, max_iter=100, threshold=1e-5, algorithm=capi.ALG_SOC)
    assert np.array_equal(io, ih) and np.max(np.abs(o - h)) < 1e-11 and np.max(np.abs(h[0] - g["gsoc_out"])) < 1e-10
    par = np.concatenate([[2], g["mlin_l"], g["mlin_u"], g["mlin_M"].ravel()])
    o, _, h, _ = _dual_project(oracle, np.ascontiguousarray(g["mlin_in"][None]), [dict(kind=capi.SET_MULTILINEAR, dim=3, par=par)])
    assert np.max(np.abs(o - h)) < 1e-13 and np.max(np.abs(h[0] - g["mlin_out"])) < 1e-11
    # row mask: untouched rows pass through bit for bit
    mask = np.zeros(60, dtype=np.int32)
    mask[[3, 17, 40, 59]] = 1
    o, io, h, ih = _dual_project(oracle, pts, shell(), rho=1.0, max_iter=5, threshold=1e-2, row_mask=mask)
    assert np.array_equal(io, ih) and np.max(np.abs(o - h)) < 1e-12 and np.array_equal(h[:, mask == 0], pts[:, mask == 0])
    # fp32
    o, _, h, _ = _dual_project(oracle, pts.astype(np.float32), shell(np.float32), max_iter=50, threshold=1e-5, algorithm=capi.ALG_DYKSTRA)
    assert np.max(np.abs(o - h)) < 1e-4


@pytest.mark.parametrize("tag", ["d1", "d3"])
def test_config5_sls_admm_kernels(oracle, golden, tag):
    """isls_sls_admm / isls_sls_closed_loop on the device against the oracle (fp64: every iteration, every problem) and
    against the reference's golden outputs: fp64 at 1e-7; fp32 (config 5's own precision) du, phi_u of every contracting
    problem at the north star's 1e-4 or ten times the reference's measured fp32 sensitivity of that problem (fp32_tols),
    residual logs 2e-3.  Problems on which the reference itself ran into max_iter (an unreachable bound: residuals in the
    thousands, no contraction, the inner projections stop on their iteration cap) are followed in fp64 only: there the inner
    stop decisions flip with the last fp32 bit and the iterates differ by O(1) (measured 0.5 - 0.9 relative)."""
    import torch
    from dual import hip_kernels
    from test_oracle_golden import _check_sls_admm, _run_sls_admm, _sls_case, fp32_tols
    g = golden(f"g7_sls_{tag}.npz")
    c = _sls_case(g)
    hip = hip_kernels()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    host = lambda t: tuple(x.cpu().numpy() for x in t)                      # noqa: E731
    # same iteration counts and logs as the oracle with the reference's stop rules (same arithmetic, fp64)
    xo, lo, io = _run_sls_admm(oracle, c, g, rel_tol=0.0)
    xh, lh, ih = host(_run_sls_admm(hip, c, g, wrap=dev, rel_tol=0.0))
    assert np.array_equal(io, ih)
    for b in range(c["P"]):
        assert np.max(np.abs(xo[b] - xh[b])) / np.max(np.abs(xo[b])) < 1e-9
        assert np.nanmax(np.abs(lo[b] - lh[b]) / np.maximum(1e-6, np.abs(lo[b]))) < 1e-6
    # against the reference itself
    _check_sls_admm(lambda sel, mi, rt: host(_run_sls_admm(hip, c, g, wrap=dev, sel=sel, max_iter=mi, rel_tol=rt)), c, g, 1e-7)
    _check_sls_admm(lambda sel, mi, rt: host(_run_sls_admm(hip, c, g, dtype=np.float32, wrap=dev, sel=sel, max_iter=mi, rel_tol=rt)),
                    c, g, 2e-3, only_converged=True, x_tols=fp32_tols(g))
    # closed-loop Monte-Carlo rollout with the reference's controller
    M = g["mc_x0"].shape[1]
    xl, ul = dev(np.zeros((M, c["N"], c["n"]))), dev(np.zeros((M, c["N"], c["m"])))
    hip.sls_closed_loop(dev(g["A"]), dev(g["B"]), dev(g["K"][0]), dev(g["k"][0]), dev(g["mc_x0"][0]), xl, ul)
    torch.cuda.synchronize()
    assert np.max(np.abs(xl.cpu().numpy() - g["mc_x"][0])) < 1e-9 and np.max(np.abs(ul.cpu().numpy() - g["mc_u"][0])) < 1e-8


def test_tassa_all_kernels(dual, golden):
    """ISLS_MODEL_TASSA + ISLS_COST_PHUBER (Tutorial.ipynb car-parking problem) kernel by kernel against the oracle: iLQR
    iterations with 40 candidates, then iLQR-ADMM with the notebook's control limits."""
    from helpers import tassa_arrays
    g = golden("g8_tassa.npz")
    dk = dual(tol=1e-9, ff_nseg=3)
    dk.int_exact = False
    d = OracleDriver(dk, tassa_arrays(g, [0, 1, 0]), project_u=False)
    for it in range(3):
        d.linearize_expand()
        d.gain(), d.ff()
        d.rollout(40, flags=capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST, cost_all=np.zeros((3, 40)))
        d.xhat[:], d.uhat[:], d.cost[:] = d.xx, d.xu, d.cost_new
    d = OracleDriver(dk, tassa_arrays(g, [0, 1]), rho_u=np.diag([1e-1, 1e-2]))
    d.run(2, 40, 5, 0.0)
    _report(dk)


@pytest.mark.parametrize("N", [1, 2, 3])
def test_degenerate_horizons_and_empty_batch(dual, N):
    """Shortest horizons (N = 1: no recursion step at all; N = 2, 3: shorter than every prefetch ring) and an empty batch
    through every kernel of the outer iteration."""
    cfg = P.config2(batch=8, N=N, seed=3)
    pa = problem_arrays(cfg, range(5))
    for nseg in (1, 4):
        dk = dual(ff_nseg=nseg)
        dk.int_exact = False
        d = OracleDriver(dk, pa, rho_u=cfg["rho_u"], relax=cfg["relax"])
        d.run(2, 20, 2, 0.0)
    # B = 0: the entry points return ISLS_OK without looking at the (null) pointers of empty arrays
    import torch
    from dual import hip_kernels
    hip = hip_kernels()
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")     # noqa: E731
    zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")      # noqa: E731
    n, m = 6, 3
    A, Bm = z(0, N, n, n), z(0, N, n, m)
    K, Quu, fac, Qux, k = z(0, N, m, n), z(0, N, m, m), z(0, N, m, m), z(0, N, m, n), z(0, N, m)
    hip.riccati_gain(A, Bm, z(0, N, n, n), z(0, N, m, m), K, Quu, fac, Qux, status=zi(0))
    hip.riccati_ff(A, Bm, z(0, N, n), z(0, N, m), K, Quu, fac, Qux, k)
    hip.admm_update(z(0, N, n), z(0, N, m), z(0, 2), zu=z(0, N, m), lu=z(0, N, m), u_lo=z(N, m), u_hi=z(N, m))
    torch.cuda.synchronize()


def test_long_horizon_car(dual):
    """N = 500 (the horizon of the car notebooks): beyond the 256-step range of the Q_t ballot masks, 50 line-search
    candidates, ragged time-parallel segments."""
    cfg = P.config4(batch=8, N=500, seed=1)
    dk = dual(ff_nseg=7)
    dk.int_exact = False
    d = OracleDriver(dk, problem_arrays(cfg, range(3)), rho_x=cfg["rho_x"], rho_u=cfg["rho_u"], project_x=True)
    d.run(2, 50, 3, 0.0)
    _report(dk)


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-10), ("f32", 1e-4)])
@pytest.mark.parametrize("mode,batch,with_x", [(capi.SOLVE_CHOL, 17, True), (capi.SOLVE_CHOL, 9, False), (capi.SOLVE_INV, 8, True)])
def test_gain_with_first_feedforward_pass(oracle, mode, batch, with_x, dtype, tol):
    """isls_riccati_gain_ff_*: K and the first k of an outer iteration from ONE backward sweep (the way the reference's
    backward_pass_DP computes them, isls/isls.py:285-302) -- against the oracle's gain pass followed by its sequential
    feed-forward pass; time-varying A, B per trajectory, ragged last wavefront, inactive trajectories untouched.  Both
    precisions of the exported entry point (include/isls_hip.h isls_riccati_gain_ff_f64 / _f32): 1e-10 / 1e-4."""
    import torch
    from dual import hip_kernels
    from helpers import rho_to_weights
    okern, hk = oracle, hip_kernels()
    f = np.float64 if dtype == "f64" else np.float32
    rng = np.random.default_rng(3)
    cfg = P.config2(batch=batch, N=60, seed=2)
    cfg = {k_: (v.astype(f) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k_, v in cfg.items()}
    N, n, m, B = 60, 6, 3, batch
    z = lambda *s_: np.zeros(s_, dtype=f)   # noqa: E731
    rn = lambda *shape: rng.standard_normal(shape).astype(f)   # noqa: E731
    # general layout: per-trajectory, time-varying perturbations of the double integrator
    A = np.tile(cfg["A"][None, None], (B, N, 1, 1)) + 0.02 * rn(B, N, n, n)
    Bm = np.tile(cfg["B"][None, None], (B, N, 1, 1)) + 0.02 * rn(B, N, n, m)
    Rr, Qr = rho_to_weights(cfg["rho_u"], N, m, f)[:1], (rho_to_weights(0.3, N, n, f)[:1] if with_x else None)   # [1,d,d]: time-invariant
    xhat, uhat = rn(B, N, n), 0.3 * rn(B, N, m)
    zx, zu = rn(B, N, n), rn(B, N, m)
    lx, lu = 0.1 * rn(B, N, n), 0.1 * rn(B, N, m)
    Cxx, Cuu, c0x, c0u = z(B, N, n, n), z(B, N, m, m), z(B, N, n), z(B, N, m)
    okern.expand_quadratic(cfg["Qs"], cfg["zs"], cfg["seq"], cfg["u_std"], c0x, c0u, xhat=xhat, uhat=uhat, Cxx=Cxx, Cuu=Cuu,
                           Qr=np.tile(Qr, (N, 1, 1)) if with_x else None, Rr=np.tile(Rr, (N, 1, 1)))
    active = np.ones(B, dtype=np.int32)
    active[[1, B - 2]] = 0
    K0 = rn(B, N, m, n)                      # what inactive trajectories must keep
    k0 = rn(B, N, m)
    # oracle: gain, then the sequential feed-forward pass
    K, Quu, fac, Qux, k = K0.copy(), z(B, N, m, m), z(B, N, m, m), z(B, N, m, n), k0.copy()
    st = np.zeros(B, dtype=np.int32)
    okern.riccati_gain(A, Bm, Cxx, Cuu, K, Quu, fac, Qux, solve_mode=mode, status=st, active=active)
    kwx = dict(Qr=np.tile(Qr, (N, 1, 1)), zx=zx, lx=lx) if with_x else {}
    okern.riccati_ff(A, Bm, c0x, c0u, K, Quu, fac, Qux, k, Rr=np.tile(Rr, (N, 1, 1)), xhat=xhat, uhat=uhat, zu=zu, lu=lu,
                     solve_mode=mode, active=active, **kwx)
    # HIP: one launch on the records (the argument blocks hold raw pointers: every device array stays referenced in `d`)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d = {k_: dev(v) for k_, v in dict(A=A, Bm=Bm, Cxx=Cxx, Cuu=Cuu, c0x=c0x, c0u=c0u, K=K0, k=k0, Rr=Rr, xhat=xhat, uhat=uhat, zu=zu,
                                      lu=lu, act=active, st=np.zeros(B, dtype=np.int32), Qr=Qr if with_x else None,
                                      zx=zx if with_x else None, lx=lx if with_x else None).items()}
    dK, dk_, dA, dB, dact, dst, dQr = d["K"], d["k"], d["A"], d["Bm"], d["act"], d["st"], d["Qr"]
    rec = torch.full((capi.ff_record_elems(B, N, n, m),), float("nan"), dtype=torch.float64 if dtype == "f64" else torch.float32, device="cuda")
    g = capi.Kernels.gain_args(dA, dB, d["Cxx"], d["Cuu"], dK, None, None, None, solve_mode=mode, status=dst, active=dact, rec=rec)
    ff = capi.Kernels.ff_args(dA, dB, d["c0x"], d["c0u"], dK, None, None, None, dk_, Qr=dQr, Rr=d["Rr"], xhat=d["xhat"], uhat=d["uhat"],
                              zx=d["zx"], lx=d["lx"], zu=d["zu"], lu=d["lu"], solve_mode=mode, active=dact, rec=rec)
    hk.riccati_gain_ff(g, ff, dtype)
    torch.cuda.synchronize()
    for name, ref, got in (("K", K, dK), ("k", k, dk_)):
        got = got.cpu().numpy()
        assert np.isfinite(ref).all(), f"{name}: oracle not finite"
        bad = np.argwhere(~np.isfinite(got))
        assert bad.size == 0, f"{name}: HIP not finite at {bad[:6].tolist()} ({len(bad)} entries)"
        err = np.max(np.abs(ref - got)) / max(1.0, np.max(np.abs(ref)))
        assert err < tol, f"{name}: rel err {err:.3e}"
        assert np.array_equal(got[[1, B - 2]], (K0 if name == "K" else k0)[[1, B - 2]]), f"{name}: inactive trajectory touched"
    assert np.array_equal(dst.cpu().numpy(), st)
    # a second feed-forward pass on the same records (the ADMM state moved) agrees with the oracle's as well
    zu2 = zu + 0.2 * rn(*zu.shape)
    k2 = k.copy()
    okern.riccati_ff(A, Bm, c0x, c0u, K, Quu, fac, Qux, k2, Rr=np.tile(Rr, (N, 1, 1)), xhat=xhat, uhat=uhat, zu=zu2, lu=lu,
                     solve_mode=mode, active=active, **kwx)
    d["zu2"] = dev(zu2)
    hk.riccati_ff(dA, dB, d["c0x"], d["c0u"], dK, None, None, None, dk_, Qr=dQr, Rr=d["Rr"], xhat=d["xhat"], uhat=d["uhat"],
                  zx=d["zx"], lx=d["lx"], zu=d["zu2"], lu=d["lu"], solve_mode=mode, active=dact, rec=rec)
    torch.cuda.synchronize()
    err = np.max(np.abs(k2 - dk_.cpu().numpy())) / max(1.0, np.max(np.abs(k2)))
    assert err < tol, f"second pass k: rel err {err:.3e}"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", [capi.SOLVE_CHOL, capi.SOLVE_INV])
@pytest.mark.parametrize("dim,batch", [(1, 23), (2, 13), (3, 11)])
def test_structured_gain_pass_is_bit_identical(dim, batch, mode, dtype):
    """isls_gain_args.lin_on (ISLS_MODEL_DI): the gain pass that neither loads nor stages [A B] and takes [A B]'V [A B] and
    A + B K from the two non-zero entries per column against the dense pass -- K, every word of the lean records it writes
    ([K | fac] of every step, against the tail of the dense pass's records),
    and (entry point isls_riccati_gain_ff_*) the first k -- for double integrators of dimension 1, 2, 3, both solve modes, a
    partly filled last wavefront and an inactive trajectory.  fp64: the SAME bits (the terms left out add exact zeros, the
    others keep the dense order).  fp32: equal to rounding only -- the compiler packs some two-term sums of the dense fp32
    kernel into unfused v_pk_mul / v_pk_add pairs and fuses them in the structured one (which reproduces a numpy emulation of
    the fused sequence bit for bit; the dense kernel is the one a unit in the last place off): 1e-5 relative, observed 3e-7 to
    1e-6 after 56 steps.  The dense pass itself is checked against the oracle elsewhere; here the contract of the hint is."""
    import torch
    from dual import hip_kernels
    from isls import models
    hk = hip_kernels()
    f = np.float64 if dtype == "f64" else np.float32
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rng = np.random.default_rng(11 + dim)
    N, n, m, B = 57, 2 * dim, dim, batch
    A1, B1 = P.double_integrator_AB(dim, 2, 0.01)
    mdl = models.LTI(A1, B1)
    assert mdl.model_id == capi.MODEL_DI
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    rn = lambda *shape: rng.standard_normal(shape).astype(f)   # noqa: E731
    par = dev(np.asarray(mdl.params(), dtype=f))
    xhat, uhat = dev(rn(B, N, n)), dev(0.3 * rn(B, N, m))
    A, Bm = torch.zeros(B, N, n, n, dtype=tdt, device="cuda"), torch.zeros(B, N, n, m, dtype=tdt, device="cuda")
    hk.linearize(capi.MODEL_DI, par, xhat, uhat, A, Bm)
    assert np.array_equal(A[3, 7].cpu().numpy(), A1.astype(f)) and np.array_equal(Bm[3, 7].cpu().numpy(), B1.astype(f))
    sq = rn(B, N, n, n)
    Cxx = dev(np.einsum("btij,btkj->btik", sq, sq) + 0.5 * np.eye(n, dtype=f))
    su = rn(B, N, m, m)
    Cuu = dev(np.einsum("btij,btkj->btik", su, su) + 0.5 * np.eye(m, dtype=f))
    Cux = dev(0.1 * rn(B, N, m, n))
    c0x, c0u = dev(rn(B, N, n)), dev(rn(B, N, m))
    Rr, Qr = dev((0.05 * np.eye(m, dtype=f))[None]), dev((0.3 * np.eye(n, dtype=f))[None])
    zx, zu, lx, lu = dev(rn(B, N, n)), dev(rn(B, N, m)), dev(0.1 * rn(B, N, n)), dev(0.1 * rn(B, N, m))
    act = np.ones(B, dtype=np.int32); act[2] = 0
    act = dev(act)
    out = {}
    for lin in (None, (capi.MODEL_DI, par)):
        for fused in (False, True):
            K = torch.full((B, N, m, n), 7.0, dtype=tdt, device="cuda")
            k = torch.full((B, N, m), 7.0, dtype=tdt, device="cuda")
            st = torch.zeros(B, dtype=torch.int32, device="cuda")
            rec = torch.full((capi.ff_record_elems(B, N, n, m),), float("nan"), dtype=tdt, device="cuda")
            g = capi.Kernels.gain_args(A, Bm, Cxx, Cuu, K, None, None, None, Cux=Cux, solve_mode=mode, status=st, active=act, rec=rec, lin=lin)
            if fused:
                ff = capi.Kernels.ff_args(A, Bm, c0x, c0u, K, None, None, None, k, Qr=Qr, Rr=Rr, xhat=xhat, uhat=uhat, zx=zx, lx=lx, zu=zu, lu=lu,
                                          solve_mode=mode, active=act, rec=rec, lin=lin)
                hk.riccati_gain_ff(g, ff, dtype)
            else:
                hk._call("riccati_gain", dtype, g, None)
            torch.cuda.synchronize()
            assert int(st.max()) == 0
            out[(lin is not None, fused)] = (K.cpu().numpy(), rec.cpu().numpy(), k.cpu().numpy())
    for fused in (False, True):
        (K0, r0, k0), (K1, r1, k1) = out[(False, fused)], out[(True, fused)]
        assert np.isfinite(K0).all() and np.abs(K0[0]).max() > 0 and np.array_equal(K0[2], np.full_like(K0[2], 7.0))
        # dense records: [Phi | B | K | fac] at an even stride; with the hint the LEAN ones: their tail [K | fac] at its own even
        # stride in a prefix of the same buffer (an odd word count is padded by one word nobody writes)
        used, tail = n * n + 2 * n * m + m * m, m * n + m * m
        mw = 6 if (n, m) == (4, 2) else 0                          # model words of the pair (rec_model_words): behind fac in both layouts
        stride, lstride = (used + mw + 1) & ~1, (tail + mw + 1) & ~1
        nrec = r0.size // stride
        r0 = r0.reshape(nrec, stride)[:, used - tail:used]
        assert np.isnan(r1[nrec * lstride:]).all(), "the lean layout wrote past its prefix of the buffer"
        r1 = r1[:nrec * lstride].reshape(nrec, lstride)[:, :tail]
        assert np.array_equal(np.isnan(r0), np.isnan(r1)) and (~np.isnan(r0)).sum() >= (B - 1) * (N - 1) * tail
        r0, r1 = np.nan_to_num(r0), np.nan_to_num(r1)
        if dtype == "f64":
            assert np.array_equal(K0, K1), f"K differs (fused={fused}): {np.abs(K0 - K1).max():.3e}"
            bad = np.argwhere(r0 != r1)
            assert bad.size == 0, f"records differ (fused={fused}) at {bad[:5].tolist()}: {r0[tuple(bad[0])]!r} vs {r1[tuple(bad[0])]!r}"
            if fused:
                assert np.isfinite(k0).all() and np.array_equal(k0, k1), f"k differs: {np.abs(k0 - k1).max():.3e}"
        else:
            rel = lambda x, y: float(np.abs(x - y).max() / max(1.0, np.abs(x).max()))   # noqa: E731
            assert rel(K0, K1) < 1e-5 and rel(r0, r1) < 1e-5, f"fused={fused}: K {rel(K0, K1):.2e} records {rel(r0, r1):.2e}"
            if fused:
                assert np.isfinite(k0).all() and rel(k0, k1) < 1e-5, f"k {rel(k0, k1):.2e}"


@pytest.mark.parametrize("nb_dim,nb_deriv", [(1, 3), (2, 3), (2, 1), (3, 1)])
def test_further_state_control_dimensions(dual, nb_dim, nb_deriv):
    """(x_dim, u_dim) beyond the notebooks' four systems: every get_double_integrator_AB(nb_dim <= 3, nb_deriv <= 3) system
    (isls/utils.py:266-276) as a dense LTI model -- (3,1), (6,2), (2,2), (3,3) -- whole DP-form iLQR-ADMM traces (gain,
    feed-forward on the records and in the array form, rollout, update) against the oracle, state and control boxes."""
    rng = np.random.default_rng(10 * nb_dim + nb_deriv)
    n, m, N, batch = nb_dim * nb_deriv, nb_dim, 40, 19
    assert capi.dims_supported(n, m)
    A, Bm = P.double_integrator_AB(nb_dim, nb_deriv, 0.05)
    zs = np.zeros((batch, 2, n))
    zs[:, 1, :nb_dim] = rng.uniform(0.5, 1.5, (batch, nb_dim))
    seq = np.zeros(N, dtype=np.int32)
    seq[N - 1] = 1
    x0 = np.zeros((batch, n))
    x0[:, :nb_dim] = rng.uniform(-0.5, 0.5, (batch, nb_dim))
    cfg = dict(name="di_extra", n=n, m=m, N=N, dt=0.05, A=A, B=Bm, zs=zs, Qs=np.stack([np.zeros((n, n)), 1e2 * np.eye(n)]), seq=seq,
               u_std=1e-2, x0=x0, u0=np.zeros((batch, N, m)), u_lo=-2.0, u_hi=2.0, rho_u=1e-1, relax=1.0, model=P.MODEL_LTI)
    pa = problem_arrays(cfg, range(batch))
    pa["x_lo"], pa["x_hi"] = np.full((N, n), -1.6), np.full((N, n), 1.6)
    for ff_record, ff_nseg in ((True, 1), (False, 1), (True, 3)):
        dk = dual(ff_record=ff_record, ff_nseg=ff_nseg)
        d = OracleDriver(dk, pa, rho_x=0.05, rho_u=cfg["rho_u"], project_x=True)
        d.run(2, 12, 3, 0.0)
        _report(dk)
    assert not capi.dims_supported(5, 7) and capi.dims_generic(5, 7) and not capi.dims_generic(17, 2) and not capi.dims_generic(4, 9)


@pytest.mark.parametrize("n,m,dtype,tol", [(5, 2, "f64", 1e-10), (8, 4, "f64", 1e-10), (12, 6, "f64", 1e-10), (16, 8, "f64", 1e-10),
                                           (1, 1, "f64", 1e-10), (7, 3, "f32", 1e-4), (5, 7, "f32", 1e-4)])
def test_any_state_and_control_dimension(dual, oracle, n, m, dtype, tol):
    """(x_dim, u_dim) WITHOUT an instantiation of the row-per-lane kernels (the reference takes any dimensions,
    isls/base.py:11-14): the generic kernels of csrc/generic.hip (dimensions at run time, matrices in LDS, one trajectory per
    wavefront) against the oracle, kernel call by kernel call over two outer iterations of the DP-form iLQR-ADMM (gain,
    feed-forward, line search with 9 candidates, box update on u and on half of the states) and both solve modes of the gain /
    feed-forward pair (the class surface and the C driver: tests/test_isls_api.py::test_any_dimension_through_the_class_surface)."""
    from helpers import rho_to_weights
    assert not capi.dims_supported(n, m) and capi.dims_generic(n, m)
    f = np.float64 if dtype == "f64" else np.float32
    cfg = P.config_generic(n, m, batch=6, N=40, seed=1)
    pa = problem_arrays(cfg, range(5), dtype=f)
    pa["x_lo"] = np.full((40, n), -np.inf, dtype=f); pa["x_hi"] = np.full((40, n), np.inf, dtype=f)
    pa["x_lo"][:, : (n + 1) // 2], pa["x_hi"][:, : (n + 1) // 2] = -1.0, 1.6
    dk = dual(tol=tol)
    dk.int_exact = dtype == "f64"
    d = OracleDriver(dk, pa, rho_x=0.05, rho_u=cfg["rho_u"], project_x=True, relax=1.2, dtype=f)
    d.run(2, 9, 3, 0.0)
    # explicit-inverse mode of the SLS path (isls/sls.py:149-151) on the same operands
    d.linearize_expand()
    for mode in (capi.SOLVE_CHOL, capi.SOLVE_INV):
        dk.riccati_gain(d.A, d.Bm, d.Cxx, d.Cuu, d.K, d.Quu, d.fac, d.Qux, solve_mode=mode, status=d.status, active=d.admm_active)
        dk.riccati_ff(d.A, d.Bm, d.c0x, d.c0u, d.K, d.Quu, d.fac, d.Qux, d.k, Qr=d.Qr, Rr=d.Rr, xhat=d.xhat, uhat=d.uhat, zx=d.zx, lx=d.lx,
                      zu=d.zu, lu=d.lu, solve_mode=mode, active=d.admm_active)
    _report(dk)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5])
def test_short_horizons_through_the_record_path(dual, N):
    """Horizons of one to five steps through the gain pass with packed records, the record form of the feed-forward pass and the
    outer driver (first feed-forward pass inside the gain pass): no step, one step, an odd and an even number of steps --
    the loops of these kernels run in pairs of steps with a peeled first step."""
    cfg = P.config2(batch=9, N=max(N, 2), seed=5)
    if N == 1:                                                 # config2 needs two steps to build its nominal: cut it back to one
        cfg = dict(cfg, N=1, seq=np.array([1], dtype=np.int32), u0=cfg["u0"][:, :1])
    pa = problem_arrays(cfg, range(9))
    dk = dual(ff_record=True)
    d = OracleDriver(dk, pa, rho_u=cfg["rho_u"], relax=cfg["relax"])
    d.run(2, 7, 3, 0.0)
    _report(dk)
    # the same through isls_ilqr_admm_outer (gain + first ff in one launch) on the device, against the oracle's driver
    from dual import hip_kernels
    from helpers import outer_iteration_on_device
    err = outer_iteration_on_device(cfg, range(9), hip_kernels(), dk.oracle, 7, 3, cfg["rho_u"], cfg["relax"])
    assert err < 1e-10, f"N={N}: {err:.2e}"


@pytest.mark.parametrize("structured", [False, True])
@pytest.mark.parametrize("dtype,tol", [("f64", 1e-10), ("f32", 1e-4)])
@pytest.mark.parametrize("B,J,L", [(33, 3, 20), (8, 5, 7)])
def test_outer_driver_both_precisions(oracle, B, J, L, dtype, tol, structured):
    """isls_ilqr_admm_outer_f64 / _f32 as bench.py runs it (gain pass with the first feed-forward pass inside, record
    feed-forward passes on time-invariant weights, ADMM updates fused into the rollout) over two outer iterations against the
    oracle's own driver of the same precision: K, k, the x-step, z, lambda, residuals, the accepted nominal and its cost.
    structured: with the model hint bench.py's engine gives (the Riccati passes on the double integrator's structure, lean
    records) -- the timed region's form; without: the general layout."""
    from dual import hip_kernels
    from helpers import outer_iteration_on_device
    cfg = P.config2(batch=B, N=100, seed=7)
    err = outer_iteration_on_device(cfg, range(B), hip_kernels(), oracle, L, J, cfg["rho_u"], cfg["relax"], dtype=dtype, outer_iters=2,
                                    structured=structured)
    assert err < tol, f"{dtype}: {err:.2e}"


@pytest.mark.parametrize("B,L", [(33, 20), (7, 5), (10, 33)])
def test_outer_driver_with_mispredicted_winners(oracle, B, L):
    """The rollout records the controls of the candidate `best` names at launch (the previous winner) and replays the winner
    only where that prediction fails.  With `best` scrambled before every outer iteration the wavefronts hold trajectories whose
    prediction hits (recorded u_t, x_t from the checkpoints), trajectories whose prediction misses (winner replay) and both:
    every one of them must give the oracle's x-step, z, lambda and residuals, whatever its neighbours in the wavefront do."""
    from dual import hip_kernels
    from helpers import outer_iteration_on_device
    cfg = P.config2(batch=B, N=100, seed=11)
    err = outer_iteration_on_device(cfg, range(B), hip_kernels(), oracle, L, 3, cfg["rho_u"], cfg["relax"], outer_iters=2, scramble_best=5)
    assert err < 1e-10, f"{err:.2e}"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_state_independent_linearisation_patterns(oracle, dtype):
    """`isls_linearize_*` for the models whose Jacobians do not depend on the state (dense LTI, double integrator): the
    per-step [A | B] pattern is streamed out as 16-byte stores with running pattern indices -- odd and even matrix sizes, one
    step, odd and even horizons, several trajectories with their own parameters, inactive trajectories left untouched; bit
    for bit against the oracle (isls/sls_base.py:49-53, utils.get_double_integrator_AB)."""
    import torch
    from dual import hip_kernels
    hip = hip_kernels()
    np_t = np.float64 if dtype == "f64" else np.float32
    rng = np.random.default_rng(3)
    for (n, m) in [(2, 1), (3, 1), (3, 3), (4, 2), (6, 3), (9, 3)]:
        for N in (1, 2, 7, 100):
            for model in (capi.MODEL_LTI, capi.MODEL_DI):
                if model == capi.MODEL_DI and n % 2:
                    continue
                B = 5
                par = rng.standard_normal((B, n * n + n * m if model == capi.MODEL_LTI else 3)).astype(np_t)
                x, u = np.zeros((B, N, n), np_t), np.zeros((B, N, m), np_t)
                active = np.array([1, 0, 1, 1, 1], dtype=np.int32)
                A0, B0 = np.full((B, N, n, n), 7.0, np_t), np.full((B, N, n, m), 7.0, np_t)
                Ao, Bo = A0.copy(), B0.copy()
                oracle.linearize(model, par, x, u, Ao, Bo, active=active)
                Ad, Bd = torch.from_numpy(A0.copy()).cuda(), torch.from_numpy(B0.copy()).cuda()
                hip.linearize(model, torch.from_numpy(par).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(u).cuda(), Ad, Bd,
                              active=torch.from_numpy(active).cuda())
                torch.cuda.synchronize()
                assert np.array_equal(Ad.cpu().numpy(), Ao) and np.array_equal(Bd.cpu().numpy(), Bo), (n, m, N, model)
                assert np.all(Ao[1] == 7.0) and np.all(Bo[1] == 7.0)


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-10), ("f32", 1e-4)])
@pytest.mark.parametrize("which", ["di3d", "arm", "car"])
def test_outer_advance_equals_accept_restart_linearize_expand(oracle, which, dtype, tol):
    """isls_outer_advance_*: accept + ADMM restart + linearisation + cost expansion of the next outer iteration in one launch,
    against the oracle's plain sequence of those four steps (isls/isls.py:488-499, 414-415, 61-66, 95-102): trajectories that
    were frozen before, that stop in this accept (cost change below tol_cost) and that go on; integer state bit-exact."""
    import torch
    from dual import hip_kernels
    from helpers import model_par, rho_to_weights
    f = np.float64 if dtype == "f64" else np.float32
    cfg = {"di3d": P.config2(batch=16, N=100, seed=3), "arm": P.config3(batch=16, N=100, seed=3), "car": P.config4(batch=16, N=200, seed=3)}[which]
    B, N, n, m = 13, cfg["N"], cfg["n"], cfg["m"]
    pa = problem_arrays(cfg, range(B), dtype=f)
    rng = np.random.default_rng(11)
    rn = lambda *sh: rng.standard_normal(sh).astype(f)   # noqa: E731
    host = dict(xx=pa["xhat"] + f(0.05) * rn(B, N, n), xu=pa["uhat"] + f(0.05) * rn(B, N, m), xhat=pa["xhat"].copy(), uhat=pa["uhat"].copy(),
                cost=(10 + rn(B)).astype(f), cost_hist=rn(B, 8), hist_len=rng.integers(1, 9, B).astype(np.int32),
                outer_active=np.ones(B, dtype=np.int32), admm_active=rng.integers(0, 2, B).astype(np.int32),
                iters=rng.integers(0, 9, B).astype(np.int32), lx=rn(B, N, n), lu=rn(B, N, m), res_prev=rn(B, 2),
                A=rn(B, N, n, n), Bm=rn(B, N, n, m), c0x=rn(B, N, n), c0u=rn(B, N, m))
    host["cost_new"] = (host["cost"] + f(0.5) * rn(B)).astype(f)
    host["cost_new"][[2, 7]] = host["cost"][[2, 7]] + f(1e-5)         # these two meet the stop rule |cost - prev| < tol_cost
    host["outer_active"][[1, 9]] = 0                                   # frozen before
    Qr = rho_to_weights(0.3, N, n, f) if which != "di3d" else None
    Rr = rho_to_weights(cfg["rho_u"], N, m, f)
    par = model_par(cfg, f)

    def run(kern, d, wrap):
        K = capi.Kernels
        acc = K.accept_args(d["xx"], d["xu"], d["cost_new"], d["xhat"], d["uhat"], d["cost"], cost_hist=d["cost_hist"], hist_len=d["hist_len"],
                            tol_cost=1e-3, tol_osc=1e-3, outer_active=d["outer_active"])
        lin = K.linearize_args(cfg["model"], wrap(par), d["xhat"], d["uhat"], d["A"], d["Bm"])
        exp = K.expand_args(wrap(pa["Qtab"]), wrap(pa["ztab"]), wrap(pa["seq"]), cfg["u_std"], d["c0x"], d["c0u"], xhat=d["xhat"], uhat=d["uhat"],
                            Qr=None if Qr is None else wrap(Qr), Rr=wrap(Rr))
        adv = K.advance_args(acc, lin, exp, admm_active=d["admm_active"], iters=d["iters"], lx=d["lx"], lu=d["lu"], res_prev=d["res_prev"])
        kern.outer_advance(adv, dtype)

    ref = {k: v.copy() for k, v in host.items()}
    keep = []
    run(oracle, ref, lambda a: a)
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in host.items()}

    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        keep.append(t)
        return t
    run(hip_kernels(), dev, to_dev)
    torch.cuda.synchronize()
    assert ref["outer_active"].tolist() == [1, 0, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1]
    for k, v in ref.items():
        got = dev[k].cpu().numpy()
        if v.dtype.kind in "iu":
            assert np.array_equal(v, got), k
        else:
            err = np.max(np.abs(v.astype(np.float64) - got)) / max(1.0, float(np.max(np.abs(v))))
            assert err < tol, f"{k}: {err:.2e}"
    # frozen trajectories keep everything; stopped ones keep the OLD linearisation and expansion
    for b in (1, 9, 2, 7):
        assert np.array_equal(dev["A"].cpu().numpy()[b], host["A"][b]) and np.array_equal(dev["c0x"].cpu().numpy()[b], host["c0x"][b])
    for b in (1, 9):
        assert np.array_equal(dev["xhat"].cpu().numpy()[b], host["xhat"][b]) and dev["admm_active"][b].item() == 0
