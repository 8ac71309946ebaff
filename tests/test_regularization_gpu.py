"""The regularised Riccati gain pass on the device (isls_riccati_gain_reg_*, isls_reg_update_*, `regularization=`) against the C
oracle run on materialised tables Cuu + mu I / Cxx + mu I (tests/reg_reference.py).  Tolerances: fp64 1e-10, fp32 1e-4, relative
to max(1, |ref|_max)."""
import numpy as np
import pytest

import isls_problems as P
from isls import _capi as capi
from reg_reference import ST_NOT_PD, ST_REG_MAX, Schedule, gain, gain_with_retries, materialise

pytestmark = pytest.mark.gpu

# (n, m, B): B spans one full wavefront (T = 64 // (n + m) trajectories; one in the generic form) and a partial one
FAST = [(6, 3, 9), (4, 2, 13), (9, 3, 7)]
SHAPES = FAST + [(5, 2, 2)]
DTYPES = [("f64", 1e-10), ("f32", 1e-4)]


def _problem(n, m, B, N, f, seed=0):
    """A convex LQ batch in the general layout: per-trajectory, time-varying A, B, cost Hessians with Cux."""
    rng = np.random.default_rng(seed + 100 * n + m)
    rn = lambda *s: rng.standard_normal(s)                     # noqa: E731
    A = np.eye(n) + 0.1 * rn(B, N, n, n) / np.sqrt(n)
    Bm = 0.1 * rn(B, N, n, m)
    M = rn(B, N, n + m, n + m) / np.sqrt(n + m)
    C = M @ M.transpose(0, 1, 3, 2) + np.eye(n + m)
    c = dict(A=A, Bm=Bm, Cxx=C[..., :n, :n], Cuu=C[..., n:, n:], Cux=0.3 * C[..., n:, :n], c0x=rn(B, N, n), c0u=rn(B, N, m))
    return {k: np.ascontiguousarray(v).astype(f) for k, v in c.items()}


def _mus(B, f):
    """a mix of zeros and values over six decades"""
    mu = np.array([0.0, 1e-3, 1e-2, 0.0, 1e-1, 1.0, 10.0, 0.0, 1e2, 1e3, 3e-3, 0.0, 30.0], dtype=f)
    return np.ascontiguousarray(mu[:B])


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    return float(np.max(np.abs(got - ref)) / max(1.0, float(np.max(np.abs(ref)))))


def _dev(c):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}


def _zeros(f, *shapes):
    import torch
    dt = torch.float64 if f == np.float64 else torch.float32
    return [torch.zeros(*s, dtype=dt, device="cuda") for s in shapes]


def _oracle_pass(okern, c, mu, on_x, mode, f, with_ff=True):
    B, N, n = c["A"].shape[:3]
    m = c["Bm"].shape[-1]
    z = lambda *s: np.zeros(s, dtype=f)                        # noqa: E731
    K, Quu, fac, Qux, k, st = z(B, N, m, n), z(B, N, m, m), z(B, N, m, m), z(B, N, m, n), z(B, N, m), np.zeros(B, dtype=np.int32)
    gain(okern, c["A"], c["Bm"], c["Cxx"], c["Cuu"], mu, on_x, (K, Quu, fac, Qux), solve_mode=mode, status=st, Cux=c["Cux"])
    if with_ff:
        okern.riccati_ff(c["A"], c["Bm"], c["c0x"], c["c0u"], K, Quu, fac, Qux, k, solve_mode=mode)
    return dict(K=K, Quu=Quu, fac=fac, Qux=Qux, k=k, st=st)


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("mode", [capi.SOLVE_CHOL, capi.SOLVE_INV])
@pytest.mark.parametrize("on_x", [False, True])
@pytest.mark.parametrize("N", [11, 12])
@pytest.mark.parametrize("n,m,B", SHAPES)
def test_kernel_parity(oracle, n, m, B, N, on_x, mode, dtype, tol):
    """Array form, record form followed by a record feed-forward pass, and the pass with the first feed-forward pass inside."""
    import torch
    from dual import hip_kernels
    hk, f = hip_kernels(), (np.float64 if dtype == "f64" else np.float32)
    c = _problem(n, m, B, N, f)
    mu = _mus(B, f)
    ref = _oracle_pass(oracle, c, mu, on_x, mode, f)
    assert not ref["st"].any()
    d = _dev(c)
    dmu = torch.from_numpy(mu).cuda()
    G, F = capi.Kernels.gain_args, capi.Kernels.ff_args
    # the arrays
    K, Quu, fac, Qux, k = _zeros(f, (B, N, m, n), (B, N, m, m), (B, N, m, m), (B, N, m, n), (B, N, m))
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    g = G(d["A"], d["Bm"], d["Cxx"], d["Cuu"], K, Quu, fac, Qux, Cux=d["Cux"], solve_mode=mode, status=st)
    hk.riccati_gain_reg(g, None, dmu, on_x, dtype)
    torch.cuda.synchronize()
    for name, got in (("K", K), ("Quu", Quu), ("fac", fac), ("Qux", Qux)):
        err = _rel(got.cpu().numpy(), ref[name])
        print(f"array form {name}: {err:.3e}")
        assert err < tol, (name, err)
    assert not st.cpu().numpy().any()
    if (n, m, B) not in FAST:
        return                                                 # the generic pairs have the array form only
    # records + K, then the feed-forward pass on the records
    K2, k2 = _zeros(f, (B, N, m, n), (B, N, m))
    rec = torch.full((capi.ff_record_elems(B, N, n, m),), float("nan"), dtype=K2.dtype, device="cuda")
    g = G(d["A"], d["Bm"], d["Cxx"], d["Cuu"], K2, None, None, None, Cux=d["Cux"], solve_mode=mode, status=st, rec=rec)
    hk.riccati_gain_reg(g, None, dmu, on_x, dtype)
    ff = F(d["A"], d["Bm"], d["c0x"], d["c0u"], K2, None, None, None, k2, solve_mode=mode, rec=rec)
    hk._call("riccati_ff", dtype, ff, None)
    torch.cuda.synchronize()
    for name, got in (("K", K2), ("k", k2)):
        err = _rel(got.cpu().numpy(), ref[name])
        print(f"record form {name}: {err:.3e}")
        assert err < tol, (name, err)
    # the first feed-forward pass inside (the pairs that have that form)
    if n * n + n * (n + m) <= 100:
        K3, k3 = _zeros(f, (B, N, m, n), (B, N, m))
        rec.fill_(float("nan"))
        g = G(d["A"], d["Bm"], d["Cxx"], d["Cuu"], K3, None, None, None, Cux=d["Cux"], solve_mode=mode, status=st, rec=rec)
        ff = F(d["A"], d["Bm"], d["c0x"], d["c0u"], K3, None, None, None, k3, solve_mode=mode, rec=rec)
        hk.riccati_gain_reg(g, ff, dmu, on_x, dtype)
        torch.cuda.synchronize()
        for name, got in (("K", K3), ("k", k3)):
            err = _rel(got.cpu().numpy(), ref[name])
            print(f"ff inside {name}: {err:.3e}")
            assert err < tol, (name, err)
    assert not st.cpu().numpy().any()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", [capi.SOLVE_CHOL, capi.SOLVE_INV])
@pytest.mark.parametrize("N", [11, 12])
@pytest.mark.parametrize("n,m,B", SHAPES)
def test_zero_mu_is_the_plain_pass_bit_for_bit(n, m, B, N, mode, dtype):
    import torch
    from dual import hip_kernels
    hk, f = hip_kernels(), (np.float64 if dtype == "f64" else np.float32)
    d = _dev(_problem(n, m, B, N, f))
    dmu = torch.zeros(B, dtype=d["A"].dtype, device="cuda")
    G, F = capi.Kernels.gain_args, capi.Kernels.ff_args
    same = lambda a, b: np.array_equal(a.cpu().numpy(), b.cpu().numpy())   # noqa: E731
    out = []
    for reg in (False, True):                                  # the arrays
        K, Quu, fac, Qux = _zeros(f, (B, N, m, n), (B, N, m, m), (B, N, m, m), (B, N, m, n))
        st = torch.zeros(B, dtype=torch.int32, device="cuda")
        g = G(d["A"], d["Bm"], d["Cxx"], d["Cuu"], K, Quu, fac, Qux, Cux=d["Cux"], solve_mode=mode, status=st)
        hk.riccati_gain_reg(g, None, dmu, True, dtype) if reg else hk._call("riccati_gain", dtype, g, None)
        torch.cuda.synchronize()
        out.append((K, Quu, fac, Qux, st))
    assert all(same(a, b) for a, b in zip(*out))
    assert np.isfinite(out[0][0].cpu().numpy()).all() and out[0][0].abs().max().item() > 0
    if (n, m, B) not in FAST:
        return
    for inside in ([False, True] if n * n + n * (n + m) <= 100 else [False]):
        out = []
        for reg in (False, True):
            K, k = _zeros(f, (B, N, m, n), (B, N, m))
            st = torch.zeros(B, dtype=torch.int32, device="cuda")
            rec = torch.full((capi.ff_record_elems(B, N, n, m),), float("nan"), dtype=K.dtype, device="cuda")
            g = G(d["A"], d["Bm"], d["Cxx"], d["Cuu"], K, None, None, None, Cux=d["Cux"], solve_mode=mode, status=st, rec=rec)
            ff = F(d["A"], d["Bm"], d["c0x"], d["c0u"], K, None, None, None, k, solve_mode=mode, rec=rec)
            if reg:
                hk.riccati_gain_reg(g, ff if inside else None, dmu, True, dtype)
            elif inside:
                hk.riccati_gain_ff(g, ff, dtype)
            else:
                hk._call("riccati_gain", dtype, g, None)
            if not inside:
                hk._call("riccati_ff", dtype, ff, None)         # the feed-forward output from the records
            torch.cuda.synchronize()
            out.append((K, k, st))
        assert all(same(a, b) for a, b in zip(*out)), f"inside={inside}"
        assert np.isfinite(out[0][1].cpu().numpy()).all() and out[0][1].abs().max().item() > 0


def test_model_hint_with_regularisation_is_unsupported():
    import torch
    from dual import hip_kernels
    hk = hip_kernels()
    B, N, n, m = 9, 11, 6, 3
    d = _dev(_problem(n, m, B, N, np.float64))
    K, = _zeros(np.float64, (B, N, m, n))
    rec = torch.zeros(capi.ff_record_elems(B, N, n, m), dtype=torch.float64, device="cuda")
    par = torch.tensor([0.01, 5e-5, 0.01], dtype=torch.float64, device="cuda")
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    g = capi.Kernels.gain_args(d["A"], d["Bm"], d["Cxx"], d["Cuu"], K, None, None, None, status=st, rec=rec, lin=(capi.MODEL_DI, par))
    with pytest.raises(capi.IslsError, match=f"-> {capi.ERR_UNSUPPORTED}"):
        hk.riccati_gain_reg(g, None, torch.zeros(B, dtype=torch.float64, device="cuda"), False, "f64")


# ---- the retry loop through the engine ---------------------------------------------------------------------------------
C_NEG = 2.1     # Cuu = -C_NEG I for the failing trajectory: between the ladder's rungs 0.32 and 13.9 (1e-6 * 1.6^27, 1e-6 * 1.6^35)


def _engine_with(c, f, reg):
    import torch
    import isls
    B, N, n = c["A"].shape[:3]
    m = c["Bm"].shape[-1]
    e = isls.Engine(B, N, n, m, dtype=torch.float64 if f == np.float64 else torch.float32)
    e.allow_shared_hessian = False
    d = _dev(c)
    e.A, e.Bm = d["A"], d["Bm"]
    e.ab_from_caller()
    e.Cxx, e.Cuu, e.Cux, e.c0x, e.c0u = d["Cxx"], d["Cuu"], d["Cux"], d["c0x"], d["c0u"]
    e.set_regularization(reg)
    return e


def _retry_case(oracle, n, m, B, N, f, c_neg, bad=3):
    """(problem, reference after the loop): trajectory `bad` has Cuu = -c I, Cux = 0 at every step"""
    c = _problem(n, m, B, N, f)
    c["Cuu"][bad] = -c_neg * np.eye(m, dtype=f)
    c["Cux"][bad] = 0
    z = lambda *s: np.zeros(s, dtype=f)                        # noqa: E731
    sched, st = Schedule(B, f), np.zeros(B, dtype=np.int32)
    out = (z(B, N, m, n), z(B, N, m, m), z(B, N, m, m), z(B, N, m, n))
    launches = gain_with_retries(oracle, c["A"], c["Bm"], c["Cxx"], c["Cuu"], sched, False, out, st)
    return c, sched, st, launches


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("N", [11, 12])
@pytest.mark.parametrize("n,m,B", [(6, 3, 9), (4, 2, 13), (9, 3, 7), (5, 2, 5)])
def test_retry_one_failing_trajectory(oracle, n, m, B, N, dtype, tol):
    """Trajectory 3 (inside the full wavefront) has Cuu = -C_NEG I.  C_NEG lies between two rungs of the ladder with more than 10 %
    to spare: the oracle reaches the same final mu for 0.95 C_NEG and 1.05 C_NEG (asserted here on the CPU)."""
    import torch
    import isls
    f = np.float64 if dtype == "f64" else np.float32
    c, sched, st_ref, launches = _retry_case(oracle, n, m, B, N, f, C_NEG)
    for scale in (0.95, 1.05):
        assert _retry_case(oracle, n, m, B, N, f, C_NEG * scale)[1].mu[3] == sched.mu[3]
    assert launches > 2 and sched.mu[3] > 0 and not np.delete(sched.mu, 3).any() and not st_ref.any()
    # the plain pass flags exactly that trajectory
    plain = _engine_with(c, f, None)
    rec0 = plain.ff_record()                                   # None for the generic pair: the arrays
    plain.gain(rec=rec0)
    torch.cuda.synchronize()
    assert plain.status.cpu().numpy().tolist() == [ST_NOT_PD if b == 3 else 0 for b in range(B)]
    # the loop
    e = _engine_with(c, f, isls.Regularization())
    rec = e.ff_record()
    assert (rec is None) == ((n, m) == (5, 2))
    e.gain(rec=rec)
    e.feedforward(rec=rec)
    torch.cuda.synchronize()
    assert not e.status.cpu().numpy().any()
    assert e.reg_gain_launches == launches
    assert np.array_equal(e.reg_mu.cpu().numpy(), sched.mu)
    others = [b for b in range(B) if b != 3]
    assert np.array_equal(e.K.cpu().numpy()[others], plain.K.cpu().numpy()[others])
    # one pass given the final mu up front: bitwise on the device, and the oracle's feed-forward pass for all trajectories
    one = _engine_with(c, f, isls.Regularization())
    one.reg_mu.copy_(e.reg_mu)
    rec1 = one.ff_record()
    one.gain(rec=rec1)
    one.feedforward(rec=rec1)
    torch.cuda.synchronize()
    assert one.reg_gain_launches == 1
    assert np.array_equal(one.K.cpu().numpy(), e.K.cpu().numpy()) and np.array_equal(one.k.cpu().numpy(), e.k.cpu().numpy())
    if rec is None:                                            # generic pair: K, Quu, fac, Qux arrays instead of records
        for name in ("Quu", "fac", "Qux"):
            assert np.array_equal(getattr(one, name).cpu().numpy(), getattr(e, name).cpu().numpy())
            assert _rel(getattr(e, name).cpu().numpy()[:, :-1], _oracle_pass(oracle, c, sched.mu, False, capi.SOLVE_CHOL, f)[name][:, :-1]) < tol
    # the records [blocks][N][T][stride]: the words of every step (t = N-1 is not written; a pad word of the stride carries nothing)
    T, used = 64 // (n + m), n * n + 2 * n * m + m * m + (6 if (n, m) in ((9, 3), (4, 2)) else 0)
    view = lambda r: r.cpu().numpy().reshape(-(-B // T), N, T, -1)[:, :N - 1, :, :used]   # noqa: E731
    if rec is not None:
        assert view(rec).shape[-1] == used and np.isfinite(view(rec)).all()
        assert np.array_equal(view(rec1), view(rec))
    ref = _oracle_pass(oracle, c, sched.mu, False, capi.SOLVE_CHOL, f)
    for name, got in (("K", e.K), ("k", e.k)):
        err = _rel(got.cpu().numpy(), ref[name])
        print(f"{name}: {err:.3e}")
        assert err < tol, (name, err)


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("N", [11, 12])
@pytest.mark.parametrize("n,m,B", [(6, 3, 9), (4, 2, 13), (9, 3, 7), (5, 2, 5)])
def test_ladder_exhausted(oracle, n, m, B, N, dtype, tol):
    """Cuu = -1e12 I: the ladder ends below mu_max = 1e10; that trajectory keeps NOT_PD and gets REG_MAX, nothing raises, the
    others are solved."""
    import torch
    import isls
    f = np.float64 if dtype == "f64" else np.float32
    c, sched, st_ref, launches = _retry_case(oracle, n, m, B, N, f, 1e12)
    assert st_ref.tolist() == [ST_NOT_PD | ST_REG_MAX if b == 3 else 0 for b in range(B)]
    e = _engine_with(c, f, isls.Regularization())
    e.gain(rec=e.ff_record())                                  # records + K; the generic pair has none: the arrays
    torch.cuda.synchronize()
    assert e.status.cpu().numpy().tolist() == st_ref.tolist()
    assert e.reg_gain_launches == launches
    assert np.array_equal(e.reg_mu.cpu().numpy(), sched.mu) and not np.delete(sched.mu, 3).any()
    plain = _engine_with(c, f, None)
    plain.gain(rec=plain.ff_record())
    torch.cuda.synchronize()
    others = [b for b in range(B) if b != 3]
    assert np.array_equal(e.K.cpu().numpy()[others], plain.K.cpu().numpy()[others])
    ref = _oracle_pass(oracle, c, np.zeros(B, dtype=f), False, capi.SOLVE_CHOL, f, with_ff=False)
    err = _rel(e.K.cpu().numpy()[others], ref["K"][others])
    print(f"K: {err:.3e}")
    assert err < tol


# ---- the front end -----------------------------------------------------------------------------------------------------
def _via_point_solver(B=9, N=12):
    import isls
    from isls import models
    cfg = P.config2(batch=B, N=N, seed=0)
    s = isls.iSLS(cfg["n"], cfg["m"], N, batch=B)
    s.forward_model = models.LTI(cfg["A"], cfg["B"])
    s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in range(B)])
    s.reset()
    s.nominal_values = np.stack(xs), np.stack(us)
    return s, cfg


def test_ilqr_admm_with_regularisation_equals_the_plain_call_on_a_convex_problem():
    import isls
    from isls import Box
    res = []
    for reg in (None, isls.Regularization()):
        s, cfg = _via_point_solver()
        kw = dict(project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=2, max_line_search_iter=20, max_admm_iter=3, rho_u=cfg["rho_u"], tol=0.0)
        s.ilqr_admm(regularization=reg, **kw) if reg is not None else s.ilqr_admm(**kw)
        a = s.engine._outer_args
        res.append((s.x_nom, s.u_nom, np.asarray(s.cost), int(a.skip_gain), int(a.gain.lin_on), s.reg_mu, s.status,
                    s.engine._structure_expected()))
    (x0, u0, c0, skip0, _, _, st0, structured0), (x1, u1, c1, skip1, lin1, mu1, st1, structured1) = res
    assert (skip0, skip1, lin1) == (0, 1, 0)                   # the driver skips its own gain pass; general layout
    # the model's structure applies to the plain call (which form of it the engine picks depends on the batch size: from 512
    # trajectories on the structured sequential passes, below that the time-parallel ones) and not to the regularised one
    assert structured0 and not structured1
    assert not mu1.any() and not st0.any() and not st1.any()
    for got, ref in ((x1, x0), (u1, u0), (c1, c0)):
        assert _rel(got, ref) < 1e-10


def test_refusals():
    import isls
    reg = isls.Regularization()
    s, cfg = _via_point_solver()
    with pytest.raises(capi.IslsError, match="regularisation"):
        s.isls_admm(2, regularization=reg)
    with pytest.raises(capi.IslsError, match="regularisation"):
        s.solve(method='batch', regularization=reg)
    with pytest.raises(capi.IslsError, match="regularisation"):
        # (a ball: no box, so the z-step runs through the host)
        s.ilqr_admm(project_u=lambda u: u * min(1.0, 5.0 / (np.linalg.norm(u) + 1e-30)), rho_u=cfg["rho_u"], max_iter=1, regularization=reg)
    s.engine.set_regularization(reg)
    with pytest.raises(capi.IslsError, match="regularisation"):
        s.backward_pass_batch()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", [capi.REG_AFTER_GAIN, capi.REG_AFTER_LS])
def test_schedule_kernel_equals_the_reference(mode, dtype):
    """isls_reg_update_* over every combination of status bits, mask and ladder position (B = 600: three blocks, the last one
    partial) against reg_reference.Schedule, bit for bit; three rounds, so that raised and lowered values are raised again."""
    import torch
    from dual import hip_kernels
    hk, f = hip_kernels(), (np.float64 if dtype == "f64" else np.float32)
    rng = np.random.default_rng(5)
    B = 600
    sched = Schedule(B, f)
    sched.mu[:] = rng.choice(np.array([0.0, 1e-6, 3e-6, 1e-3, 1.0, 1e5, 3e9, 9e9, 1e10], dtype=f), B)
    sched.delta[:] = rng.choice(np.array([1.0, 1.6, 1 / 1.6, 4.096, 0.2, 30.0], dtype=f), B)
    active = (rng.random(B) < 0.8).astype(np.int32)
    mu, delta, act = torch.from_numpy(sched.mu.copy()).cuda(), torch.from_numpy(sched.delta.copy()).cuda(), torch.from_numpy(active).cuda()
    retry, count = torch.full((B,), 7, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    fail = ST_NOT_PD if mode == capi.REG_AFTER_GAIN else capi.ST_LS_REJECT
    for _ in range(3):
        st = rng.choice(np.array([0, 1, 2, 4, 5, 8, 9, 12], dtype=np.int32), B)
        dst = torch.from_numpy(st.copy()).cuda()
        count.zero_()
        hk.reg_update(mode, dst, mu, delta, 1.6, 1e-6, 1e10, active=act, retry=retry, count=count)
        torch.cuda.synchronize()
        want_retry = np.zeros(B, dtype=np.int32)
        for b in range(B):
            if not active[b] or st[b] & ST_REG_MAX:
                continue
            if st[b] & fail:
                if sched.raise_(b):
                    if mode == capi.REG_AFTER_GAIN:
                        st[b] &= ~ST_NOT_PD
                        want_retry[b] = 1
                else:
                    st[b] |= ST_REG_MAX
            elif mode == capi.REG_AFTER_LS and not st[b] & ST_NOT_PD:
                sched.lower(b)
        assert np.array_equal(dst.cpu().numpy(), st)
        assert np.array_equal(mu.cpu().numpy(), sched.mu) and np.array_equal(delta.cpu().numpy(), sched.delta)
        if mode == capi.REG_AFTER_GAIN:
            assert np.array_equal(retry.cpu().numpy(), want_retry) and int(count.item()) == want_retry.sum() > 0


def test_one_regularised_iteration_on_a_convex_problem_is_the_plain_one():
    """The convex via-point problem with linear dynamics, one iteration: no Quu fails and every step is accepted, so mu stays 0
    (a lowered 0 is 0) and the regularised route (K and k from the one launch on the records) gives the plain solve's result."""
    import isls
    one = []
    for reg in (None, isls.Regularization()):
        s, cfg = _via_point_solver()
        s.solve(max_iter=1, max_line_search_iter=20, regularization=reg)
        one.append((np.asarray(s.cost), s.x_nom, s.u_nom, s.reg_mu, s.status))
    (c0, x0, u0, _, st0), (c1, x1, u1, mu1, st1) = one
    assert not mu1.any() and not st0.any() and not st1.any()
    for got, ref in ((c1, c0), (x1, x0), (u1, u0)):
        assert _rel(got, ref) < 1e-10


# ---- end to end --------------------------------------------------------------------------------------------------------
REG = dict(mu_init=0.0, mu_min=1e-6, mu_max=1e10, factor=1.6)
BUMP_PAR = [0.01, 40.0, 0.5, 0.0, 0.25, 0.05, 20.0, 1.0, 0.0]   # [w_u, w_o, ox, oy, r, w_x, w_f, gx, gy]


def _compare_with_reference(s, ref, iters):
    """cost logs and final mu at 1e-6 relative, the accept / reject sequence and the final status exactly"""
    costs = np.array(s.cost_log)
    assert costs.shape == ref["costs"].shape == (iters + 1, s.batch)
    acc = np.diff(costs, axis=0) != 0                           # an accepted step moves the cost, a rejected one keeps it
    assert np.array_equal(acc, ref["ok"])
    assert (np.diff(costs, axis=0)[acc] < 0).all()              # every accepted cost is below its predecessor
    err = np.max(np.abs(costs - ref["costs"]) / np.maximum(1.0, np.abs(ref["costs"])))
    print(f"cost logs: {err:.3e}")
    assert err < 1e-6
    mu_err = np.max(np.abs(s.reg_mu - ref["mu_final"]) / np.maximum(1.0, np.abs(ref["mu_final"])))
    print(f"reg_mu: {mu_err:.3e}  {s.reg_mu}")
    assert mu_err < 1e-6
    assert np.array_equal(s.status, ref["status"])


def test_nonconvex_solve_end_to_end(oracle):
    """Double integrator in the plane (4, 2) past an exp(-d^2/r^2) obstacle bump (costs.Custom), B = 9, N = 30, start points
    straddling the obstacle.  At mu = 0 the oracle's first gain pass reports NOT_PD for some trajectories and not for all (the
    plain solve raises LinAlgError for the call); with a regularisation the call returns and follows reg_reference.solve."""
    import isls
    import reg_reference as R
    from isls import costs, models
    B, N, dt, iters, L = 9, 30, 0.1, 12, 10
    A, Bm = P.double_integrator_AB(2, 2, dt)
    f = lambda x, u: x @ A.T + u @ Bm.T                        # noqa: E731
    get_AB = lambda x, u: (np.broadcast_to(A, (N, 4, 4)).copy(), np.broadcast_to(Bm, (N, 4, 2)).copy())   # noqa: E731
    x0 = np.zeros((B, 4))
    x0[:, 1] = np.linspace(-1.0, 1.0, B) + 0.03
    u0 = np.zeros((B, N, 2))
    xs = np.stack([P.rollout_open_loop(f, x0[b], u0[b]) for b in range(B)])
    bump = R.BumpCost(BUMP_PAR)
    # the oracle at mu = 0: some, not all
    c0x, c0u, Cxx, Cuu, Cux = bump.expand(xs, u0)
    z = lambda *sh: np.zeros(sh)                               # noqa: E731
    st = np.zeros(B, dtype=np.int32)
    oracle.riccati_gain(np.broadcast_to(A, (B, N, 4, 4)).copy(), np.broadcast_to(Bm, (B, N, 4, 2)).copy(), Cxx, Cuu,
                        z(B, N, 2, 4), z(B, N, 2, 2), z(B, N, 2, 2), z(B, N, 2, 4), Cux=Cux, status=st)
    bad = (st & ST_NOT_PD) != 0
    assert bad.any() and not bad.all()

    def solver():
        s = isls.iSLS(4, 2, N, batch=B)
        s.forward_model = models.LTI(A, Bm)
        s.cost_function = costs.Custom(4, 2, BUMP_PAR, R.BumpCost.SOURCE)
        s.nominal_values = xs, u0
        return s
    s = solver()
    assert _rel(np.asarray(s.cost), bump.value(xs, u0)) < 1e-12
    with pytest.raises(np.linalg.LinAlgError) as info:
        s.solve(max_iter=iters, max_line_search_iter=L)
    assert str(np.nonzero(bad)[0].tolist()) in str(info.value)   # the same trajectories as the oracle's
    with pytest.raises(np.linalg.LinAlgError):
        R.solve(oracle, f, get_AB, bump, xs, u0, iters, L)
    s = solver()
    s.solve(max_iter=iters, max_line_search_iter=L, regularization=isls.Regularization())
    ref = R.solve(oracle, f, get_AB, bump, xs, u0, iters, L, reg=REG)
    assert (ref["mu"] > 0).any() and ref["ok"].any() and not ref["ok"].all()
    _compare_with_reference(s, ref, len(ref["ok"]))
    assert _rel(s.x_nom, ref["x"]) < 1e-6


def test_rejected_line_search_on_the_car(oracle):
    """Simple car (config 4's via-point cost, N = 30, B = 3) from random controls with two line-search candidates: reg_reference
    rejects the first step of trajectory 0.  Without the keyword that trajectory stops there (present behaviour); with it mu
    rises, a later step is accepted and the final cost is below the cost at the reject."""
    import isls
    import reg_reference as R
    from isls import models
    B, N, L, iters = 3, 30, 2, 15
    cfg = P.config4(batch=B, N=N, seed=1)
    f, get_AB = P.car_f(cfg["dt"]), P.car_get_AB(cfg["dt"], N)
    u0 = 0.5 * np.random.default_rng(0).standard_normal((B, N, 2))
    xs = np.stack([P.rollout_open_loop(f, cfg["x0"][b], u0[b]) for b in range(B)])
    zs = cfg["zs"] if cfg["zs"].ndim == 2 else cfg["zs"][0]
    cost = R.ViaCost(zs, cfg["Qs"], cfg["seq"], cfg["u_std"])
    ref, ref_plain = R.solve(oracle, f, get_AB, cost, xs, u0, iters, L, reg=REG), R.solve(oracle, f, get_AB, cost, xs, u0, iters, L)
    assert not ref["ok"][0, 0] and ref["ok"][1:, 0].any()       # rejected at once, accepted later
    assert ref["mu"][0, 0] == 1e-6 and ref["costs"][-1, 0] < ref["costs"][1, 0] == ref["costs"][0, 0]

    def solver():
        s = isls.iSLS(4, 2, N, batch=B)
        s.forward_model = models.CarSimple(cfg["dt"])
        s.set_cost_variables(zs, cfg["Qs"], cfg["seq"], cfg["u_std"])
        s.nominal_values = xs, u0
        return s
    # present behaviour: the trajectory stops at the reject
    p = solver()
    p.solve(max_iter=iters, max_line_search_iter=L)
    costs = np.array(p.cost_log)
    assert costs.shape == ref_plain["costs"].shape and np.array_equal(np.diff(costs, axis=0) != 0, ref_plain["ok"])
    # (the plain loop clears every status word at the start of an iteration, so the reject bit itself is gone by the end)
    assert (costs[:, 0] == costs[0, 0]).all() and not p.engine.outer_active.cpu().numpy()[0] and len(costs) - 1 < iters
    # with the keyword it goes on
    s = solver()
    s.solve(max_iter=iters, max_line_search_iter=L, regularization=isls.Regularization())
    _compare_with_reference(s, ref, len(ref["ok"]))
    costs = np.array(s.cost_log)
    assert costs[-1, 0] < costs[1, 0] == costs[0, 0]
