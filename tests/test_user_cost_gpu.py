"""User-written cost functions (isls.costs.Custom) on the device.

The expansion (hyper-dual numbers) and the nominal cost agree with the reference's pseudo-Huber derivatives and with the
hand-written numpy derivatives of a coupled cost.  The line search with a Custom restatement of a built-in cost agrees with the
built-in one.  The Tassa car-parking runs end to end with no get_Cs, and a coupled cost on a models.Custom quadrotor equals the
host path of the same cost given as numpy callables, through solve, ilqr_admm and the timed driver with advance()."""
import numpy as np
import pytest
import torch

from test_isls_api import _check_final, rel

import user_costs as uc
import user_models as um

pytestmark = pytest.mark.gpu


def tassa_costs(g):
    from isls import costs
    ph = costs.PseudoHuber(g["par_cu"], g["par_cx"], g["par_px"], g["par_cf"], g["par_pf"])
    cu = costs.Custom(4, 2, uc.phuber_params(g["par_cu"], g["par_cx"], g["par_cf"]), uc.phuber_source(4, 2, g["par_px"], g["par_pf"]))
    return ph, cu


# ---- 1. expansion and nominal cost ------------------------------------------------------------------------------------------
def test_phuber_restatement_against_the_reference(golden):
    g = golden("g8_tassa.npz")
    _, cu = tassa_costs(g)
    cs, Cs = cu.get_Cs(g["fd_x"], g["fd_u"])
    print("phuber get_Cs", rel(cs, g["fd_cs"]), rel(Cs, g["fd_Cs"]))
    assert rel(cs, g["fd_cs"]) < 1e-10 and rel(Cs, g["fd_Cs"]) < 1e-10
    c0 = cu(g["x_nom0"], g["u0"])
    print("phuber cost0", rel(c0, g["cost0"]))
    assert c0.shape == (2,) and rel(c0, g["cost0"]) < 1e-10


@pytest.mark.parametrize("n, m", [(4, 2), (9, 3)])
def test_coupled_expansion_against_numpy(n, m):
    """B = 5, N = 23 (no multiple of the steps a workgroup takes), per-trajectory parameters, non-zero Qr, Rr, an active mask:
    inactive rows keep their sentinel.  (9, 3) walks its 78 pairs in more than one sweep."""
    from isls import costs
    from isls import _capi as capi
    from isls.engine import kernels
    B, N = 5, 23
    rng = np.random.default_rng(n)
    x, u = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
    par = uc.COUPLED_PAR * (1.0 + 0.1 * rng.normal(size=(B, uc.COUPLED_PAR.size)))
    Qr, Rr = rng.normal(size=(1, n, n)), rng.normal(size=(1, m, m))
    cost, g, H = uc.coupled_numpy(x, u, par)
    H[..., :n, :n] += 2 * Qr
    H[..., n:, n:] += 2 * Rr
    cst = costs.Custom(n, m, par, uc.coupled_source(n, m))
    kern, dev = kernels(), torch.device("cuda")
    active = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32, device=dev)
    on = active.bool().cpu().numpy()
    res = {}
    for dt in (torch.float64, torch.float32):
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)   # noqa: E731
        capi.user_cost_load(cst.cost_model, -1, dt)
        out = dict(Cxx=(B, N, n, n), Cuu=(B, N, m, m), Cux=(B, N, m, n), c0x=(B, N, n), c0u=(B, N, m), cost=(B,))
        out = {k: torch.full(sh, 7.0, dtype=dt, device=dev) for k, sh in out.items()}
        zero = torch.zeros(1, n, n, dtype=dt, device=dev)
        exp = capi.Kernels.expand_args(zero, zero[0, :1], torch.zeros(N, dtype=torch.int32, device=dev), 0.0, out["c0x"], out["c0u"],
                                       xhat=t(x), uhat=t(u), Cxx=out["Cxx"], Cuu=out["Cuu"], Qr=t(Qr), Rr=t(Rr), cost=out["cost"],
                                       active=active, cost_model=cst.cost_model, cost_par=t(par))
        kern.user_cost_expand(exp, out["Cux"], "f64" if dt == torch.float64 else "f32")
        torch.cuda.synchronize()
        res[dt] = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
        for k, v in res[dt].items():
            assert (v[~on] == 7.0).all(), k                    # inactive trajectories: left untouched
    ref = dict(Cxx=H[..., :n, :n], Cuu=H[..., n:, n:], Cux=H[..., n:, :n], c0x=g[..., :n], c0u=g[..., n:], cost=cost)
    for k, r in ref.items():
        e64, e32 = rel(res[torch.float64][k][on], r[on]), rel(res[torch.float32][k][on], res[torch.float64][k][on])
        print(f"coupled ({n},{m}) {k}: fp64 {e64:.2e} fp32 vs fp64 {e32:.2e}")
        assert e64 < 1e-10 and e32 < 1e-4, k
    assert np.abs(ref["Cux"]).max() > 0.01 and np.abs(ref["Cxx"][..., 0, 1]).max() > 0.01   # cross and off-diagonal terms are there


# ---- 2. line search: a restatement against the built-in cost -------------------------------------------------------------------
def tassa_problem(g, B, seed=3):
    """g8's initial nominal with perturbed controls, rolled out again"""
    from isls import models
    mdl = models.TassaCar(float(g["dt"]), float(g["dist"]))
    rng = np.random.default_rng(seed)
    N = int(g["N"])
    u = g["u0"][np.arange(B) % 2] + 0.05 * rng.normal(size=(B, N, 2))
    x = np.zeros((B, N, 4))
    x[:, 0] = g["x0"][np.arange(B) % 2]
    for t in range(N - 1):
        x[:, t + 1] = mdl(x[:, t], u[:, t])
    return mdl, x, u


def tassa_isls(g, mdl, cost, x, u, dtype):
    from isls import iSLS
    s = iSLS(4, 2, int(g["N"]), batch=x.shape[0], dtype=dtype)
    s.forward_model = mdl
    s.cost_function = cost
    s.nominal_values = x, u
    return s


def share(src, dst, names):
    for k in names:
        getattr(dst, k).copy_(getattr(src, k))


def compare_searches(eb, ec, ca_b, ca_c, tol):
    """cost_new / cost_all within tol; best exact wherever the built-in's two smallest candidate costs are not a near tie"""
    B = ca_b.shape[0]
    cb, cc = ca_b.double().cpu().numpy(), ca_c.double().cpu().numpy()
    e_all, e_new = rel(cc, cb), rel(ec.cost_new.double().cpu().numpy(), eb.cost_new.double().cpu().numpy())
    srt = np.sort(cb, axis=1)
    clear = (srt[:, 1] - srt[:, 0]) > 1e-9 * np.maximum(1.0, np.abs(srt[:, 0]))
    print(f"line search: cost_all {e_all:.2e} cost_new {e_new:.2e}, {int((~clear).sum())} of {B} near ties")
    assert e_all < tol and e_new < tol
    assert (~clear).sum() <= 0.1 * B
    assert (eb.best.cpu().numpy()[clear] == ec.best.cpu().numpy()[clear]).all()


@pytest.mark.parametrize("dtype, tol", [(np.float64, 1e-12), (np.float32, 1e-4)])
def test_line_search_phuber_restatement_equals_builtin(golden, dtype, tol):
    """Pseudo-Huber on the Tassa car, B = 33 (three trajectories per wavefront, a partial last wavefront), L = 20; both sides on
    the same A, B, expansion and gains (the built-in's, copied)."""
    from isls import Box
    from isls import _capi as capi
    g = golden("g8_tassa.npz")
    B, L = 33, 20
    ph, cu = tassa_costs(g)
    mdl, x, u = tassa_problem(g, B)
    sb, sc = tassa_isls(g, mdl, ph, x, u, dtype), tassa_isls(g, mdl, cu, x, u, dtype)
    eb, ec = sb.engine, sc.engine
    assert rel(ec.cost.double().cpu().numpy(), eb.cost.double().cpu().numpy()) < tol
    sb._linearize(None)
    sb._expand()
    eb.gain(active=eb.outer_active)
    eb.feedforward(active=eb.outer_active)
    share(eb, ec, ("A", "Bm", "K", "k"))
    flags = capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST
    ca_b, ca_c = torch.zeros(B, L, dtype=eb.dtype, device=eb.device), torch.zeros(B, L, dtype=eb.dtype, device=eb.device)
    eb.rollout(L, flags=flags, cost_all=ca_b, active=eb.outer_active)
    ec.rollout(L, flags=flags, cost_all=ca_c, active=ec.outer_active)
    torch.cuda.synchronize()
    compare_searches(eb, ec, ca_b, ca_c, tol)
    same = (eb.best == ec.best)                                # the same winner: the same trajectory, bit for bit
    assert torch.equal(eb.xx[same], ec.xx[same]) and torch.equal(eb.xu[same], ec.xu[same])
    if dtype != np.float64:
        return
    # once through the outer driver with a control box: the fused ADMM update and the recorded winner
    box = Box(np.array([-0.5, -2.0]), np.array([0.5, 2.0]))
    for s in (sb, sc):
        s._setup_admm(False, box, None, np.diag([1e-1, 1e-2]), 1.0)
    sb._expand_regularised(None)
    sc._expand_regularised(None)                               # (its own expansion: Cux, here zeros, must exist for the gain block)
    share(eb, ec, ("Cxx", "Cuu", "c0x", "c0u"))
    outs = []
    for e in (eb, ec):
        e.build_outer(L, 4)
        e.run_outer()
        torch.cuda.synchronize()
        outs.append([t.clone().cpu().numpy() for t in (e.xx, e.xu, e.cost_new, e.zu, e.lu, e.res)])
    for i, (a, b) in enumerate(zip(*outs)):
        print("outer driver", i, rel(b, a))
        assert rel(b, a) < 1e-12, i
    assert (eb.best == ec.best).all() and (eb.admm_iters == ec.admm_iters).all()


@pytest.mark.parametrize("L", [20, 40])
def test_line_search_via_point_restatement_on_the_arm(L):
    """The via-point cost restated as a stage cost, on Planar3R (9, 3): B = 33, the same A, B and gains.  L = 20 runs the
    one-wave-per-SIMD kernels; L = 40 the two-wave ones, which with a user cost replay the winner on a ring of three operands.
    Either way the launch plan takes the row form of the replay (one control row per lane): at N = 40 the slot's LDS budget
    leaves both forms 8 segments of 5 steps, and the row form is kept unless it needs four times the iterations.  `best` is 0
    before the first search, so every trajectory that accepts another candidate has missed its prediction and is replayed."""
    from isls import _capi as capi
    from isls import costs, iSLS, models
    import isls_problems as P
    B, N = 33, 40
    cfg = P.config3(batch=B, N=N, seed=0)
    par = uc.VIA_ARM_PAR
    zs, Qs, seq, u_std = uc.via_arm_tables(par, N, **uc.VIA_ARM_W)
    mdl = models.Planar3R(cfg["dt"])
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in range(B)])
    rng = np.random.default_rng(5)
    us = np.stack(us) + 0.2 * rng.normal(size=(B, N, 3))
    xs = np.stack(xs)
    for t in range(N - 1):
        xs[:, t + 1] = mdl(xs[:, t], us[:, t])
    sides = []
    for custom in (False, True):
        s = iSLS(9, 3, N, batch=B)
        s.forward_model = mdl
        s.set_cost_variables(zs, Qs, seq, u_std)
        if custom:
            s.cost_function = costs.Custom(9, 3, par, uc.via_arm_source(**uc.VIA_ARM_W))
        s.nominal_values = xs, us
        sides.append(s)
    eb, ec = sides[0].engine, sides[1].engine
    assert rel(ec.cost.cpu().numpy(), eb.cost.cpu().numpy()) < 1e-12
    sides[0]._linearize(None)
    sides[0]._expand()
    sides[1]._expand()
    for k in ("c0x", "c0u", "Cxx", "Cuu"):                     # the hyper-dual expansion against the via-point tables'
        a = getattr(ec, k).cpu().numpy()
        b = (eb.hessians()[0 if k == "Cxx" else 1] if k in ("Cxx", "Cuu") else getattr(eb, k)).cpu().numpy()
        assert rel(a, np.broadcast_to(b, a.shape)) < 1e-10, k
    assert float(ec.Cux.abs().max()) == 0.0
    eb.gain(active=eb.outer_active)
    eb.feedforward(active=eb.outer_active)
    share(eb, ec, ("A", "Bm", "K", "k"))
    ca_b, ca_c = torch.zeros(B, L, dtype=eb.dtype, device=eb.device), torch.zeros(B, L, dtype=eb.dtype, device=eb.device)
    flags = capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST
    eb.rollout(L, flags=flags, cost_all=ca_b, active=eb.outer_active)
    ec.rollout(L, flags=flags, cost_all=ca_c, active=ec.outer_active)
    torch.cuda.synchronize()
    compare_searches(eb, ec, ca_b, ca_c, 1e-12)
    # the winner replay: the same winner gives the same trajectory, bit for bit (same model, gains and operand order)
    same = (eb.best == ec.best)
    replayed = same & (eb.best != 0) & ((eb.status & capi.ST_LS_REJECT) == 0)
    print(f"arm L={L}: {int(replayed.sum())} of {B} trajectories replayed after a missed prediction")
    assert int(replayed.sum()) >= B // 2
    assert torch.equal(eb.xx[same], ec.xx[same]) and torch.equal(eb.xu[same], ec.xu[same])
    assert not torch.equal(ec.xx[replayed], ec.xhat[replayed])  # (and it is the winner, not the nominal handed back)


def test_line_search_with_a_model_and_a_cost_of_the_same_id_number():
    """A Custom car and the coupled cost registered under the same id number (the two kinds count their ids independently), fp64,
    B = 5, N = 6, L = 20: three trajectories per wavefront, the second wavefront partial.  One launcher serves the three kinds
    of program and picks each by (model, cost): (a) the Custom car with the via-point cost gives the built-in car's bits;
    (c) the coupled cost with the Custom car gives the bits of (b) the coupled cost with the built-in car -- the same template
    with the same arithmetic, on the same A, B and gains ((b)'s, copied).  (Measured with the two launchers this one replaced:
    (c) and (b) bit-identical in best, xx, xu and cost_new, so bit identity is what is asserted.)"""
    from isls import _capi as capi
    from isls import iSLS, models
    import isls_problems as P
    B, N, L = 5, 6, 20
    cfg = P.config4(batch=B, N=N, seed=0)
    builtin = models.CarSimple(cfg["dt"])
    custom, coupled = uc.same_id_pair((4, 2, [cfg["dt"]], um.CAR), (4, 2, uc.COUPLED_PAR, uc.coupled_source(4, 2)))
    assert custom.model_id == coupled.cost_model
    xs, us = (np.stack(v) for v in zip(*[P.initial_nominal(cfg, b) for b in range(B)]))

    def search(model, cost, gains_of=None):
        s = iSLS(4, 2, N, batch=B)
        s.forward_model = model
        s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
        if cost is not None:
            s.cost_function = cost
        s.reset()
        s.nominal_values = xs, us
        e = s.engine
        if gains_of is None:
            s._linearize(lambda x, u: builtin.get_AB(x, u))     # (a callable: the host route, the same A, B for every side)
            s._expand()
            e.gain(active=e.outer_active)
            e.feedforward(active=e.outer_active)
        else:
            share(gains_of, e, ("A", "Bm", "K", "k"))
        e.rollout(L, flags=capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST, active=e.outer_active)
        torch.cuda.synchronize()
        return e

    def same_bits(ea, eb, what):
        for k in ("best", "xx", "xu", "cost_new"):
            a, b = getattr(ea, k), getattr(eb, k)
            print(f"{what}: {k} differs by at most {(a.double() - b.double()).abs().max().item():.3e}")
        for k in ("best", "xx", "xu", "cost_new"):
            a, b = getattr(ea, k), getattr(eb, k)
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                               b.view(torch.int64) if b.dtype == torch.float64 else b), (what, k)

    e0, ea = search(builtin, None), search(custom, None)
    eb = search(builtin, coupled)
    ec = search(custom, coupled, gains_of=eb)
    same_bits(ea, e0, "(a) Custom car, via-point cost, against the built-in car")
    same_bits(ec, eb, "(c) coupled cost on the Custom car against (b) on the built-in car")
    assert torch.isfinite(e0.xx).all() and torch.isfinite(eb.xx).all()
    assert not torch.equal(eb.cost_new, e0.cost_new)           # (the two costs are two costs)


def test_second_derivatives_of_every_operation():
    """Every second-order rule of the hyper-dual type (sin cos sqrt exp log tanh asin atan2 fabs, division, isls::sin_cos,
    isls::py_mod, compound assignment, mixed operands) on the device: the Hessian of a cost that uses them all against central
    differences of the device gradient, and the gradient against central differences of the device value.  Step h = 1e-5 on
    arguments of order one: truncation h^2 / 6 times the third derivative of what is differenced ~ 1e-10 of its scale, rounding
    eps / h ~ 1e-11; the bound 1e-6 relative leaves both orders of magnitude of room and catches any wrong coefficient or sign."""
    from isls import costs
    from test_user_cost_host import EVERY_OP
    n, m, N, h = 4, 2, 12, 1e-5
    rng = np.random.default_rng(11)
    x, u = rng.uniform(0.3, 1.3, size=(N, n)), rng.uniform(0.3, 1.3, size=(N, m))      # away from the kinks of fabs / py_mod / the branch
    x[:, 2] = rng.uniform(0.2, 0.8, N)                          # x2 < x3, py_mod(x2, 2) away from its jump
    x[:, 3] = rng.uniform(1.1, 1.6, N)
    cst = costs.Custom(n, m, [0.5], EVERY_OP)
    cs, Cs = cst.get_Cs(x, u)
    w = np.concatenate([x, u], axis=-1)
    assert np.abs(Cs - np.swapaxes(Cs, -1, -2)).max() <= 1e-12 * np.abs(Cs).max()
    K = n + m
    wp, wm = np.repeat(w[None], K, 0), np.repeat(w[None], K, 0)    # [K, N, K]: direction k perturbed at every step at once
    for k in range(K):
        wp[k, :, k] += h
        wm[k, :, k] -= h
    gp, _ = cst.get_Cs(wp[..., :n], wp[..., n:])
    gm, _ = cst.get_Cs(wm[..., :n], wm[..., n:])
    fd_H = np.moveaxis((gp - gm) / (2 * h), 0, -1)                 # [N, K (entry), K (direction)]
    print("every op: Hessian vs central differences", rel(Cs, fd_H), "scale", np.abs(Cs).max())
    assert np.abs(Cs - fd_H).max() < 1e-6 * max(1.0, np.abs(Cs).max())
    assert (np.abs(Cs).max(axis=0) > 1e-3).all()               # every entry pair is exercised
    # the gradient: per step, so perturb one step at a time through the value (a sum over the steps)
    for t in (0, N - 1):
        for k in range(K):
            a, b = w.copy(), w.copy()
            a[t, k] += h
            b[t, k] -= h
            fd = (cst(a[:, :n], a[:, n:]) - cst(b[:, :n], b[:, n:])) / (2 * h)
            assert abs(fd - cs[t, k]) < 1e-6 * max(1.0, np.abs(cs).max()), (t, k, fd, cs[t, k])


def test_batch_form_is_refused_with_a_user_cost(golden):
    """The batch-form iLQR goes through the column roll-out, which takes Cuu alone: refused, not computed without Cux."""
    from isls import iSLS, models
    g = golden("g8_tassa.npz")
    s = iSLS(4, 2, int(g["N"]), batch=2)
    s.forward_model = models.TassaCar(float(g["dt"]), float(g["dist"]))
    s.cost_function = tassa_costs(g)[1]
    s.nominal_values = g["x_nom0"], g["u0"]
    with pytest.raises(Exception, match="batch-form"):
        s.solve(method='batch', max_iter=1)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
def test_tassa_car_parking_with_a_custom_cost(golden):
    """test_isls_api.test_tassa_car_parking_api with costs.Custom in place of costs.PseudoHuber and no get_Cs."""
    from isls import Box, iSLS, models
    g = golden("g8_tassa.npz")
    _, cost = tassa_costs(g)
    mdl = models.TassaCar(float(g["dt"]), float(g["dist"]))

    def fresh():
        s = iSLS(4, 2, int(g["N"]), batch=2)
        s.forward_model = mdl
        s.cost_function = cost
        s.nominal_values = g["x_nom0"], g["u0"]
        return s
    s = fresh()
    assert rel(s.cost, g["cost0"]) < 1e-12
    s.solve(max_iter=6, max_line_search_iter=40, method='dp')
    print("tassa solve", rel(s.cost, g["cost_log"][:, 6]), rel(s.x_nom, g["x_fin"]), rel(s.u_nom, g["u_fin"]))
    assert rel(s.cost, g["cost_log"][:, 6]) < 1e-7 and rel(s.x_nom, g["x_fin"]) < 1e-5 and rel(s.u_nom, g["u_fin"]) < 1e-5
    s = fresh()
    s.ilqr_admm(project_u=Box(np.array([-0.5, -2.0]), np.array([0.5, 2.0])), max_iter=3,
                max_line_search_iter=40, max_admm_iter=5, rho_u=np.diag([1e-1, 1e-2]), tol=0.0)
    _check_final(s, g, "o2", [0, 1], 3, 5, {k: 1e-7 for k in ("xx", "xu", "K", "cost")})
    with pytest.raises(Exception, match="isls_admm does not serve a user cost"):
        s.isls_admm(2)


def quad_sides(batch, N=40):
    """The coupled cost on the models.Custom quadrotor: (device iSLS, host iSLS, get_AB, get_Cs) on the same problem"""
    from isls import costs, iSLS, models
    from test_user_model_gpu import quad_problem
    pb = quad_problem(batch, N)
    f, get_AB = um.quad_numpy()
    par = uc.COUPLED_PAR
    host_cost = lambda x, u: uc.coupled_numpy(x, u, par)[0]    # noqa: E731
    get_Cs = lambda x, u: uc.coupled_numpy(x, u, par)[1:]      # noqa: E731
    xs = np.zeros((batch, N, 6))
    xs[:, 0] = pb["x0"]
    for t in range(N - 1):
        xs[:, t + 1] = f(xs[:, t], pb["u0"][:, t])
    out = []
    for host in (False, True):
        s = iSLS(6, 2, N, batch=batch)
        s.forward_model = (lambda x, u: f(x, u)) if host else models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
        s.cost_function = host_cost if host else costs.Custom(6, 2, par, uc.coupled_source(6, 2))
        s.reset()
        s.nominal_values = xs, pb["u0"]
        out.append(s)
    return out[0], out[1], get_AB, get_Cs


def test_coupled_cost_on_the_quadrotor_matches_the_host_path():
    from isls import Box
    box = Box(np.array([0.0, 0.0]), np.array([8.0, 8.0]))
    d, h, get_AB, get_Cs = quad_sides(3)
    assert rel(d.cost, h.cost) < 1e-12
    d.solve(max_iter=4, max_line_search_iter=20)
    h.solve(get_AB, get_Cs, max_iter=4, max_line_search_iter=20)
    print("quad solve", rel(d.x_nom, h.x_nom), rel(d.u_nom, h.u_nom), rel(d.cost, h.cost))
    assert rel(d.x_nom, h.x_nom) < 1e-9 and rel(d.u_nom, h.u_nom) < 1e-9 and rel(d.cost, h.cost) < 1e-9
    assert float(d.engine.Cux.abs().max()) > 0.0
    d, h, get_AB, get_Cs = quad_sides(3)
    d.ilqr_admm(project_u=box, max_iter=3, max_line_search_iter=20, max_admm_iter=5, rho_u=0.1, tol=0.0)
    h.ilqr_admm(get_AB, get_Cs, project_u=box, max_iter=3, max_line_search_iter=20, max_admm_iter=5, rho_u=0.1, tol=0.0)
    print("quad ilqr_admm", rel(d.x_nom, h.x_nom), rel(d.u_nom, h.u_nom), rel(d.cost, h.cost))
    assert rel(d.x_nom, h.x_nom) < 1e-9 and rel(d.u_nom, h.u_nom) < 1e-9 and rel(d.cost, h.cost) < 1e-9
    assert (d.status == 0).all()


def test_coupled_cost_timed_driver_with_advance():
    """build_outer(begin_done=True) / run_outer / advance() (the advance runs without a fused expansion and the user expansion
    follows it) equal the launch-by-launch sequence accept_x_step, linearize, expand."""
    from isls import Box
    box = Box(np.array([0.0, 0.0]), np.array([8.0, 8.0]))
    outs = []
    for timed in (True, False):
        s = quad_sides(6)[0]
        s._setup_admm(False, box, None, 0.1, 1.0)
        s._linearize(None)
        s._expand_regularised(None)
        e = s.engine
        if timed:
            e.begin_outer()
            e.build_outer(20, 4, begin_done=True)
            for _ in range(2):
                e.run_outer()
                e.advance()
        else:
            e.build_outer(20, 4)
            for _ in range(2):
                e.run_outer()
                e.accept_x_step()
                e.linearize()
                e.expand()
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (e.xhat, e.uhat, e.cost, e.A, e.Bm, e.c0x, e.c0u, e.Cxx, e.Cuu, e.Cux, e.K, e.k)])
    for i, (a, b) in enumerate(zip(*outs)):
        assert rel(a.cpu().numpy(), b.cpu().numpy()) < 1e-12, i
