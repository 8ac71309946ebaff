#!/usr/bin/env python3
"""Built-in CarSimple against the same car written as an isls.models.Custom source, at config 4 shapes (B = 4096, N = 200,
L = 20, J = 5, control box + the two keep-out rectangles).

    python tools/user_model_bench.py [--batch 4096] [--reps 20]

* line search: ONE engine, the same K, k, nominal and ADMM targets; the rollout launch with the built-in model id and with the
  user model id alternate, outputs compared bit for bit;
* outer iteration (run_outer + advance, the step bench.py times): two engines, built-in and Custom, alternating.  The built-in
  car gets the model-structured passes (lean records) by default; it is also timed in the general layout the Custom model runs
  (use_model_structure = False), which isolates what the model itself costs.  Outputs compared to rounding (the Jacobians come
  from closed forms on one side and dual numbers on the other);
* the run-time compile of the Custom source (fp64, fresh source) and one `solve` iteration of the host slow path (the car as a
  numpy callable plus get_AB) at a small batch, for contrast.
`--legs table` times the per-step table of a models.Custom instead: the car with its constants in `params` against the same car
reading them from a shared [N, 2] table and from a [B, N, 2] table (table_legs).
Prints the numbers and one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ilqr-admm_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import isls_problems as P  # noqa: E402
import user_models as um  # noqa: E402


def make(cfg, B, model, structure=True):
    import isls
    from isls import Box
    pj = sys.modules["isls.projections"]
    s = isls.iSLS(4, 2, cfg["N"], batch=B)
    s.forward_model = model
    s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in range(B)])
    s.reset()
    s.nominal_values = np.stack(xs), np.stack(us)
    N = cfg["N"]
    rho_x = np.zeros((N, 4, 4)); rho_x[:, :2, :2] = 0.1 * np.eye(2)
    cs = pj.keepout_rectangles(4, [[-7.0, -3.0], [-3.0, -7.0]], [[2.0, 1.0], [2.0, 1.0]], -np.pi / 4)
    s._setup_admm(cs, Box(cfg["u_lo"], cfg["u_hi"]), rho_x, cfg["rho_u"], 1.0)
    e = s.engine
    e.use_model_structure = structure
    e.outer_active.fill_(1)
    e.build_outer(20, 5, tol_abs=0.0, tol_rel=0.0, begin_done=True)
    e.linearize(); e.expand(); e.begin_outer()
    return s


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps            # us per call


def car_with_push(c, table):
    """The car of tests/user_models.py with two constants c[0] = dt and c[1] = a lateral push, read from `par` or from `row`: the
    same arithmetic either way, so the forms differ in where the two words come from and in nothing else."""
    sig = "const P *par, const P *row, S *xn" if table else "const P *par, S *xn"
    return f"""template <typename S, typename P>
__device__ void step(const S *x, const S *u, {sig}) {{
    const P dt = {c}[0];
    S sn, cs;
    isls::sin_cos(x[2], sn, cs);
    xn[0] = x[0] + dt * x[3] * cs;
    xn[1] = x[1] + dt * x[3] * sn + {c}[1];
    xn[2] = isls::py_mod(x[2] + dt * x[3] * u[0], P(2 * 3.14159265358979323846));
    xn[3] = x[3] + dt * u[1];
}}"""


def table_legs(args):
    """--legs table: the car with its constants in `params`, with a shared [N, 2] table (row = [dt, lateral push 0]) and with a
    [B, N, 2] table of the same rows, one engine each from the same start; the rollout launch and the outer iteration of the
    three alternate within this call.  The yardstick is the params form of the same call."""
    from isls import models
    B, N = args.batch, 200
    cfg = P.config4(batch=B, N=N, seed=0)
    rows = np.tile([cfg["dt"], 0.0], (N, 1))
    forms = {"params": models.Custom(4, 2, rows[0], car_with_push("par", False)),
             "table_shared": models.Custom(4, 2, [0.0], car_with_push("row", True), table=rows),
             "table_per_traj": models.Custom(4, 2, [0.0], car_with_push("row", True), table=np.broadcast_to(rows, (B, N, 2)).copy())}
    eng = {k: make(cfg, B, mdl).engine for k, mdl in forms.items()}
    for x in eng.values():                            # realistic K, k and ADMM targets, the same for the three
        x.run_outer()
    torch.cuda.synchronize()
    best0 = {k: x.best.clone() for k, x in eng.items()}

    def ls(k):
        eng[k].best.copy_(best0[k])
        eng[k].rollout(20)
    outs = {}
    for k in eng:
        ls(k)
        torch.cuda.synchronize()
        outs[k] = [t.clone() for t in (eng[k].xx, eng[k].xu, eng[k].cost_new, eng[k].best)]
    ls_equal = {k: all(torch.equal(a, b) for a, b in zip(outs["params"], outs[k])) for k in eng if k != "params"}
    ls_t, ot = {k: [] for k in eng}, {k: [] for k in eng}
    for _ in range(args.rounds):
        for k in eng:
            ls(k)
            ls_t[k].append(timed(lambda: ls(k), args.reps))

    def outer(x):
        x.run_outer()
        x.advance()
    for _ in range(args.rounds):
        for k, x in eng.items():
            ot[k].append(timed(lambda: outer(x), max(1, args.reps // 4)))
    med = lambda v: float(np.median(v))               # noqa: E731
    spread = lambda v: float(np.max(v) - np.min(v))   # noqa: E731
    res = dict(legs="table", batch=B, N=N, L=20, J=5, rounds=args.rounds,
               ls_us={k: med(v) for k, v in ls_t.items()}, ls_spread_us={k: spread(v) for k, v in ls_t.items()},
               ls_bitwise_equal_to_params=ls_equal,
               outer_us={k: med(v) for k, v in ot.items()}, outer_spread_us={k: spread(v) for k, v in ot.items()})
    for k in eng:
        print(f"{k:15s} B={B}: line search {res['ls_us'][k]:.1f} us (spread {res['ls_spread_us'][k]:.1f}), outer iteration "
              f"{res['outer_us'][k]:.1f} us (spread {res['outer_spread_us'][k]:.1f})")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", choices=["model", "table"], default="model",
                    help="model: built-in against Custom (the default); table: params form against the two table forms")
    args = ap.parse_args()
    from isls import models
    torch.cuda.set_device(0)
    if args.legs == "table":
        if args.rounds < 5:
            ap.error("--legs table alternates the forms over at least 5 rounds")
        return table_legs(args)
    B = args.batch
    cfg = P.config4(batch=B, N=200, seed=0)
    dt = cfg["dt"]

    # run-time compile of a source this process has not seen (fp64 at create, fp32 on first use; one load onto the device)
    t0 = time.perf_counter()
    car = models.Custom(4, 2, [dt], um.CAR + f"\n// {os.getpid()} {time.time_ns()}\n")
    t_compile = time.perf_counter() - t0
    t0 = time.perf_counter()
    from isls import _capi as capi
    capi.user_model_load(car.model_id, np.float64)
    t_load = time.perf_counter() - t0

    # ---- line search: one engine, the two model ids alternate on identical inputs
    s = make(cfg, B, models.CarSimple(dt))
    e = s.engine
    e.run_outer()                                     # realistic K, k and ADMM targets
    torch.cuda.synchronize()
    ids = {"builtin": (models.CarSimple.model_id, e.model_par), "custom": (car.model_id, e.model_par)}
    best0 = e.best.clone()

    def ls(which):
        e.model = ids[which][0]
        e.best.copy_(best0)
        e.rollout(20)
    outs = {}
    for which in ("builtin", "custom"):
        ls(which)
        torch.cuda.synchronize()
        outs[which] = [t.clone() for t in (e.xx, e.xu, e.cost_new, e.best)]
    ls_equal = all(torch.equal(a, b) for a, b in zip(outs["builtin"], outs["custom"]))
    ls_t = {"builtin": [], "custom": []}
    for _ in range(args.rounds):
        for which in ("builtin", "custom"):
            ls(which)
            ls_t[which].append(timed(lambda: ls(which), args.reps))
    e.model = models.CarSimple.model_id

    # ---- outer iteration: run_outer + advance on three engines, alternating
    eng = {"builtin": make(cfg, B, models.CarSimple(dt)).engine,
           "builtin_general": make(cfg, B, models.CarSimple(dt), structure=False).engine,
           "custom": make(cfg, B, car).engine}

    def outer(x):
        x.run_outer()
        x.advance()
    for x in eng.values():                            # one iteration each from the same start, outputs compared
        outer(x)
    torch.cuda.synchronize()
    ref = eng["builtin_general"]
    dev = max(float(((eng["custom"].xhat - ref.xhat).abs().max() / ref.xhat.abs().max()).item()),
              float(((eng["custom"].uhat - ref.uhat).abs().max() / ref.uhat.abs().max()).item()))
    ot = {k: [] for k in eng}
    for _ in range(args.rounds):
        for k, x in eng.items():
            ot[k].append(timed(lambda: outer(x), max(1, args.reps // 4)))

    # ---- host slow path at a small batch: the car as numpy callables, one solve iteration
    hb = 4
    hcfg = P.config4(batch=hb, N=200, seed=0)
    f = models.CarSimple(dt)
    import isls
    h = isls.iSLS(4, 2, 200, batch=hb)
    h.forward_model = lambda x, u: f(x, u)
    h.set_cost_variables(hcfg["zs"], hcfg["Qs"], hcfg["seq"], hcfg["u_std"])
    xs, us = zip(*[P.initial_nominal(hcfg, b) for b in range(hb)])
    h.reset()
    h.nominal_values = np.stack(xs), np.stack(us)
    t0 = time.perf_counter()
    h.solve(lambda x, u: f.get_AB(x, u), max_iter=1, max_line_search_iter=20)
    torch.cuda.synchronize()
    t_host = time.perf_counter() - t0

    med = lambda v: float(np.median(v))               # noqa: E731
    spread = lambda v: float(np.max(v) - np.min(v))   # noqa: E731
    res = dict(batch=B, N=200, L=20, J=5,
               ls_us={k: med(v) for k, v in ls_t.items()}, ls_spread_us={k: spread(v) for k, v in ls_t.items()},
               ls_bitwise_equal=ls_equal,
               outer_us={k: med(v) for k, v in ot.items()}, outer_spread_us={k: spread(v) for k, v in ot.items()},
               outer_custom_vs_general_rel=dev,
               compile_s=round(t_compile, 2), load_s=round(t_load, 3),
               host_path_solve_iter_s_b4=round(t_host, 3))
    print(f"line search  B={B}: built-in {res['ls_us']['builtin']:.1f} us, Custom {res['ls_us']['custom']:.1f} us "
          f"(spread {res['ls_spread_us']['builtin']:.1f} / {res['ls_spread_us']['custom']:.1f}), bitwise equal: {ls_equal}")
    print(f"outer iter   B={B}: built-in {res['outer_us']['builtin']:.1f} us (structured), {res['outer_us']['builtin_general']:.1f} us "
          f"(general layout), Custom {res['outer_us']['custom']:.1f} us; Custom vs general nominal rel {dev:.1e}")
    print(f"compile {t_compile:.1f} s, load {t_load:.3f} s; host slow path, one solve iteration at B={hb}: {t_host:.2f} s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
