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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from isls import models
    torch.cuda.set_device(0)
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
