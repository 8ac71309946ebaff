#!/usr/bin/env python
"""Receding-horizon control at the headline problem (B = 4096, N = 100, n = 6, m = 3, J = 5, L = 20, double integrator, one
outer iteration per control step): control steps per second of iSLS.mpc, the median time of the isls_mpc_step launch alone and
of one outer iteration of the same problem (run_outer + advance) from HIP events, and the same number of control steps driven the
way the code before iSLS.mpc allows: ilqr_admm(max_iter=1), the plant and the shift in numpy, the nominal_values setter.

    python tools/mpc_bench.py [--batch 4096] [--steps 20] [--blocks 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ilqr-admm_amd"))

import isls                                                      # noqa: E402
import isls_problems as P                                        # noqa: E402
from isls import Box, models                                     # noqa: E402

J, L = 5, 20


def solver(B, N):
    cfg = P.config2(batch=B, N=N, seed=0)
    s = isls.iSLS(6, 3, N, batch=B)
    s.forward_model = models.LTI(cfg["A"], cfg["B"])
    s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in range(B)])
    s.reset()
    s.nominal_values = np.stack(xs), np.stack(us)
    return s, cfg


def admm(cfg):
    return dict(project_u=Box(cfg["u_lo"], cfg["u_hi"]), rho_u=cfg["rho_u"], max_admm_iter=J, max_line_search_iter=L)


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    B, N, T = a.batch, a.horizon, a.steps

    # ---- the loop on the device ----------------------------------------------------------------------------------------------
    q, cfg = solver(B, N)
    q.mpc(steps=2, iters=1, **admm(cfg))                        # warm-up: modules, buffers, the gain memo
    times = []
    for _ in range(a.blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q.mpc(steps=T, iters=1, **admm(cfg))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    mpc_s = float(np.median(times))

    # ---- the launch alone, and one outer iteration of the same problem --------------------------------------------------------
    e = q.engine
    step_ms = [event_ms(lambda: e.kern.mpc_step(e.model, e.model_par, e.xhat, e.uhat, K=e.K,
                                                stream=torch.cuda.current_stream().cuda_stream), 10) for _ in range(a.blocks)]
    q2, _ = solver(B, N)
    q2.ilqr_admm(max_iter=1, **admm(cfg))
    e2 = q2.engine
    e2.linearize(), e2.expand()
    e2.build_outer(L, J, tol_abs=1e-3, tol_rel=1e-3, begin_done=True)
    e2.begin_outer()

    def outer():
        e2.run_outer()
        e2.advance()
    outer()
    outer_ms = [event_ms(outer, 10) for _ in range(a.blocks)]

    # ---- the route without iSLS.mpc: host plant, numpy shift, nominal_values setter ---------------------------------------
    h, _ = solver(B, N)
    A, Bm = cfg["A"], cfg["B"]

    def host_steps(n_steps):
        for _ in range(n_steps):
            h.ilqr_admm(max_iter=1, **admm(cfg))
            x, u = h.x_nom, h.u_nom
            x_next = x[:, 0] @ A.T + u[:, 0] @ Bm.T
            u = np.concatenate([u[:, 1:], u[:, -1:]], axis=1)
            xs = np.empty_like(x)
            xs[:, 0] = x_next
            for t in range(N - 1):
                xs[:, t + 1] = xs[:, t] @ A.T + u[:, t] @ Bm.T
            h.nominal_values = xs, u
    host_steps(2)
    times = []
    for _ in range(max(3, a.blocks // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_steps(T)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    host_s = float(np.median(times))

    out = dict(batch=B, horizon=N, steps=T, J=J, L=L, blocks=a.blocks,
               mpc_steps_per_s=T / mpc_s, mpc_ms_per_step=1e3 * mpc_s / T,
               mpc_step_launch_us=1e3 * float(np.median(step_ms)), outer_iteration_us=1e3 * float(np.median(outer_ms)),
               host_route_steps_per_s=T / host_s, host_route_ms_per_step=1e3 * host_s / T, speedup=host_s / mpc_s)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
