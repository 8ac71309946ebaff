#!/usr/bin/env python3
"""Built-in PseudoHuber against the same cost written as an isls.costs.Custom source, on the Tassa parking problem (N = 100,
L = 20, J = 5, control box) at B = 4096.

    python tools/user_cost_bench.py [--batch 4096] [--reps 20] [--rounds 5] [--legs phuber,arm,table,host,al]

Two engines on the same problem, the forms alternating over the rounds (medians; spread = max - min over the rounds):
* one rollout launch (the line search of the ADMM iteration, same gains and ADMM targets on both sides);
* one expansion launch (built-in: expand_kernel; Custom: user_expand_kernel, which also writes Cux);
* one outer iteration: run_outer, then accept_x_step + linearize + expand on both sides (the built-in pseudo-Huber cost has
  per-trajectory Hessians, which Engine.advance() does not serve), and for the Custom cost also run_outer + advance();
* the 3R arm (9, 3) at L = 40 candidates, built-in via-point cost against its Custom restatement, one rollout launch with the
  prediction reset before each (every winner is replayed): the two-waves-per-SIMD kernels, whose replay keeps three operand
  sets in flight with a user cost and four without;
* a tracking cost (tests/table_costs.py) in three forms on the Tassa shapes, one rollout launch and one expansion launch each:
  a constant reference folded into `params` (what a cost without a table can hold), the same reference as a shared [N, W]
  table, and as a [B, N, W] table -- what the row's way through the line search (fetched two steps ahead, staged in LDS) and
  the expansion's global reads of it cost;
* a cost with K = 3 path constraints (tests/al_reference.py, costs.Custom(constraints=3)) against the same stage without them on
  the Tassa shapes, non-zero multipliers: one rollout launch and one expansion launch each -- what the augmented-Lagrangian terms
  cost --, and one multiplier update launch (isls_user_constraint_update_*);
* the run-time compile of the Custom source (fresh source: registration with the expansion, then the program with the Tassa
  rollout kernels) and one `solve` iteration of the host slow path (the cost as numpy callables + get_Cs) at a small batch.
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

import al_reference as al  # noqa: E402
import table_costs as tc  # noqa: E402
import user_costs as uc  # noqa: E402


def problem(B, seed=3):
    from isls import models
    g = np.load(os.path.join(ROOT, "tests", "golden", "g8_tassa.npz"))
    mdl = models.TassaCar(float(g["dt"]), float(g["dist"]))
    rng = np.random.default_rng(seed)
    N = int(g["N"])
    u = g["u0"][np.arange(B) % 2] + 0.05 * rng.normal(size=(B, N, 2))
    x = np.zeros((B, N, 4))
    x[:, 0] = g["x0"][np.arange(B) % 2]
    for t in range(N - 1):
        x[:, t + 1] = mdl(x[:, t], u[:, t])
    return g, mdl, x, u


def make(g, mdl, cost, x, u, begin_done):
    from isls import Box, iSLS
    s = iSLS(4, 2, int(g["N"]), batch=x.shape[0])
    s.forward_model = mdl
    s.cost_function = cost
    s.nominal_values = x, u
    s._setup_admm(False, Box(np.array([-0.5, -2.0]), np.array([0.5, 2.0])), None, np.diag([1e-1, 1e-2]), 1.0)
    e = s.engine
    e.outer_active.fill_(1)
    e.linearize(); e.expand(); e.begin_outer()
    e.build_outer(20, 5, tol_abs=0.0, tol_rel=0.0, begin_done=begin_done)
    return s


def arm_section(a, out, N=100, L=40):
    import isls_problems as P
    from isls import costs, iSLS, models
    cfg = P.config3(batch=a.batch, N=N, seed=0)
    mdl = models.Planar3R(cfg["dt"])
    zs, Qs, seq, u_std = uc.via_arm_tables(uc.VIA_ARM_PAR, N, **uc.VIA_ARM_W)
    xs, us = zip(*[P.initial_nominal(cfg, b) for b in range(a.batch)])
    engines = []
    for custom in (False, True):
        s = iSLS(9, 3, N, batch=a.batch)
        s.forward_model = mdl
        s.set_cost_variables(zs, Qs, seq, u_std)
        if custom:
            s.cost_function = costs.Custom(9, 3, uc.VIA_ARM_PAR, uc.via_arm_source(**uc.VIA_ARM_W))
        s.nominal_values = np.stack(xs), np.stack(us)
        e = s.engine
        e.linearize(); e.expand(); e.gain(); e.feedforward()
        engines.append(e)

    def launch(e):
        e.best.zero_()                                         # the prediction misses: the winner is replayed
        e.rollout(L)
    runs = [[], []]
    for e in engines:
        timed(lambda: launch(e), 3)
    for _ in range(a.rounds):
        for i, e in enumerate(engines):
            runs[i].append(timed(lambda: launch(e), a.reps))
    replayed = [int((e.best != 0).sum()) for e in engines]
    for i, label in enumerate(("builtin", "custom")):
        out[f"arm_L40_rollout_{label}_us"] = [float(np.median(runs[i])), float(max(runs[i]) - min(runs[i]))]
        print(f"arm L=40 rollout {label:8s} median {np.median(runs[i]):9.1f} us  spread {max(runs[i]) - min(runs[i]):7.1f}  "
              f"({replayed[i]} of {a.batch} winners replayed)")


def table_section(a, out, g, mdl, x, u):
    from isls import costs
    N, B = int(g["N"]), a.batch
    row = np.array([0.5, -0.5, 0.3, 1.0, 1.0, 1.2, 0.8, 0.6])   # z (4), diag Q (4): the same reference at every step
    u_std = 0.01
    forms = {"params": costs.Custom(4, 2, np.concatenate([[u_std], row]), tc.params_source(4, 2, row)),
             "table_shared": costs.Custom(4, 2, [u_std], tc.tracking_source(4, 2), table=np.tile(row, (N, 1))),
             "table_batch": costs.Custom(4, 2, [u_std], tc.tracking_source(4, 2), table=np.tile(row, (B, N, 1)))}
    engines = {}
    for k, c in forms.items():
        e = make(g, mdl, c, x, u, False).engine
        e.gain(active=e.admm_active); e.feedforward(active=e.admm_active)
        engines[k] = e
    costs0 = [e.cost.cpu().numpy() for e in engines.values()]
    assert all(np.allclose(c, costs0[0], rtol=1e-12) for c in costs0)   # the three forms are the same cost
    for what, fn in (("rollout", lambda e: e.rollout(20, active=e.admm_active)), ("expand", lambda e: e.expand())):
        runs = {k: [] for k in engines}
        for e in engines.values():
            timed(lambda: fn(e), 3)
        for _ in range(a.rounds):
            for k, e in engines.items():
                runs[k].append(timed(lambda: fn(e), a.reps))
        for k, r in runs.items():
            out[f"tracking_{what}_{k}_us"] = [float(np.median(r)), float(max(r) - min(r))]
            print(f"tracking {what:8s} {k:13s} median {np.median(r):9.1f} us  spread {max(r) - min(r):7.1f}")


def al_section(a, out, g, mdl, x, u):
    from isls import costs
    K, B = 3, a.batch
    forms = {"plain": costs.Custom(4, 2, al.PAR, al.full_source(4, 2, 0, K, constraints=False)),
             "constraints": costs.Custom(4, 2, al.PAR, al.full_source(4, 2, 0, K), constraints=K)}
    engines = {}
    for k, c in forms.items():
        s = make(g, mdl, c, x, u, False)
        e = s.engine
        if k == "constraints":                                 # multipliers that stand: both branches of the PHR form are taken
            e.cost_tab[..., :K] = 0.1
            e.cost_tab[..., K] = 1.0
            e.evaluate_cost()
        e.gain(active=e.admm_active); e.feedforward(active=e.admm_active)
        engines[k] = e
    for what, fn in (("rollout", lambda e: e.rollout(20, active=e.admm_active)), ("expand", lambda e: e.expand())):
        runs = {k: [] for k in engines}
        for e in engines.values():
            timed(lambda: fn(e), 3)
        for _ in range(a.rounds):
            for k, e in engines.items():
                runs[k].append(timed(lambda: fn(e), a.reps))
        for k, r in runs.items():
            out[f"al_{what}_{k}_us"] = [float(np.median(r)), float(max(r) - min(r))]
            print(f"al {what:8s} {k:13s} median {np.median(r):9.1f} us  spread {max(r) - min(r):7.1f}")
    e = engines["constraints"]
    viol, prev = torch.zeros(B, dtype=e.dtype, device=e.device), torch.full((B,), float("inf"), dtype=e.dtype, device=e.device)
    keep = e.cost_tab.clone()

    def update():
        e.kern.user_constraint_update(e.cost_model, e.cost_par, e.cost_tab, e.xhat, e.uhat, viol, prev, update=True, eta=0.25, phi=1.0,
                                      mu_max=1e8, stream=torch.cuda.current_stream().cuda_stream)
    timed(update, 3)
    r = [timed(update, a.reps) for _ in range(a.rounds)]
    e.cost_tab.copy_(keep)
    out["al_update_launch_us"] = [float(np.median(r)), float(max(r) - min(r))]
    print(f"al update   one launch    median {np.median(r):9.1f} us  spread {max(r) - min(r):7.1f}")


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="phuber,arm,table,host", help="comma-separated: phuber, arm, table, host, al")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    from isls import costs
    g, mdl, x, u = problem(a.batch)
    out = {"batch": a.batch}
    if "table" in legs:
        table_section(a, out, g, mdl, x, u)
    if "al" in legs:
        al_section(a, out, g, mdl, x, u)
    if "arm" in legs:
        arm_section(a, out)
    if "phuber" in legs:
        phuber_section(a, out, g, mdl, x, u, "host" in legs)
    print(json.dumps(out))


def phuber_section(a, out, g, mdl, x, u, host):
    from isls import costs
    t0 = time.time()
    src = uc.phuber_source(4, 2, g["par_px"], g["par_pf"]) + f"// {time.time()}\n"      # a fresh source: nothing cached
    cu = costs.Custom(4, 2, uc.phuber_params(g["par_cu"], g["par_cx"], g["par_cf"]), src)
    t_create = time.time() - t0
    t0 = time.time()
    cu.code(mdl, np.float64)
    t_pair = time.time() - t0
    ph = costs.PseudoHuber(g["par_cu"], g["par_cx"], g["par_px"], g["par_cf"], g["par_pf"])
    sb, sc, sa = make(g, mdl, ph, x, u, False), make(g, mdl, cu, x, u, False), make(g, mdl, cu, x, u, True)
    eb, ec, ea = sb.engine, sc.engine, sa.engine

    def step(e):
        e.run_outer(); e.accept_x_step(tol_cost=-1.0, tol_osc=-1.0); e.linearize(); e.expand()

    def step_adv(e):
        e.run_outer(); e.advance()

    for e in (eb, ec):                                         # gains and ADMM targets for the single launches
        e.gain(active=e.admm_active); e.feedforward(active=e.admm_active)
    forms = {"rollout": (lambda: eb.rollout(20, active=eb.admm_active), lambda: ec.rollout(20, active=ec.admm_active)),
             "expand": (eb.expand, ec.expand),
             "outer": (lambda: step(eb), lambda: step(ec), lambda: step_adv(ea))}
    for name in ("rollout", "expand", "outer"):
        fns = forms[name]
        for f in fns:
            timed(f, 3)                                        # warm-up
        runs = [[] for _ in fns]
        for _ in range(a.rounds):
            for i, f in enumerate(fns):
                runs[i].append(timed(f, a.reps))
        for i, label in enumerate(("builtin", "custom", "custom_advance")[:len(fns)]):
            out[f"{name}_{label}_us"] = [float(np.median(runs[i])), float(max(runs[i]) - min(runs[i]))]
            print(f"{name:8s} {label:15s} median {np.median(runs[i]):9.1f} us  spread {max(runs[i]) - min(runs[i]):7.1f}")
    out.update(compile_create_s=t_create, compile_pair_s=t_pair)
    print(f"compile: registration + expansion {t_create:.2f} s, program with the Tassa rollout kernels {t_pair:.2f} s")
    if not host:
        return
    # host slow path for contrast: the same cost as numpy callables, one solve iteration at B = 4
    from isls import iSLS
    hs = iSLS(4, 2, int(g["N"]), batch=4)
    hs.forward_model = mdl
    hs.cost_function = lambda xx, uu: ph(xx, uu)              # a plain callable: the host route
    hs.nominal_values = x[:4], u[:4]
    torch.cuda.synchronize()
    t0 = time.time()
    hs.solve(get_Cs=ph.get_Cs, max_iter=1, max_line_search_iter=20)
    torch.cuda.synchronize()
    out.update(host_solve_iter_s_B4=time.time() - t0)
    print(f"host slow path, one solve iteration at B = 4: {out['host_solve_iter_s_B4']:.3f} s")


if __name__ == "__main__":
    main()
