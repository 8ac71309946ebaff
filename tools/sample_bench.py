#!/usr/bin/env python
"""The sampling warm start (iSLS.sample_nominal) at B = 4096, N = 100, S = 1024, fp64, on (a) the headline double integrator
(n = 6, m = 3) with its via-point cost and (b) the README's quadrotor (models.Custom) with its bump cost (costs.Custom): the
median over `--blocks` blocks of each of one round's two launches (isls_sample_nominal_* with phase = 1 / 2, HIP events around
each) and of one sample_nominal call (wall clock: the launches, the nominal's cost and the read-back of the statistics); the numpy restatement of
the tests at B = 8, stated per problem (extrapolating it to B = 4096 is a multiplication, not a measurement); and, for (b), the
share of problems whose straight-line guess crosses the bump and whose cost after solve(max_iter=20) is lower with one sampling
round in front than without.

    python tools/sample_bench.py [--batch 4096] [--samples 1024] [--blocks 7] [--out profiles/sample_bench.json]
    python tools/sample_bench.py --feedback [...]    the closed-loop round (sample_nominal(feedback=)): its two launches beside the
                                 open-loop ones in the same blocks, gains from a regularised backward pass, and the warm start of
                                 (b) with feedback=True at the recorded sigma and at 0.3; added to --out under keys of their own
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ilqr-admm_amd"), os.path.join(ROOT, "tests")]

import isls                                                      # noqa: E402
import isls_problems as P                                        # noqa: E402
import sampling_reference as R                                   # noqa: E402
from isls import costs, models                                   # noqa: E402

QUAD = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    const S f = u[0] + u[1], s = sin(x[2]), c = cos(x[2]);
    xn[0] = x[0] + par[0] * x[3];  xn[1] = x[1] + par[0] * x[4];  xn[2] = x[2] + par[0] * x[5];
    xn[3] = x[3] - par[0] * f * s / par[1];  xn[4] = x[4] + par[0] * (f * c / par[1] - par[4]);
    xn[5] = x[5] + par[0] * par[3] * (u[0] - u[1]) / par[2];
}'''
SOFT = r'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {
    const S dx = x[0] - par[2], dy = x[1] - par[3], ex = x[0] - par[7], ey = x[1] - par[8];
    S c = par[0] * (u[0] * u[0] + u[1] * u[1]) + par[1] * exp(-(dx * dx + dy * dy) / (par[4] * par[4]));
    S d2 = ex * ex + ey * ey;
    for (int i = 2; i < 6; ++i) d2 += x[i] * x[i];
    c += par[5] * d2;
    if (t == N - 1) c += par[6] * d2;
    return c;
}'''
QUAD_PAR = np.array([0.05, 1.0, 0.02, 0.15, 9.81])
SOFT_PAR = np.array([0.05, 5.0, 0.5, 0.2, 0.3, 0.5, 50.0, 1.0, 0.5])


def quad_step(x, u, par):
    dt, mass, inertia, arm, g = par
    f, s, c = u[..., 0] + u[..., 1], np.sin(x[..., 2]), np.cos(x[..., 2])
    return np.stack([x[..., 0] + dt * x[..., 3], x[..., 1] + dt * x[..., 4], x[..., 2] + dt * x[..., 5], x[..., 3] - dt * f * s / mass,
                     x[..., 4] + dt * (f * c / mass - g), x[..., 5] + dt * arm * (u[..., 0] - u[..., 1]) / inertia], axis=-1)


def soft_stage(x, u, t, N):
    p = SOFT_PAR
    d2 = (x[..., 0] - p[7]) ** 2 + (x[..., 1] - p[8]) ** 2 + np.sum(x[..., 2:] ** 2, axis=-1)
    c = p[0] * np.sum(u * u, axis=-1) + p[1] * np.exp(-((x[..., 0] - p[2]) ** 2 + (x[..., 1] - p[3]) ** 2) / p[4] ** 2)
    return c + (p[5] + (p[6] if t == N - 1 else 0.0)) * d2


def di_problem(B, N):
    cfg = P.config2(batch=B, N=N, seed=0)
    xs, us = (np.stack(a) for a in zip(*[P.initial_nominal(cfg, b) for b in range(B)]))

    def make():
        s = isls.iSLS(6, 3, N, batch=B)
        s.forward_model = models.LTI(cfg["A"], cfg["B"])
        s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
        s.reset()
        s.nominal_values = xs, us
        return s
    A, Bm = cfg["A"], cfg["B"]
    step = lambda x, u, par: x @ A.T + u @ Bm.T                  # noqa: E731
    zs = np.asarray(cfg["zs"])
    ref = (step, np.zeros(1), R.via_cost(zs[:8] if zs.ndim == 3 else zs, cfg["Qs"], np.asarray(cfg["seq"]), cfg["u_std"]), xs[:8], us[:8])
    return make, ref, dict(sigma=0.5, temperature=0.05)


def quad_problem(B, N):
    """hover controls from starts to the lower left of the bump at (0.5, 0.2): the straight line to the goal (1, 0.5) crosses it"""
    rng = np.random.default_rng(0)
    us = np.full((B, N, 2), 0.5 * QUAD_PAR[1] * QUAD_PAR[4])
    x0 = np.zeros((B, 6))
    x0[:, :2] = np.array([0.0, -0.1]) + 0.05 * rng.standard_normal((B, 2))
    xs = R.rollout(quad_step, x0, us, QUAD_PAR)

    def make():
        s = isls.iSLS(6, 2, N, batch=B)
        s.forward_model = models.Custom(6, 2, QUAD_PAR, QUAD)
        s.cost_function = costs.Custom(6, 2, SOFT_PAR, SOFT)
        s.reset()
        s.nominal_values = xs, us
        return s
    return make, (quad_step, QUAD_PAR, R.sum_cost(soft_stage), xs[:8], us[:8]), dict(sigma=1.0, temperature=0.05, clip_u=(0.0, 12.0))


def measure(name, make, ref, kw, S, blocks):
    q = make()
    e = q.engine
    q.sample_nominal(samples=S, seed=0, **kw)                   # warm-up: modules, buffers
    sigma = e._t(np.full(e.m, float(kw["sigma"])))
    costs_ = torch.zeros(e.B, S, dtype=e.dtype, device=e.device)
    clip = [None if "clip_u" not in kw else e._t(np.full(e.m, float(v))) for v in kw.get("clip_u", (0, 0))]
    cost_ms, update_ms, call_ms = [], [], []
    for k in range(blocks):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        e.sample_round(sigma, costs_, u_lo=clip[0], u_hi=clip[1], temperature=kw["temperature"], seed=100 + k, phase=1)
        ev[1].record()
        e.sample_round(sigma, costs_, u_lo=clip[0], u_hi=clip[1], temperature=kw["temperature"], seed=100 + k, phase=2)
        ev[2].record()
        torch.cuda.synchronize()
        cost_ms.append(ev[0].elapsed_time(ev[1]))
        update_ms.append(ev[1].elapsed_time(ev[2]))
        t0 = time.perf_counter()
        q.sample_nominal(samples=S, seed=200 + k, **kw)
        torch.cuda.synchronize()
        call_ms.append(1e3 * (time.perf_counter() - t0))
    step, par, cost, xh, uh = ref
    t0 = time.perf_counter()
    R.sample_nominal(step, par, cost, xh, uh, kw["sigma"], seed=0, samples=S, temperature=kw["temperature"], clip_u=kw.get("clip_u"))
    numpy_ms = 1e3 * (time.perf_counter() - t0) / xh.shape[0]
    return {f"{name}_sample_cost_kernel_ms": float(np.median(cost_ms)), f"{name}_sample_update_kernel_ms": float(np.median(update_ms)),
            f"{name}_sample_nominal_ms": float(np.median(call_ms)),
            f"{name}_numpy_ms_per_problem_at_B8": numpy_ms,
            f"{name}_numpy_ms_extrapolated_to_batch": numpy_ms * e.B}


def measure_feedback(name, make, kw, S, blocks):
    """Both launches of a round in closed loop about the gains of a backward pass (isls_sample_nominal_fb_*) and, in the same
    blocks, in open loop: each between its own HIP events through `phase`, medians over the blocks."""
    from isls import Regularization
    q = make()
    e = q.engine
    q.sample_nominal(samples=S, seed=0, feedback=True, regularization=Regularization(), **kw)   # warm-up; leaves gains in e.K
    K = e.K.clone()
    sigma = e._t(np.full(e.m, float(kw["sigma"])))
    costs_ = torch.zeros(e.B, S, dtype=e.dtype, device=e.device)
    clip = [None if "clip_u" not in kw else e._t(np.full(e.m, float(v))) for v in kw.get("clip_u", (0, 0))]
    ms = {(fb, ph): [] for fb in (False, True) for ph in (1, 2)}
    for k in range(blocks):
        for fb in (False, True):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            for ph in (1, 2):
                ev[ph - 1].record()
                e.sample_round(sigma, costs_, u_lo=clip[0], u_hi=clip[1], temperature=kw["temperature"], seed=100 + k, phase=ph,
                               K=K if fb else None)
            ev[2].record()
            torch.cuda.synchronize()
            ms[fb, 1].append(ev[0].elapsed_time(ev[1]))
            ms[fb, 2].append(ev[1].elapsed_time(ev[2]))
    med = lambda fb, ph: float(np.median(ms[fb, ph]))            # noqa: E731
    return {f"{name}_sample_cost_fb_kernel_ms": med(True, 1), f"{name}_sample_update_fb_kernel_ms": med(True, 2),
            f"{name}_sample_cost_kernel_ms_beside_fb": med(False, 1), f"{name}_sample_update_kernel_ms_beside_fb": med(False, 2)}


def feedback_main(a):
    """--feedback: the closed-loop kernels beside the open-loop ones, and the warm-start experiment on (b) with feedback=True at the
    recorded sigma and at a smaller one; written under new keys of the existing file (the recorded open-loop figures stay)."""
    from isls import Regularization
    B, N, S = a.batch, a.horizon, a.samples
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    make_di, _, kw_di = di_problem(B, N)
    out.update(measure_feedback("di", make_di, kw_di, S, a.blocks))
    make_q, _, kw_q = quad_problem(B, N)
    out.update(measure_feedback("quad_bump", make_q, kw_q, S, a.blocks))
    plain = make_q()
    plain.solve(max_iter=20, regularization=Regularization())
    for sigma in (kw_q["sigma"], 0.3):
        warm = make_q()
        w = warm.sample_nominal(samples=S, seed=0, feedback=True, regularization=Regularization(), **{**kw_q, "sigma": sigma})
        warm.solve(max_iter=20, regularization=Regularization())
        tag = f"quad_bump_fb_sigma_{sigma:g}"
        out.update({f"{tag}_median_cost_before": float(np.median(w.cost_before)),
                    f"{tag}_median_cost_after_sampling": float(np.median(w.cost_after)),
                    f"{tag}_share_moved": float(np.mean(w.cost_after < w.cost_before)),
                    f"{tag}_median_cost_warm": float(np.median(warm.cost)),
                    f"{tag}_share_lower_with_warm_start": float(np.mean(warm.cost < plain.cost))})
    out["quad_bump_fb_median_cost_plain"] = float(np.median(plain.cost))
    out["feedback_batch_horizon_samples_blocks"] = [B, N, S, a.blocks]
    print(json.dumps({k: v for k, v in out.items() if "fb" in k or "feedback" in k}))
    with open(a.out, "w") as f:
        json.dump(out, f)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--feedback", action="store_true", help="measure the closed-loop round (feedback=) beside the open-loop one and "
                    "add its figures to --out; the recorded open-loop figures stay")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    a = ap.parse_args()
    if a.feedback:
        return feedback_main(a)
    B, N, S = a.batch, a.horizon, a.samples
    out = dict(batch=B, horizon=N, samples=S, blocks=a.blocks, dtype="float64",
               not_measured=["rocprofv3 kernel-trace durations", "fp32", "other S, N, B"])
    make_di, ref_di, kw_di = di_problem(B, N)
    out.update(measure("di", make_di, ref_di, kw_di, S, a.blocks))
    make_q, ref_q, kw_q = quad_problem(B, N)
    out.update(measure("quad_bump", make_q, ref_q, kw_q, S, a.blocks))
    # the warm start in front of the solver on (b): reported, not asserted
    from isls import Regularization
    plain, warm = make_q(), make_q()
    w = warm.sample_nominal(samples=S, seed=0, **kw_q)
    for s in (plain, warm):
        s.solve(max_iter=20, regularization=Regularization())
    out.update(quad_bump_share_lower_with_warm_start=float(np.mean(warm.cost < plain.cost)),
               quad_bump_median_cost_plain=float(np.median(plain.cost)), quad_bump_median_cost_warm=float(np.median(warm.cost)),
               quad_bump_median_cost_after_sampling=float(np.median(w.cost_after)), quad_bump_median_cost_before=float(np.median(w.cost_before)))
    print(json.dumps(out))
    with open(a.out, "w") as f:
        json.dump(out, f)
        f.write("\n")


if __name__ == "__main__":
    main()
