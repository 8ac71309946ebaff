"""Time the line-search roll-out of a cost that reads a 2-D field (costs.Custom(field=), isls::field) against the same cost in
closed form.  The cost is the README's keep-out constraint, `g[0] = par[0] - isls::field(0, x[0], x[1])`, carried over to the car
(CarSimple, (4, 2)): a control cost, a terminal pull to a goal and a clearance from a disc, read once from the disc's
squared-distance map on a 257 x 257 grid and written out once -- at B = 4096, N = 100, L = 20, penalty on.
What is timed: HIP events around the roll-out entry (engine.rollout -> isls_rollout_ls_*), i.e. from the launch to the kernel's
completion, the Python call and its argument marshalling included; at this size the kernel is nearly all of it.  A warm-up, then
the median of `--launches`.  Registers and scratch of both programs' roll-out variants come from their code objects, and
`launched` names the one the launch plan picks (plan_rollout, csrc/rollout_kernel.hpp: two waves per SIMD, OCC = 2, where
max(L, 8) >= 16 and n < 9, else one; JM = 1 for this engine's arrays).

    python tools/field_bench.py [--batch 4096] [--steps 100] [--candidates 20] [--launches 30] [--dtype f64|f32]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ilqr-admm_amd"), os.path.join(ROOT, "tools")]

STAGE = r'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {
    S c = par[1] * (u[0] * u[0] + u[1] * u[1]);
    if (t == N - 1) c += par[2] * ((x[0] - par[3]) * (x[0] - par[3]) + (x[1] - par[4]) * (x[1] - par[4]));
    return c;
}
template <typename S, typename P>
__device__ void constraint(const S *x, const S *u, const P *par, int t, int N, S *g) { g[0] = par[0] - CLEARANCE; }
'''
PAR = [0.16, 0.05, 5.0, 2.0, 0.5]


def main():
    import torch
    import scan_kernels
    from isls import _capi as capi
    from isls import costs, iSLS, models
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    a = ap.parse_args()
    dtype = np.float64 if a.dtype == "f64" else np.float32
    B, N, L = a.batch, a.steps, a.candidates
    G, origin, spacing = 257, (-8.0, -8.0), (0.0625, 0.0625)
    X, Y = np.meshgrid(origin[0] + spacing[0] * np.arange(G), origin[1] + spacing[1] * np.arange(G), indexing="ij")
    sides = {"field": costs.Custom(4, 2, PAR, STAGE.replace("CLEARANCE", "isls::field(0, x[0], x[1])"), constraints=1,
                                   field=(X - 1.0) ** 2 + (Y - 0.1) ** 2, field_origin=origin, field_spacing=spacing),
             "closed form": costs.Custom(4, 2, PAR, STAGE.replace("CLEARANCE", "((x[0] - 1.0) * (x[0] - 1.0) + (x[1] - 0.1) * (x[1] - 0.1))"),
                                         constraints=1)}
    mdl = models.CarSimple(0.05)
    rng = np.random.default_rng(0)
    us = 0.3 * rng.normal(size=(B, N, 2))
    xs = np.zeros((B, N, 4))
    xs[:, 0] = rng.normal(size=(B, 4)) * [0.5, 0.5, 0.3, 0.3] + [0, 0, 0, 1.0]
    for t in range(N - 1):
        xs[:, t + 1] = mdl(xs[:, t], us[:, t])
    out = {"batch": B, "steps": N, "candidates": L, "dtype": a.dtype, "launches": a.launches}
    for name, cost in sides.items():
        s = iSLS(4, 2, N, batch=B, dtype=dtype)
        s.forward_model, s.cost_function = mdl, cost
        cost.reset_multipliers(10.0)                          # the penalty on: the constraint is evaluated and costed
        s.nominal_values = xs, us
        e = s.engine
        e.K.copy_(e._t(0.05 * np.random.default_rng(1).normal(size=(B, N, 2, 4))))
        e.k.copy_(e._t(0.05 * np.random.default_rng(2).normal(size=(B, N, 2))))
        flags = capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST
        for _ in range(5):
            e.rollout(L, flags=flags, active=e.outer_active)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.launches):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            e.rollout(L, flags=flags, active=e.outer_active)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        md = {k[".name"]: k for k in scan_kernels._metadata(cost.code(mdl, dtype))["amdhsa.kernels"]}
        regs = {k.split("rollout_kernel")[1][:24]: dict(vgpr=v.get(".vgpr_count"), agpr=v.get(".agpr_count"), sgpr=v.get(".sgpr_count"),
                                                        scratch=v.get(".private_segment_fixed_size"))
                for k, v in md.items() if "rollout_kernel" in k}
        for v in regs.values():                               # waves per SIMD the registers allow (512 unified registers per lane)
            v["waves_per_simd"] = min(8, 512 // max(1, -(-int(v["vgpr"]) // 8) * 8))
        occ = 2 if max(L, 8) >= 16 else 1
        launched = [k for k in regs if k.endswith(f"Li1ELi{occ}EEE")]
        out[name] = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "variants": regs,
                     "launched": launched}
    out["ratio"] = out["field"]["median_ms"] / out["closed form"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
