#!/usr/bin/env python3
"""The Monte-Carlo closed loop (isls_mc_closed_loop_*) against the route it replaces, at config 5's shape.

    python tools/mc_bench.py [--rounds 5] [--skip-large]

* DI-3D (n = 6, m = 3), N = 50, P = 16 dense causal controllers x M = 4096 initial states, noise-free, trajectories written,
  fp64 and fp32: ONE isls_mc_closed_loop launch against 16 calls of isls_sls_closed_loop (one controller per call), device
  tensors on both sides, outputs compared.  One call each per round, HIP events, the two forms alternating over the rounds;
  medians and spread (max - min).
* recorded without a bar: statistics only with drawn initial states and noise at P = 1024, M = 4096 (stage-local gains), and the
  arm (n = 9, m = 3) at P = 1024, M = 1024, N = 100 (stage-local gains, statistics only).
Prints the numbers and one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ilqr-admm_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from isls import _capi as capi  # noqa: E402
from isls.utils import get_double_integrator_AB  # noqa: E402

DEV = "cuda:0"


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median_ms=float(np.median(ts)), spread_ms=float(max(ts) - min(ts)))


def mc_args(kern, dt, P, M, N, n, m, model, par, K, k, form, x0s=None, x0=None, x0_std=None, noise_std=None, traj=True, bounds=None):
    z = lambda *s, d=dt: torch.zeros(*s, dtype=d, device=DEV)                         # noqa: E731
    keep = dict(par=par, K=K, k=k, x0s=x0s, x0=x0, x0_std=x0_std, noise_std=noise_std)
    a = capi.McLoopArgs(P=P, M=M, N=N, n=n, m=m, model=model, K_form=form)
    a.model_par, a.K, a.k = par.data_ptr(), K.data_ptr(), k.data_ptr()
    a.K_sb, a.k_sb = K[0].numel(), k[0].numel()
    a.x0s, a.x0, a.x0_sb = capi._ptr(x0s), capi._ptr(x0), (n if x0 is not None else 0)
    a.x0_std, a.noise_std, a.seed = capi._ptr(x0_std), capi._ptr(noise_std), 1
    keep["viol"] = [z(P, N, m, d=torch.int32), z(P, N, n, d=torch.int32), z(P, d=torch.int32)]
    a.viol_u, a.viol_x, a.viol_any = (t.data_ptr() for t in keep["viol"])
    keep["ext"] = [torch.full((P, N, d_), v, dtype=dt, device=DEV) for d_, v in ((m, np.inf), (m, -np.inf), (n, np.inf), (n, -np.inf))]
    a.u_min, a.u_max, a.x_min, a.x_max = (t.data_ptr() for t in keep["ext"])
    if bounds is not None:
        keep["b"] = [torch.full((m,), -bounds, dtype=dt, device=DEV), torch.full((m,), bounds, dtype=dt, device=DEV)]
        a.u_lo, a.u_hi = capi.View(keep["b"][0].data_ptr(), 0, 0), capi.View(keep["b"][1].data_ptr(), 0, 0)
    if traj:
        keep["x"], keep["u"] = z(P, M, N, n), z(P, M, N, m)
        a.x_log, a.u_log = keep["x"].data_ptr(), keep["u"].data_ptr()
    if form == 1:
        keep["work"] = torch.empty(capi.mc_work_elems(P, M, N, n, m, 1), dtype=dt, device=DEV)
        a.work, a.work_elems = keep["work"].data_ptr(), keep["work"].numel()
    return a, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    kern = capi.Kernels(capi.library())
    stream = lambda: torch.cuda.current_stream().cuda_stream                          # noqa: E731
    rng = np.random.default_rng(0)
    out = {}
    P, M, N, n, m = 16, 4096, 50, 6, 3
    A, B = get_double_integrator_AB(3, 2, 1.0 / N)
    K_h = 0.05 * np.tril(rng.standard_normal((P, N * m, N * n)))
    for i in range(N):
        K_h[:, i * m:(i + 1) * m, (i + 1) * n:] = 0.0
    k_h, x0_h = 0.1 * rng.standard_normal((P, N * m)), rng.standard_normal((P, M, n))
    for dt, name in ((torch.float64, "f64"), (torch.float32, "f32")):
        t = lambda a_: torch.as_tensor(np.ascontiguousarray(a_), dtype=dt, device=DEV)   # noqa: E731
        A_d, B_d, K, k, x0s = t(A), t(B), t(K_h), t(k_h), t(x0_h)
        par = torch.cat([A_d.reshape(-1), B_d.reshape(-1)])
        a, keep = mc_args(kern, dt, P, M, N, n, m, capi.MODEL_LTI, par, K, k, 1, x0s=x0s)
        xl, ul = torch.zeros(P, M, N, n, dtype=dt, device=DEV), torch.zeros(P, M, N, m, dtype=dt, device=DEV)

        def new():
            kern.mc_closed_loop(a, name, stream=stream())

        def old():
            for p in range(P):
                kern.sls_closed_loop(A_d, B_d, K[p], k[p], x0s[p], xl[p], ul[p], stream=stream())
        new(), old()                                           # warm-up; the comparison
        torch.cuda.synchronize()
        err = max(float((keep["x"] - xl).abs().max()), float((keep["u"] - ul).abs().max())) / max(1.0, float(xl.abs().max()))
        tn, to = [], []
        for r in range(args.rounds):
            for which in ((new, old) if r % 2 == 0 else (old, new)):
                (tn if which is new else to).append(event_ms(which))
        sn, so = stats(tn), stats(to)
        bar = so["median_ms"] + max(sn["spread_ms"], so["spread_ms"])
        out[name] = dict(new=sn, parent=so, rel_diff=err, within_bar=bool(sn["median_ms"] <= bar))
        print(f"DI-3D N=50 P=16 M=4096 {name}: one launch {sn['median_ms']:.3f} ms (spread {sn['spread_ms']:.3f}), 16 calls of "
              f"sls_closed_loop {so['median_ms']:.3f} ms (spread {so['spread_ms']:.3f}); outputs differ by {err:.1e} rel; "
              f"{'within' if out[name]['within_bar'] else 'MISSES'} the bar")
        del a, keep, xl, ul
    if not args.skip_large:
        dt = torch.float64
        t = lambda a_: torch.as_tensor(np.ascontiguousarray(a_), dtype=dt, device=DEV)   # noqa: E731
        # statistics only, drawn initial states and noise, stage-local gains
        P, M = 1024, 4096
        par = torch.cat([t(A).reshape(-1), t(B).reshape(-1)])
        K, k = t(0.1 * rng.standard_normal((P, N, m, n))), t(0.1 * rng.standard_normal((P, N, m)))
        a, keep = mc_args(kern, dt, P, M, N, n, m, capi.MODEL_LTI, par, K, k, 0, x0=t(rng.standard_normal((P, n))),
                          x0_std=t(np.full(n, 0.3)), noise_std=t(np.full(n, 0.01)), traj=False, bounds=1.0)
        kern.mc_closed_loop(a, "f64", stream=stream())
        ts = [event_ms(lambda: kern.mc_closed_loop(a, "f64", stream=stream())) for _ in range(args.rounds)]
        out["stats_only_P1024_M4096"] = stats(ts)
        print(f"DI-3D statistics only, drawn x0 and noise, P=1024 M=4096 N=50 f64: {stats(ts)}")
        del a, keep
        # the arm
        P, M, N2, n2, m2 = 1024, 1024, 100, 9, 3
        K, k = t(0.05 * rng.standard_normal((P, N2, m2, n2))), t(0.1 * rng.standard_normal((P, N2, m2)))
        q0 = np.array([np.pi / 3, -np.pi / 2, -np.pi / 4])
        x0 = np.concatenate([q0, np.zeros(3), [np.cos(np.cumsum(q0)).sum(), np.sin(np.cumsum(q0)).sum(), 0.0]])
        a, keep = mc_args(kern, dt, P, M, N2, n2, m2, capi.MODEL_ARM3R, t([0.01]), K, k, 0, x0=t(np.tile(x0, (P, 1))),
                          x0_std=t(np.full(n2, 0.05)), noise_std=t(np.full(n2, 0.01)), traj=False, bounds=6.0)
        kern.mc_closed_loop(a, "f64", stream=stream())
        ts = [event_ms(lambda: kern.mc_closed_loop(a, "f64", stream=stream())) for _ in range(args.rounds)]
        out["arm_P1024_M1024_N100"] = stats(ts)
        print(f"arm statistics only, drawn x0 and noise, P=1024 M=1024 N=100 f64: {stats(ts)}")
    print(json.dumps(dict(tool="mc_bench", device=torch.cuda.get_device_name(0), **out)))


if __name__ == "__main__":
    main()
