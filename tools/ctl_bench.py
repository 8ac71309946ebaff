#!/usr/bin/env python3
"""Timing of the device SLS controller synthesis (SLS.controller / iSLS.controller -> isls_sls_controller):
    python tools/ctl_bench.py [--reps 5] [--host-problems 3] [--out profiles/ctl_bench.txt]

Cases: config 5's DI-1D (N=50, n=2, m=1) and DI-3D (N=50, n=6, m=3) at B=8192, the 3R arm (N=100, n=9, m=3) at B=1024 with
a linearisation per problem, both with isls_admm's PHI_U = [phi_u, 0] and with a dense causal PHI_U.  For each case: the
device time from torch inputs (no PCIe time; HIP events around the class call, which includes the flag read-back), the
numpy-in / numpy-out wall time, the dense host path (sls_dense.controller) on a few problems scaled to the batch, and the
bytes the kernels move (PHI_U read + K written + workspace written and read) against the HBM rate they imply."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ilqr-admm_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def lower_mask(N, n, m):
    import numpy as np
    return (np.arange(N * n) // n)[None, :] <= (np.arange(N * m) // m)[:, None]


def make_case(name, B, N, n, m, ltv, first_column_only, seed=0):
    import numpy as np
    import torch

    import isls
    import isls_problems as P
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(seed)
    if ltv:
        s = isls.iSLS(n, m, N, batch=B)
        A_, B_ = P.double_integrator_AB(3, 2, 0.01)
        rng = np.random.default_rng(seed)
        A = np.broadcast_to(np.pad(A_, ((0, 3), (0, 3))), (B, N, n, n)).copy()
        A[..., 6:, :] = 0.01 * rng.standard_normal((B, N, 3, n))        # the arm's Jacobian rows, per problem and step
        A[..., 6:, 6:] += np.eye(3)
        Bm = np.concatenate([np.broadcast_to(B_, (B, N, 6, m)), 5e-5 * rng.standard_normal((B, N, 3, m))], axis=2)
        s.engine.A.copy_(torch.as_tensor(A))
        s.engine.Bm.copy_(torch.as_tensor(Bm))
        dense_args = lambda b: (A[b], Bm[b])                                  # noqa: E731
    else:
        s = isls.SLS(n, m, N)
        A, Bm = P.double_integrator_AB(n // 2, 2, 0.02)
        s.AB = [A, Bm]
        dense_args = lambda b: (np.broadcast_to(A, (N, n, n)), np.broadcast_to(Bm, (N, n, m)))     # noqa: E731
    if first_column_only:
        PHI_U = torch.zeros(B, N * m, N * n, dtype=torch.float64, device=dev)
        PHI_U[:, :, :n // 3 if ltv else n // 2] = 0.1 * torch.randn(B, N * m, n // 3 if ltv else n // 2, generator=gen,
                                                                      dtype=torch.float64, device=dev)
    else:
        PHI_U = 0.1 * torch.randn(B, N * m, N * n, generator=gen, dtype=torch.float64, device=dev) \
            * torch.as_tensor(lower_mask(N, n, m), device=dev)
    du = torch.randn(B, N * m, generator=gen, dtype=torch.float64, device=dev)
    return dict(name=name, B=B, N=N, n=n, m=m, s=s, PHI_U=PHI_U, du=du, dense_args=dense_args)


def run_case(c, reps, host_problems):
    import numpy as np
    import torch

    from isls import _capi as capi
    from isls import sls_dense as dense
    s, PHI_U, du = c["s"], c["PHI_U"], c["du"]
    B, N, n, m = c["B"], c["N"], c["n"], c["m"]
    s.controller(PHI_U, du)                                                  # warm-up: code objects, workspace allocation
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        K, k = s.controller(PHI_U, du)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    assert not s.controller_flags.any()
    P_np, d_np = PHI_U.cpu().numpy(), du.cpu().numpy()
    t0 = time.perf_counter()
    Kn, kn = s.controller(P_np, d_np)
    wall_np = time.perf_counter() - t0
    host, worst = [], 0.0
    for b in np.linspace(0, B - 1, host_problems).astype(int):
        A_, B_ = c["dense_args"](b)
        t0 = time.perf_counter()
        Kd, kd = dense.controller(*dense.transfer_matrices_ltv(A_, B_), P_np[b], d_np[b])
        host.append(time.perf_counter() - t0)
        worst = max(worst, float(np.max(np.abs(Kn[b] - Kd)) / np.max(np.abs(Kd))))
    ws = capi.sls_controller_work_elems(B, N, n) * 8
    moved = 2 * B * (N * m) * (N * n) * 8 + 2 * ws + 2 * B * N * m * 8      # PHI_U in, K out, workspace out + in, du / k
    med = float(np.median(times))
    return (f"{c['name']:34s} B={B:5d} N={N:3d} n={n} m={m}: device {med:9.2f} ms (min {min(times):.2f}, {reps} reps, torch in); "
            f"numpy in/out wall {wall_np * 1e3:9.1f} ms; host dense path {np.mean(host) * 1e3:8.2f} ms/problem -> "
            f"{np.mean(host) * B:8.1f} s per batch (scaled from {host_problems}); bytes {moved / 1e9:6.2f} GB -> "
            f"{moved / 1e9 / (med / 1e3):7.0f} GB/s; max rel diff to host {worst:.1e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-problems", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "ctl_bench.py times the device path: it needs a GPU"
    cases = [("config5 DI-1D dense causal PHI_U", 8192, 50, 2, 1, False, False),
             ("config5 DI-3D dense causal PHI_U", 8192, 50, 6, 3, False, False),
             ("arm [phi_u, 0] (isls_admm)", 1024, 100, 9, 3, True, True),
             ("arm dense causal PHI_U", 1024, 100, 9, 3, True, False)]
    lines = [f"device: {torch.cuda.get_device_name(0)}; host threads: {torch.get_num_threads()}"]
    print(lines[0], flush=True)
    for spec in cases:
        c = make_case(*spec)
        lines.append(run_case(c, a.reps, a.host_problems))
        print(lines[-1], flush=True)
        del c
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
