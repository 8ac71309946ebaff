#!/usr/bin/env python3
"""The closed-loop covariance kernel (isls_cov_closed_loop_*) against what a user could do before it: the same recursion as a
loop of batched matrix products in torch on the device.

    python tools/cov_bench.py [--rounds 7] [--P 4096] [--N 100]

DI-3D dimensions (n = 6, m = 3) with a time-varying linearisation A, B [P,N,..], per-problem gains K, k, a shared process-noise
covariance, fp64 and fp32.  Both sides produce the means, the variances and the full covariances of x and u from device tensors:
  * ONE isls_cov_closed_loop launch;
  * the torch loop: per step torch.baddbmm / bmm on [P,n,n] (about 10 launches per step), the diagonals gathered at the end.
One call each per round, HIP events, the two forms alternating over the rounds; medians and spread (max - min); outputs compared.
Bar: the kernel is not slower than the torch loop by more than the larger of the two spreads.  The bytes are the algorithmic
w N [n n + n m + m n + m + outputs] per problem (A, B, K, k read once; x_mean, u_mean, x_var, u_var, x_cov, u_cov written once).
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


def torch_loop(A, B, K, k, xhat, uhat, S0, W, out):
    """the recursion of include/isls_hip.h (isls_cov_args) as batched matrix products"""
    P, N = K.shape[:2]
    Sig = 0.5 * (S0 + S0.transpose(-1, -2)).expand(P, -1, -1)
    d = torch.zeros(P, A.shape[-1], 1, dtype=A.dtype, device=A.device)
    for t in range(N):
        Kt, Bt = K[:, t], B[:, t]
        Phi = torch.baddbmm(A[:, t], Bt, Kt)
        out["x_cov"][:, t] = Sig
        out["x_mean"][:, t] = xhat[:, t] + d[..., 0]
        KS = torch.bmm(Kt, Sig)
        Su = torch.bmm(KS, Kt.transpose(-1, -2))
        out["u_cov"][:, t] = 0.5 * (Su + Su.transpose(-1, -2))
        kt = k[:, t, :, None]
        out["u_mean"][:, t] = uhat[:, t] + torch.baddbmm(kt, Kt, d)[..., 0]
        d = torch.baddbmm(torch.bmm(Bt, kt), Phi, d)
        S = torch.baddbmm(W.expand(P, -1, -1), torch.bmm(Phi, Sig), Phi.transpose(-1, -2))
        Sig = 0.5 * (S + S.transpose(-1, -2))
    out["x_var"].copy_(torch.diagonal(out["x_cov"], dim1=-2, dim2=-1))
    out["u_var"].copy_(torch.diagonal(out["u_cov"], dim1=-2, dim2=-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--P", type=int, default=4096)
    ap.add_argument("--N", type=int, default=100)
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least 5 rounds")
    kern = capi.Kernels(capi.library())
    stream = lambda: torch.cuda.current_stream().cuda_stream                          # noqa: E731
    rng = np.random.default_rng(0)
    P, N, n, m = args.P, args.N, 6, 3
    G = rng.standard_normal((P, N, n, n))
    A_h = G * (rng.uniform(0.7, 1.0, (P, N)) / np.linalg.norm(G, 2, axis=(-2, -1)))[..., None, None]
    B_h, K_h = rng.uniform(-0.3, 0.3, (P, N, n, m)), rng.uniform(-0.3, 0.3, (P, N, m, n))
    k_h, xh_h, uh_h = rng.uniform(-0.5, 0.5, (P, N, m)), rng.standard_normal((P, N, n)), rng.standard_normal((P, N, m))
    L0, Lw = rng.uniform(-1, 1, (P, n, n)), 0.2 * rng.uniform(-1, 1, (n, n))
    S0_h, W_h = L0 @ np.swapaxes(L0, -1, -2), Lw @ Lw.T
    out = {}
    for dt, name, w in ((torch.float64, "f64", 8), (torch.float32, "f32", 4)):
        t = lambda a_: torch.as_tensor(np.ascontiguousarray(a_), dtype=dt, device=DEV)   # noqa: E731
        A, B, K, k, xh, uh, S0, W = (t(x) for x in (A_h, B_h, K_h, k_h, xh_h, uh_h, S0_h, W_h))
        shapes = dict(x_mean=(P, N, n), u_mean=(P, N, m), x_var=(P, N, n), u_var=(P, N, m), x_cov=(P, N, n, n), u_cov=(P, N, m, m))
        new_o = {kk: torch.zeros(s, dtype=dt, device=DEV) for kk, s in shapes.items()}
        old_o = {kk: torch.zeros(s, dtype=dt, device=DEV) for kk, s in shapes.items()}
        a = capi.CovArgs(P=P, N=N, n=n, m=m)
        a.A, a.Bm = capi.make_view(A, P, N, (n, n), "A"), capi.make_view(B, P, N, (n, m), "B")
        a.K, a.K_sb, a.k, a.k_sb = K.data_ptr(), N * m * n, k.data_ptr(), N * m
        a.xhat, a.xhat_sb, a.uhat, a.uhat_sb = xh.data_ptr(), N * n, uh.data_ptr(), N * m
        a.S0, a.S0_sb, a.W = S0.data_ptr(), n * n, capi.View(W.data_ptr(), 0, 0)
        for kk, v in new_o.items():
            setattr(a, kk, v.data_ptr())

        def new():
            kern.cov_closed_loop(a, name, stream=stream())

        def old():
            torch_loop(A, B, K, k, xh, uh, S0, W, old_o)
        new(), old()                                           # warm-up; the comparison
        torch.cuda.synchronize()
        err = max(float((new_o[kk] - old_o[kk]).abs().max()) / max(1.0, float(old_o[kk].abs().max())) for kk in shapes)
        tn, to = [], []
        for r in range(args.rounds):
            for which in ((new, old) if r % 2 == 0 else (old, new)):
                (tn if which is new else to).append(event_ms(which))
        sn, so = stats(tn), stats(to)
        bar = so["median_ms"] + max(sn["spread_ms"], so["spread_ms"])
        nbytes = w * P * N * (n * n + n * m + m * n + m + 2 * (n + m) + n * n + m * m)
        out[name] = dict(kernel=sn, torch_loop=so, rel_diff=err, within_bar=bool(sn["median_ms"] <= bar),
                         algorithmic_bytes=nbytes, achieved_GBps=nbytes / (sn["median_ms"] * 1e-3) / 1e9)
        print(f"(6,3) P={P} N={N} {name}: one launch {sn['median_ms']:.3f} ms (spread {sn['spread_ms']:.3f}), torch loop "
              f"{so['median_ms']:.3f} ms (spread {so['spread_ms']:.3f}); {nbytes / 1e6:.1f} MB algorithmic = "
              f"{out[name]['achieved_GBps']:.0f} GB/s; outputs differ by {err:.1e} rel; "
              f"{'within' if out[name]['within_bar'] else 'MISSES'} the bar")
        del a, new_o, old_o
    print(json.dumps(dict(tool="cov_bench", device=torch.cuda.get_device_name(0), P=P, N=N, **out)))


if __name__ == "__main__":
    main()
