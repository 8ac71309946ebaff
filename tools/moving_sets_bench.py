#!/usr/bin/env python3
"""Cost of the per-row read of the row projection (project_rows_moving_kernel against project_rows_kernel, csrc/project.hip) on
config 4's own row shape: B = 4096 problems x R = 200 rows of the car's state (dimension 4), the two keep-out rectangles of
bench.py --config 4 (project_set_convex, rho = 10, at most 15 iterations, threshold 1e-3), fp64 and fp32.  The per-row table
repeats the shared block in every row, so both kernels do the same arithmetic on the same numbers; what differs is where the
operands come from (scalar loads of one block per workgroup against per-lane vector loads of a block per row).

    python tools/moving_sets_bench.py [--reps 40] [--batch 4096] [--rows 200]

Prints the median, minimum and maximum of `reps` launches per form (HIP events around each launch, five warm-up launches) and
checks that the two outputs are equal bit for bit."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ilqr-admm_amd"))
from isls import _capi as capi                                 # noqa: E402

pj = importlib.import_module("isls.projections")


def timed(kern, a, sfx, reps):
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        kern._call("project_rows", sfx, a, stream)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        kern._call("project_rows", sfx, a, stream)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1) * 1e3)
    return np.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=200)
    a = ap.parse_args()
    B, R = a.batch, a.rows
    centres, sizes, angle = np.array([[-7.0, -3.0], [-3.0, -7.0]]), np.array([[2.0, 1.0], [2.0, 1.0]]), -np.pi / 4   # bench.py --config 4
    shared = pj.keepout_rectangles(4, centres, sizes, angle)
    moving = pj.keepout_rectangles(4, np.broadcast_to(centres, (R,) + centres.shape), sizes, angle)
    rng = np.random.default_rng(0)
    y = rng.standard_normal((B, R, 4)) * np.array([3.0, 3.0, 1.0, 1.0]) + np.array([-5.0, -5.0, 0.0, 0.0])   # about the obstacles
    kern = capi.Kernels(capi.library())
    for dtype, sfx in ((torch.float64, "f64"), (torch.float32, "f32")):
        def wrap(v, dtype=dtype):
            t = torch.as_tensor(np.ascontiguousarray(v), device="cuda")
            return t.to(dtype) if v.dtype.kind == "f" else t
        yd = torch.as_tensor(y, device="cuda").to(dtype)
        outs = []
        for name, cs in (("shared", shared), ("per-row", moving)):
            od, it = yd.clone(), torch.zeros(B, dtype=torch.int32, device="cuda")
            desc = capi.Kernels.project_args_chain(yd, od, cs.stages(), wrap=wrap, iters=it)
            med, lo, hi = timed(kern, desc, sfx, a.reps)
            outs.append(od.cpu().numpy())
            print(f"{sfx} {name:8s} B={B} R={R}: median {med:8.1f} us  min {lo:8.1f}  max {hi:8.1f}  inner iterations "
                  f"{int(it.min())}..{int(it.max())}")
        print(f"{sfx} outputs equal bit for bit: {np.array_equal(outs[0], outs[1])}")


if __name__ == "__main__":
    main()
