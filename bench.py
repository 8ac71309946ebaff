#!/usr/bin/env python3
"""bench.py -- iLQR-ADMM outer iterations per second on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run)
    python bench.py ... --full                             (+ general-layout and shared-LTI legs, per-kernel events, roofline, CPU baseline)
    python bench.py ... --dump-outputs DIR                 (+ the last timed step's results as DIR/<name>.npy, float64)

A plain run sets up, warms up, times the K steps and prints the result line; everything else it can measure is behind --full.

Workload (config 2 of BASELINE.json): 3-D double integrator iLQR-ADMM, fp64, per GPU
B=4096 trajectories x N=100 steps, n=6, m=3, J=5 ADMM iterations per outer iteration, L=20 line-search
candidates, box constraint on u, early exit disabled (fixed work).  A_t, B_t are passed in the general
time-varying per-trajectory layout [B,N,n,n] (--lti uses the stride-0 shared layout instead).
One "step" = one outer iteration over the rank's batch:
    linearise + quadratic expansion -> Riccati gain pass -> J x [feed-forward pass -> L-candidate
    rollout + cost + arg-min + winner -> ADMM projection/dual/residual update] -> nominal update ->
    convergence reduction (+ one 40-byte RCCL all-reduce when N>1).
Inputs are resident in HBM before the timed region.  Multi-GPU = weak scaling: every rank owns its own
4096 trajectories; value = n_gpus * K / (max-over-ranks time)  [batch-4096 iterations per second].
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "ilqr-admm_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

EVENT_PERIOD = 4               # kernel-family durations are sampled on every 4th timed step
# ISLS_BENCH_REHEARSAL=1: the N>1 code path on a box with ONE device -- every rank drives cuda:0 and the collectives go over
# gloo (RCCL refuses two ranks on one device).  The line it prints says so ("rehearsal": true) and is not a measurement.
REHEARSAL = os.environ.get("ISLS_BENCH_REHEARSAL", "0") == "1"
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
KIND_NAMES = ["riccati_gain_kernel", "riccati_ff_kernel", "rollout_kernel", "admm_update_kernel", "ff_prepare_kernel"]
# kernels behind each timed family (isls_timing kind): the time-parallel feed-forward pass is two launches
KIND_KERNELS = [["riccati_gain_kernel"], ["riccati_ff_kernel", "riccati_ffrec_kernel", "riccati_ffrec2_kernel", "ff_stitch_kernel"], ["rollout_kernel"],
                ["admm_update_kernel"], ["ff_prepare_kernel", "ff_prepare_rec_kernel"]]
def _latest_pmc_file():
    """Newest committed PMC traffic table (profiles/rNN_pmc_traffic.json, written by tools/pmc_traffic.py)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    return files[-1] if files else None


PMC_FILE = _latest_pmc_file()


def pmc_tree():
    """The source tree the committed PMC table was measured on (written into it by tools/pmc_traffic.py)."""
    try:
        return json.load(open(PMC_FILE)).get("tree")
    except (OSError, ValueError, TypeError, AttributeError):
        return None


# position of the LIN template argument (0: dense form, else a model-structured one) in the kernels that have it
LIN_ARG = {"riccati_gain_kernel": 8, "riccati_ffrec2_kernel": 6}


def pmc_traffic(kind, structured=False):
    """HBM bytes per launch of a kernel family from the committed rocprofv3 PMC passes (tools/pmc_traffic.py),
    or None when no profile of this workload is available.  The profiled run holds both forms of the Riccati passes (the
    timed region and the general-layout leg): the instances of the form the timed region ran are the ones counted."""
    try:
        kernels = json.load(open(PMC_FILE))["kernels"]
    except (OSError, ValueError, KeyError, TypeError):
        return None
    total, found = 0.0, False
    for name, rec in kernels.items():
        fam = next((k for k in KIND_KERNELS[kind] if ("isls::" + k + "<") in name), None)
        if fam is None or "<double" not in name:
            continue
        if fam in LIN_ARG:
            targs = [t.strip() for t in name[name.index("<") + 1:name.rindex(">")].split(",")]
            lin = targs[LIN_ARG[fam]] if len(targs) > LIN_ARG[fam] else "0"
            if (lin != "0") != bool(structured):
                continue
        total += rec["hbm_bytes"]
        found = True
    return total if found else None


def algorithmic_bytes(n, m, N, w, has_x, has_u, lti, hess_shared, records, gain_ff=False, structured=False):
    """HBM bytes per trajectory per launch that each kernel family MUST move in the layout in use (each distinct array
    once; stride-0 shared tables cost nothing per trajectory):
      hess_shared : Cxx, Cuu are batch-shared [N,.,.] tables (Engine._shared_hessian) -> not counted;
      records     : the feed-forward passes read the packed step records [A+BK | B | K | fac] of the gain pass, so the
                    gain pass does not write Quu / fac / Qux and ff reads n^2+2nm+m^2 words per step instead of the six
                    arrays.  The records themselves are an internal layout: the gain pass is credited with A, B in and
                    K out only (writing them is its own overhead), ff with what it reads.
      gain_ff     : the first feed-forward pass of an outer iteration rides on the gain pass (isls_riccati_gain_ff_*): that
                    launch is credited with the pass's vectors as well (c0, the regularised blocks in, k out) -- not with
                    the operators, which it never reads back.
      structured  : A, B are the linearisation of a model whose structure the passes know (isls_gain_args.lin_on /
                    isls_ff_args.lin_on: the double integrator): the gain pass does not read A, B, a feed-forward pass
                    reads [K | fac] of a record (mn + m^2 words) instead of all of it."""
    ab = 0 if (lti or structured) else n * n + n * m
    hess = 0 if hess_shared else n * n + m * m
    reg = (3 * n if has_x else 0) + (3 * m if has_u else 0)            # xhat/uhat, z, lambda of the regularised blocks
    gain = ab + hess + m * n + (0 if records else m * n + 2 * m * m)   # A,B,(Cxx,Cuu) in; K (,Qux,Quu,fac) out
    if gain_ff:
        gain += (n + m) + reg + m
    ops = (n * n + 2 * n * m + m * m) if records else (ab + 2 * m * n + 2 * m * m)
    ops_ff = (m * n + m * m) if (records and structured) else ops
    ff = ops_ff + (n + m) + reg + m                                    # operators, c0, reg in; k out
    ro = m * n + m + (n + m) + ((2 * n if has_x else 0) + (2 * m if has_u else 0)) + (n + m)   # K,k,nominal,z,l in; x,u out
    admm = (5 * n if has_x else 0) + (5 * m if has_u else 0)          # x,z,l in; z,l out
    prep = ops + m * n                                                 # operators in; G out (once per gain pass)
    return [w * N * v for v in (gain, ff, ro, admm, prep)]


def iteration_bytes(n, m, N, w, hess_shared, has_x=True, has_u=True, ab_shared=False):
    """SURVEY 8(d) official figure: bytes_traj = w*N*[2n^2 + 2nm + m^2 + m + 7(n+m)] (fully fused ideal).  Of the 7(n+m), 3(n+m)
    are cx,cu in, xhat,uhat in and out; 4(n+m) are z, lambda in and out, which exist only for the constrained blocks (config 2
    constrains u alone: 4m); the n^2 + m^2 of Cxx, Cuu are dropped when they are batch-shared tables ("drop the
    Cxx,Cuu terms when they are shared")."""
    zl = 4 * ((n if has_x else 0) + (m if has_u else 0))
    ab = 0 if ab_shared else n * n + n * m                     # A, B: nothing per trajectory when they are the model's constants
    return w * N * (n * n + n * m + ab + m * m + m + 3 * (n + m) + zl - (n * n + m * m if hess_shared else 0))


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(out_dir, per_trajectory, whole):
    """`--dump-outputs DIR`: every array as DIR/<name>.npy in float64.  `per_trajectory` holds [B, ...] arrays (None entries are
    skipped); when they and `whole` would exceed DUMP_LIMIT_BYTES, a fixed, seeded sample of trajectories is written (the same
    rows of every array).  trajectory_index.npy names the rows written."""
    host = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in per_trajectory.items() if v is not None}
    whole = {k: np.asarray(v, dtype=np.float64) for k, v in whole.items()}
    B = next(iter(host.values())).shape[0]
    row_bytes = 8 + sum(a[0].nbytes for a in host.values())          # + the row's entry in trajectory_index
    headers = 1024 * (len(host) + len(whole) + 1)                     # .npy headers, generously
    rows = max(1, (DUMP_LIMIT_BYTES - headers - sum(a.nbytes for a in whole.values())) // row_bytes)
    idx = np.arange(B) if rows >= B else np.sort(np.random.default_rng(0).choice(B, int(rows), replace=False))
    os.makedirs(out_dir, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), np.ascontiguousarray(a[idx]))
    for k, a in whole.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), a)
    np.save(os.path.join(out_dir, "trajectory_index.npy"), idx.astype(np.float64))


def spawn_ranks(n_gpus):
    """`python bench.py --gpus N` without a launcher: start `torch.distributed.run` with N ranks (one per GPU, RCCL) as a
    CHILD process and return its exit code.  Called before anything initialises the GPU; device_count() does not."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < n_gpus and not REHEARSAL:
        sys.exit(f"bench.py: --gpus {n_gpus} requested but only {have} HIP device(s) are visible; refusing to print a "
                 f"{n_gpus}-GPU line from fewer devices")
    if REHEARSAL and have < 1:
        sys.exit("bench.py: the rehearsal needs one HIP device")
    with socket.socket() as so:                                # a free rendezvous port on the loopback interface
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    # dmabuf IPC: this image's host driver supports no legacy IPC handles, and RCCL / cross-process device memory fail with
    # `hipIpcGetMemHandle: invalid argument` without it (the image exports it already; kept for environments built by hand)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4096, help="trajectories per GPU")
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--J", type=int, default=5)
    ap.add_argument("--L", type=int, default=20)
    ap.add_argument("--lti", action="store_true", help="share A,B over batch and time (stride-0 views)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--only-timed-region", action="store_true",
                    help="profiling with --full: skip the general-layout and shared-LTI legs behind the timed region (counter passes then see its kernels only)")
    ap.add_argument("--separate-launches", action="store_true",
                    help="A/B: accept, ADMM restart, linearisation and expansion as four launches instead of isls_outer_advance")
    ap.add_argument("--cpu-sample", type=int, default=0, help="trajectories in the CPU-baseline sample (0: auto)")
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 4),
                    help="2: the headline workload (default); 3: 3R arm, state + control boxes; 4: car, control box + keep-out rectangles")
    ap.add_argument("--config5", action="store_true", help="secondary workload: SLS-ADMM with chance constraints (B=8192, N=50)")
    ap.add_argument("--config5-dim", type=int, default=1, help="double integrator dimension of the config-5 workload (1 or 3)")
    ap.add_argument("--isls-admm", action="store_true", help="secondary workload: iSLS.isls_admm on the 3R arm with robust control bounds")
    ap.add_argument("--full", action="store_true",
                    help="headline workload: also time the general-layout and shared-LTI legs, sample per-kernel HIP events in the "
                         "timed region (kernels_ms_per_step, roofline) and time the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="headline workload: write what the last timed step computed as DIR/<name>.npy (float64, at most 64 MB; "
                         "rank 0's trajectories when --gpus > 1)")
    args = ap.parse_args()
    if args.dump_outputs and (args.config5 or args.isls_admm or args.config in (3, 4)):
        ap.error("--dump-outputs serves the headline workload only")
    if args.config5:
        return config5_main(args)
    if args.isls_admm:
        return isls_admm_main(args)
    if args.config in (3, 4):
        return secondary_config_main(args)

    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn_ranks(args.gpus)                         # child launcher; nothing has touched the GPU yet
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if REHEARSAL:
        local_rank = 0                                        # every rank on the one device of a test box, table over gloo
    if torch.cuda.device_count() < (local_rank + 1 if world > 1 else 1):
        sys.exit(f"bench.py: rank {rank} needs device {local_rank}, only {torch.cuda.device_count()} HIP device(s) visible")
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        try:
            if REHEARSAL:
                dist.init_process_group("gloo")
            else:
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        except Exception as exc:                               # a rank that cannot join says why and fails the launch
            print(f"bench.py: rank {rank}: init_process_group failed: {type(exc).__name__}: {exc}", file=sys.stderr, flush=True)
            sys.exit(3)
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", torch.cuda.current_device())

    import isls_problems as P
    from isls import _capi as capi
    from isls.engine import Engine, library
    from isls.shard import TableExchange

    B, N, J, L = args.batch, args.horizon, args.J, args.L
    cfg = P.config2(batch=B, N=N, seed=rank)
    n, m = cfg["n"], cfg["m"]
    eng = Engine(B, N, n, m, dtype=torch.float64, device=dev)
    from isls import models
    mdl = models.LTI(cfg["A"], cfg["B"])      # recognised as a double integrator -> ISLS_MODEL_DI (same numbers as the dense LTI map)
    eng.set_model(mdl.model_id, mdl.params())
    eng.set_quadratic_cost(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    # initial nominal: u = 0 from x0 (the double integrator keeps position, zero velocity)
    x_nom = np.repeat(cfg["x0"][:, None, :], N, axis=1)
    eng.set_nominal(x_nom, cfg["u0"])
    eng.set_admm(rho_u=cfg["rho_u"], u_box=(cfg["u_lo"], cfg["u_hi"]), relax=cfg["relax"])
    if args.lti:
        eng.A = torch.as_tensor(cfg["A"], device=dev).reshape(1, 1, n, n)
        eng.Bm = torch.as_tensor(cfg["B"], device=dev).reshape(1, 1, n, m)
    # tolerances 0: no early exit, fixed work.  begin_done: every step ends with eng.advance(), which makes the ADMM restart
    eng.build_outer(L, J, tol_abs=0.0, tol_rel=0.0, begin_done=not args.separate_launches)
    # convergence table of every outer iteration: this shard's row + ONE asynchronous all-reduce (RCCL's own stream); the
    # compute stream never waits for it, the host reads the table an iteration late (isls/shard.py::TableExchange)
    xch = TableExchange(world, rank, torch.float64, dev)

    def exchange():
        xch.post(lambda table, r: eng.reduce(table=table, rank=r))

    def step():
        # one outer iteration = gain + J x (ff, rollout, update) [one C call], then ONE launch for what sits between two
        # x-step solves: nominal <- x-step and cost log (no stop rule), ADMM restart, A_t,B_t of every trajectory rewritten
        # in HBM (--lti: shared, not rewritten), c0x,c0u about the new nominal -- every step runs each stage once; the
        # linearisation / expansion the first step consumes is made below, before the warm-up
        eng.run_outer()
        if args.separate_launches:
            eng.accept_x_step()
            if not args.lti:
                eng.linearize()
            eng.expand()
        else:
            eng.advance(linearize=not args.lti)
        exchange()                                            # this shard's row of the [W,5] table (one launch) + the one collective

    if not args.lti:
        eng.linearize()
    eng.expand()                                              # also writes the batch-shared Cxx, Cuu tables once
    eng.begin_outer()
    lib = library()
    for _ in range(args.warmup):
        step()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    timing = None
    if args.full:
        timing = lib.isls_timing_create()                    # caller-owned event context, handed to the C driver
        eng._outer_args.timing = timing
        lib.isls_timing_reset(timing)
    t0 = time.perf_counter()
    for i in range(args.steps):
        # --full: per-launch HIP events on every EVENT_PERIOD-th step of the timed region: an event pair per launch costs a
        # few microseconds of queue bubbles (measured: 2.03 ms per step with events on every step, 1.89 without)
        if timing is not None:
            lib.isls_timing_pause(timing, 0 if i % EVENT_PERIOD == 0 else 1)
        step()
    xch.finish()                                             # every exchange of the timed region is inside it
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng._outer_args.timing = None
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device="cpu" if REHEARSAL else dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    red_host = xch.finish().cpu().numpy()
    hess_shared = bool(eng._shared_hessian())
    if args.dump_outputs and rank == 0:                      # before the --full legs below run more steps on the same engine
        dump_outputs(args.dump_outputs, {
            "x": eng.xhat, "u": eng.uhat, "cost": eng.cost,  # nominal trajectory after the last step's accept, and its cost
            "z_u": eng.zu, "admm_residuals": eng.res,         # ADMM state the last step left (its lambda is restarted)
            "status": eng.status}, {"convergence_table": red_host})

    # ---- the same workload in the GENERAL layout: time-varying A_t, B_t per trajectory read from HBM by the gain pass, whole
    # records by the feed-forward passes, A_t, B_t rewritten by every step -- what any model that is not a double integrator
    # (or a caller's get_AB) runs; the timed region above is the product's default path, which recognises the model
    structured = bool(eng._outer_args.ff.lin_on)               # what the timed region ran with
    general_it_per_s = None
    if structured and args.full and not args.only_timed_region:
        eng.use_model_structure = False
        step()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        tg = time.perf_counter()
        for _ in range(args.steps):
            step()
        xch.finish()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        dg = time.perf_counter() - tg
        if dist is not None:
            tg_ = torch.tensor([dg], dtype=torch.float64, device="cpu" if REHEARSAL else dev)
            dist.all_reduce(tg_, op=dist.ReduceOp.MAX)
            dg = float(tg_.item())
        general_it_per_s = world * args.steps / dg
        eng.use_model_structure = True

    # ---- the same workload with A,B shared over batch and time (stride-0 views; SURVEY 8(d): "report both") ----
    lti_it_per_s = None
    if not args.lti and args.full and not args.only_timed_region:
        eng.A = torch.as_tensor(cfg["A"], device=dev).reshape(1, 1, n, n)
        eng.Bm = torch.as_tensor(cfg["B"], device=dev).reshape(1, 1, n, m)
        eng.build_outer(L, J, tol_abs=0.0, tol_rel=0.0, begin_done=not args.separate_launches)

        def step_lti():
            eng.run_outer()
            if args.separate_launches:
                eng.accept_x_step()
                eng.expand()
            else:
                eng.advance(linearize=False)
            exchange()

        step_lti()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step_lti()
        xch.finish()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        dl = time.perf_counter() - t1
        if dist is not None:
            tl = torch.tensor([dl], dtype=torch.float64, device="cpu" if REHEARSAL else dev)
            dist.all_reduce(tl, op=dist.ReduceOp.MAX)
            dl = float(tl.item())
        lti_it_per_s = world * args.steps / dl

    # ---- --full: per-kernel-family durations from the HIP events recorded on the launch stream ------------
    fam = None
    if timing is not None:
        fam = []
        for kind in range(5):
            cnt = ctypes.c_int(0)
            ms = lib.isls_timing_read_ms(timing, kind, ctypes.byref(cnt))
            fam.append((ms, cnt.value))
        lib.isls_timing_destroy(timing)

    if rank == 0:
        it_per_s = world * args.steps / dt
        # fewer ff launches than rollouts: the first pass rode on the gain pass (counted by the events of --full)
        gain_ff = fam[1][1] < fam[2][1] if fam is not None else None
        out = {
            "metric": "iLQR-ADMM iterations/sec, batch=4096 N=100 x_dim=6",
            "value": it_per_s, "unit": "iterations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "config2: 3-D double integrator iLQR-ADMM (DP form), box constraint on u",
                       "batch_per_gpu": B, "horizon": N, "x_dim": n, "u_dim": m, "admm_iters_J": J,
                       "line_search_L": L,
                       "layout": ("LTI stride-0 A,B" if args.lti else
                                  ("double integrator recognised (isls.models.LTI -> ISLS_MODEL_DI): Riccati passes on the model's structure, "
                                   "A,B linearised once, not read per step; the general layout is general_ab_iterations_per_s" if structured
                                   else "time-varying A,B per trajectory")),
                       "general_ab_iterations_per_s": general_it_per_s,   # time-varying A_t,B_t per trajectory read from HBM, rewritten every step
                       "cost_hessians": ("batch-shared [N,n,n] / [N,m,m] tables written once (via-point cost with a shared Q and rho; "
                                         "SURVEY 8d: Cxx,Cuu terms dropped)" if hess_shared else "per trajectory [B,N,n,n]"),
                       "early_exit": False, "lti_stride0_layout_iterations_per_s": lti_it_per_s,
                       "ff_time_parallel_segments": max(1, int(eng._outer_args.ff.seg.nseg)),
                       "first_ff_pass_inside_gain_pass": gain_ff, "trajectory_iterations_per_s": it_per_s * B,
                       "admm_iterations_per_s": it_per_s * J},
            "convergence": {"sum_cost": float(red_host[:, 0].sum()), "max_prim": float(red_host[:, 1].max()),
                            "max_dual": float(red_host[:, 2].max()), "active": float(red_host[:, 3].sum()),
                            "failed": float(red_host[:, 4].sum())},
        }
        if fam is not None:
            w = 8
            records = eng.ff_record() is not None
            has_x, has_u = eng.zx is not None, eng.zu is not None
            abytes = algorithmic_bytes(n, m, N, w, has_x=has_x, has_u=has_u, lti=args.lti, hess_shared=hess_shared, records=records,
                                       gain_ff=gain_ff, structured=structured)
            nseg_ff = max(1, int(eng._outer_args.ff.seg.nseg))
            abytes[4] = abytes[4] * (nseg_ff - 1) / nseg_ff          # the operators cover every segment but the last
            sampled = len(range(0, args.steps, EVENT_PERIOD))
            dom = int(np.argmax([ms for ms, _ in fam]))
            default_workload = (B, N, J, L) == (4096, 100, 5, 20) and not args.lti
            avg_ms = fam[dom][0] / max(1, fam[dom][1])
            achieved = abytes[dom] * B / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            it_bytes = iteration_bytes(n, m, N, w, hess_shared, has_x=has_x, has_u=has_u, ab_shared=structured or args.lti) * B
            # every kernel family against the same HBM figure (algorithmic bytes / event-timed launch) with the PMC-measured
            # traffic of the committed profile next to it: the rollout is issue bound, the feed-forward pass is the one that streams
            families = {}
            for k in range(5):
                avg = fam[k][0] / max(1, fam[k][1])
                ach = abytes[k] * B / (avg * 1e-3) / 1e9 if avg > 0 else 0.0
                pmc = pmc_traffic(k, structured) if default_workload else None
                families[KIND_NAMES[k]] = {"avg_launch_ms": avg, "algorithmic_bytes_per_launch": abytes[k] * B, "achieved": ach,
                                           "frac": ach / HBM_PEAK_GBS, "pmc_bytes": pmc,
                                           "pmc_over_algorithmic": (pmc / (abytes[k] * B) if pmc and abytes[k] else None)}
            out["roofline"] = {"bound": "hbm", "kernel": KIND_NAMES[dom], "achieved": achieved, "peak": HBM_PEAK_GBS,
                               "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                               "traffic": pmc_traffic(dom, structured) if default_workload else None,
                               "avg_launch_ms": avg_ms, "algorithmic_bytes_per_launch": abytes[dom] * B,
                               "iteration_algorithmic_bytes": it_bytes,
                               "iteration_frac": it_bytes * (it_per_s / world) / 1e9 / HBM_PEAK_GBS,
                               "pmc_profile": os.path.basename(PMC_FILE) if (PMC_FILE and default_workload) else None,
                               "pmc_tree": pmc_tree() if default_workload else None,
                               "families": families}
            out["kernels_ms_per_step"] = {KIND_NAMES[k]: fam[k][0] / sampled for k in range(5)}
            out["launches_per_step"] = {KIND_NAMES[k]: fam[k][1] / sampled for k in range(5)}
            out["event_sampled_steps"] = sampled
        # what the collective layer saw: ranks that joined the process group (1 without one) and the RCCL build
        out["n_ranks_joined"] = int(dist.get_world_size()) if dist is not None else 1
        out["collective_backend"] = (dist.get_backend() if dist is not None else None)
        try:
            out["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            out["rccl_version"] = None
        if REHEARSAL:
            out["rehearsal"] = True                             # N ranks on one device over gloo: exercises the code path, measures nothing
        # --full: the CPU baseline is timed on rank 0 at N = 1 only (the key is present, null, on the other lines)
        out["cpu_baseline"] = (cpu_baseline(cfg, args, B, N, n, m, J, L)
                               if (args.full and not args.no_cpu_baseline and world == 1) else None)
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


# ---- configs 3 and 4 (`--config 3|4`): the nonlinear workloads of BASELINE.json at their full per-GPU size ---------------------
def secondary_config_main(args):
    """`bench.py --config 3`: 3R planar arm (n = 9, m = 3, N = 100, B = 4096), state + control boxes, J = 10 ADMM iterations x
    L = 5 candidates (notebooks/3DoF robot/State and control bound constraints.ipynb cells 22-23).
    `bench.py --config 4`: car (n = 4, m = 2, N = 200, B = 4096 per GPU), control box + two keep-out rectangles on the
    position (project_set_convex over the 200 position rows), J = 5 x L = 20 (notebooks/Car/Iterative LQR with state
    constraints.ipynb cell 18).  Same step as the headline (one C-driver call + isls_outer_advance + the reduction), early
    exit off; one JSON line with `roofline` of the dominant kernel family and `cpu_baseline` (the oracle on a sample)."""
    from isls import Box
    from isls import _capi as capi
    from isls.engine import library
    import isls_problems as P
    from test_full_size import _make
    pj = sys.modules["isls.projections"]
    torch.cuda.set_device(0)
    B = args.batch
    if args.config == 3:
        cfg = P.config3(batch=B, N=100, seed=0)
        N, L, J = 100, cfg["max_line_search"], cfg["max_admm_iter"]
        proj = dict(project_x=Box(cfg["x_lo"], cfg["x_hi"]), project_u=Box(cfg["u_lo"], cfg["u_hi"]), rho_x=cfg["rho_x"], rho_u=cfg["rho_u"])
        label = "config3: 3R planar arm iLQR-ADMM (DP form), boxes on joint velocities, final end-effector x and u"
    else:
        cfg = P.config4(batch=B, N=200, seed=0)
        N, L, J = 200, 20, 5
        rho_x = np.zeros((N, 4, 4)); rho_x[:, :2, :2] = 0.1 * np.eye(2)
        cs = pj.keepout_rectangles(4, [[-7.0, -3.0], [-3.0, -7.0]], [[2.0, 1.0], [2.0, 1.0]], -np.pi / 4)
        proj = dict(project_x=cs, project_u=Box(cfg["u_lo"], cfg["u_hi"]), rho_x=rho_x, rho_u=cfg["rho_u"])
        label = "config4: car iLQR-ADMM (DP form), control box + two keep-out rectangles on the position"
    n, m = cfg["n"], cfg["m"]
    s = _make(cfg, range(B))
    s._setup_admm(proj["project_x"], proj["project_u"], proj["rho_x"], proj["rho_u"], 1.0)
    e = s.engine
    e.outer_active.fill_(1)
    e.build_outer(L, J, tol_abs=0.0, tol_rel=0.0, begin_done=True)
    e.linearize(); e.expand(); e.begin_outer()
    lib = library()

    def step():
        e.run_outer()
        e.advance()
        e.reduce()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    timing = lib.isls_timing_create()
    e._outer_args.timing = timing
    lib.isls_timing_reset(timing)
    t0 = time.perf_counter()
    for i in range(args.steps):
        lib.isls_timing_pause(timing, 0 if i % EVENT_PERIOD == 0 else 1)
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    e._outer_args.timing = None
    fam = []
    for kind in range(5):
        cnt = ctypes.c_int(0)
        fam.append((lib.isls_timing_read_ms(timing, kind, ctypes.byref(cnt)), cnt.value))
    lib.isls_timing_destroy(timing)
    st = e.status.cpu().numpy()
    w, has_x, has_u = 8, e.zx is not None, e.zu is not None
    hess_shared = bool(e._shared_hessian())
    gain_ff = fam[1][1] < fam[2][1]
    abytes = algorithmic_bytes(n, m, N, w, has_x=has_x, has_u=has_u, lti=False, hess_shared=hess_shared, records=e.ff_record() is not None,
                               gain_ff=gain_ff)
    sampled = len(range(0, args.steps, EVENT_PERIOD))
    dom = int(np.argmax([ms for ms, _ in fam]))
    families = {}
    for k in range(5):
        avg = fam[k][0] / max(1, fam[k][1])
        ach = abytes[k] * B / (avg * 1e-3) / 1e9 if avg > 0 else 0.0
        families[KIND_NAMES[k]] = {"avg_launch_ms": avg, "launches_per_step": fam[k][1] / sampled, "ms_per_step": fam[k][0] / sampled,
                                   "algorithmic_bytes_per_launch": abytes[k] * B, "achieved": ach, "frac": ach / HBM_PEAK_GBS}
    it_per_s = args.steps / dt
    it_bytes = iteration_bytes(n, m, N, w, hess_shared, has_x=has_x, has_u=has_u) * B
    out = {"metric": f"iLQR-ADMM iterations/sec (config {args.config})", "value": it_per_s, "unit": "iterations/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": label, "batch_per_gpu": B, "horizon": N, "x_dim": n, "u_dim": m, "admm_iters_J": J, "line_search_L": L,
                      "layout": "time-varying A,B per trajectory (device linearisation)", "early_exit": False,
                      "state_constraint": "box" if args.config == 3 else "project_set_convex over two keep-out rectangles (device)",
                      "trajectory_iterations_per_s": it_per_s * B, "status_bits_set": int((st != 0).sum())},
           "roofline": {"bound": "hbm", "kernel": KIND_NAMES[dom], "achieved": families[KIND_NAMES[dom]]["achieved"], "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": families[KIND_NAMES[dom]]["frac"], "traffic": None,
                        "avg_launch_ms": families[KIND_NAMES[dom]]["avg_launch_ms"],
                        "algorithmic_bytes_per_launch": abytes[dom] * B, "iteration_algorithmic_bytes": it_bytes,
                        "iteration_frac": it_bytes * it_per_s / 1e9 / HBM_PEAK_GBS, "families": families},
           "cpu_baseline": None}
    if not args.no_cpu_baseline:
        from helpers import OracleDriver, problem_arrays
        from oracle import oracle as orc
        kern, olib = orc.load()
        cores = orc.set_threads(olib, host_cores())
        sample = args.cpu_sample or min(B, 256)
        scfg = P.config3(batch=sample, N=N, seed=0) if args.config == 3 else P.config4(batch=sample, N=N, seed=0)
        pa = problem_arrays(scfg, range(sample))
        if args.config == 3:
            d = OracleDriver(kern, pa, rho_x=scfg["rho_x"], rho_u=scfg["rho_u"], project_x=True)
        else:
            d = OracleDriver(kern, pa, rho_x=proj["rho_x"], rho_u=scfg["rho_u"], project_x=True, x_sets=proj["project_x"])
        d.run(1, L, J, 0.0)
        d.outer_active[:] = 1
        reps, t1 = 0, time.perf_counter()
        while True:
            d.run(1, L, J, 0.0)
            d.outer_active[:] = 1                              # the natural stop rules are not part of the timed work
            reps += 1
            el = time.perf_counter() - t1
            if el > 12.0 or reps >= 200:
                break
        tps = sample * reps / el
        out["cpu_baseline"] = {"value": tps / B, "unit": "iterations/s", "cores": cores, "kind": "port",
                               "sample": f"{reps} outer iterations (J={J}, L={L}) of {sample} trajectories of the same workload through the "
                                         f"oracle's kernels, {el:.1f} s, scaled linearly to batch {B}",
                               "trajectory_iterations_per_s": tps}
    print(json.dumps(out))


# ---- config 5 (SLS-ADMM with chance constraints): secondary workload, `--config5` ----------------------------------------
def config5_problem(B, nb_dim, N, seed=0):
    from isls import sls_dense as dense
    from isls.utils import get_double_integrator_AB
    pj = sys.modules["isls.projections"]
    rng = np.random.default_rng(seed)
    n, m, p = 2 * nb_dim, nb_dim, nb_dim
    A, Bm = get_double_integrator_AB(nb_dim, nb_deriv=2, dt=1.0 / N)
    Sw, Su = dense.transfer_matrices(A, Bm, N)
    targets = np.concatenate([rng.uniform(0.5, 1.5, (B, nb_dim)), np.zeros((B, nb_dim))], 1)
    zs = np.stack([np.zeros((B, n)), targets], 1)
    seq = np.zeros(N, dtype=np.int32); seq[N - 1] = 1
    Q, R, xd = dense.dense_cost(zs, np.stack([np.zeros((n, n)), 1e6 * np.eye(n)]), seq, 1e-2, N, n, m)
    rr = dense.rho_diagonal(1e2, N, m)
    Linv, r_side = dense.admm_sls_setup(Sw, Su, Q, R, xd, rr, p, B)
    # Bounds that every problem can meet: a rest-to-rest move of d in T = 1 needs |u| >= 4 d (bang-bang) and the unconstrained
    # optimum peaks at 6 d, so a bound of (4.8 .. 6.5) max_i d_i + 0.5 binds without making the ADMM iteration infeasible
    # (round 2 drew the bounds independently of the targets: a tenth of the problems did not contract and their fp32 / fp64
    # iterates differ by O(1))
    dmax = targets[:, :nb_dim].max(axis=1)
    ub = rng.uniform(4.8, 6.5, B) * dmax + 0.5
    cs = pj.chance_constraint_rows(p, ub, -ub, rng.uniform(0.005, 0.02, B), 1.6448536269514722)
    return Linv, r_side, rr, cs


def config5_run(kern, Linv, r_side, rr, cs, iters, dtype, wrap, sync, gpu_events=False):
    mk = lambda a: wrap(np.ascontiguousarray(a, dtype=dtype))   # noqa: E731
    sets = [{k: (mk(v) if isinstance(v, np.ndarray) else v) for k, v in st.items()} for st in cs.sets]
    x_u = wrap(np.zeros(r_side.shape, dtype=dtype))
    it = wrap(np.zeros(r_side.shape[0], dtype=np.int32))
    args = (mk(Linv), mk(r_side), mk(rr), sets, x_u)
    kw = dict(alpha=1.0, tol=0.0, rel_tol=0.0, max_iter=iters, rho=cs.rho, inner_max_iter=cs.max_iter, threshold=cs.threshold, iters=it)
    kern.sls_admm(*args, **kw)
    sync()
    t0 = time.perf_counter()
    reps = 0
    events = []
    while True:
        if gpu_events:                                           # the launch runs on torch's current stream
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        kern.sls_admm(*args, **kw)
        if gpu_events:
            ev[1].record()
            events.append(ev)
        reps += 1
        sync()
        if time.perf_counter() - t0 > 2.0 or reps >= 20:
            break
    wall = (time.perf_counter() - t0) / reps
    kernel_ms = sum(a.elapsed_time(b) for a, b in events) / len(events) if events else None
    return wall, x_u, kernel_ms


def config5_counters(dim, dtype_name, D):
    """Fractions of the wave cycles of sls_admm_kernel from the committed rocprofv3 SQ / TCC passes (tools/pmc_config5.sh)."""
    try:
        k = json.load(open(os.path.join(ROOT, "profiles", "r03_config5_pmc.json")))["kernels"]
        return k.get(f"d{dim} isls::sls_admm_kernel<{'float' if dtype_name == 'f32' else 'double'}, {D}, 256>")
    except (OSError, ValueError, KeyError):
        return None


def config5_main(args):
    """`bench.py --config5`: config 5 of BASELINE.json / SURVEY 8(d) -- SLS-ADMM with SOC chance constraints, N=50, B=8192
    problems that differ in target, bound and variance, fp32 and fp64.  One JSON line per precision: ADMM iterations/s over
    the whole batch (max_iter fixed, stop rules off so the work is constant), the CPU oracle timed beside it on a sample."""
    import isls  # noqa: F401
    from isls.engine import kernels
    torch.cuda.set_device(0)
    B, N, iters = (args.batch if args.batch != 4096 else 8192), (args.horizon if args.horizon != 100 else 50), 50
    Linv, r_side, rr, cs = config5_problem(B, args.config5_dim, N)
    hip = kernels()
    dev = lambda a: torch.from_numpy(a).cuda()                  # noqa: E731
    for dtype, name in ((np.float32, "f32"), (np.float64, "f64")):
        dt, x_u, kms = config5_run(hip, Linv, r_side, rr, cs, iters, dtype, dev, torch.cuda.synchronize, gpu_events=True)
        R_, D_ = r_side.shape[1], r_side.shape[2]
        w = 4 if dtype == np.float32 else 8
        # the one kernel of this workload (isls_sls_admm): per problem it reads its right-hand side and writes the iterate once
        # (the shared inverse stays in the L2), and every ADMM iteration is an [R x R] . [R x D] product plus the per-row
        # project_set_convex iterations (data dependent, not counted): it is bound by vector arithmetic and LDS, not by HBM,
        # and fp32 MFMA runs at the vector rate on gfx950 (MI355X_MICROARCH.md), so the peak is the 157.3 TFLOP/s of either
        flops = 2.0 * B * iters * R_ * R_ * D_
        vec_peak = 157.3 if dtype == np.float32 else 78.6
        out = {"metric": "SLS-ADMM iterations/sec (config 5)", "value": iters / dt, "unit": "iterations/s", "n_gpus": 1,
               "dtype": name, "data": "synthetic", "higher_is_better": True,
               "config": {"workload": f"config5: DI-{args.config5_dim}D SLS-ADMM, SOC chance constraints", "batch": B, "horizon": N,
                          "admm_iters": iters, "inner_max_iter": cs.max_iter},
               "problems_per_s": B / dt, "ms_per_solve": 1e3 * dt,
               "roofline": {"bound": "latency", "kernel": "sls_admm_kernel", "avg_launch_ms": kms,
                            "limiter": "L2 round trips on every row's dependent chain: rocprofv3 SQ counters of this kernel (committed "
                                       "profile below) show the wavefronts parked in s_waitcnt / s_barrier for most of their cycles, the vector "
                                       "ALU active for a fifth, the LDS for 1-3 %, HBM idle (39 MB per batch solve); neither the HBM nor a matrix roof applies",
                            "achieved": flops / (kms * 1e-3) / 1e12, "peak": vec_peak, "unit": "TFLOP/s",
                            "frac": flops / (kms * 1e-3) / 1e12 / vec_peak, "traffic": None,
                            "counters": config5_counters(args.config5_dim, name, D_), "pmc_profile": "r03_config5_pmc.json",
                            "algorithmic_flops_per_launch": flops,
                            "algorithmic_bytes_per_launch": 2.0 * B * R_ * D_ * w,
                            "hbm_achieved_GBs": 2.0 * B * R_ * D_ * w / (kms * 1e-3) / 1e9,
                            "note": "`achieved` / `frac` count the x-step's multiply-adds only, against the vector peak (fp32 MFMA runs at the "
                                    "vector rate on gfx950): a figure of merit, not the bound"}}
        if not args.no_cpu_baseline:                             # the CPU oracle, a reported baseline only
            from oracle import oracle as orc
            okern, olib = orc.load()
            cores = orc.set_threads(olib, host_cores())
            sample = min(B, 1024)
            cs_s = type(cs)(cs.dim, cs.cols, [{k: (v[:sample] if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[0] == B else v)
                                               for k, v in st.items()} for st in cs.sets], rho=cs.rho, max_iter=cs.max_iter,
                            threshold=cs.threshold)
            dtc, x_c, _ = config5_run(okern, Linv, r_side[:sample], rr, cs_s, iters, dtype, lambda a: a, lambda: None)
            d = np.abs(x_u.cpu().numpy()[:sample].astype(np.float64) - x_c.astype(np.float64)).reshape(sample, -1).max(1)
            d = d / np.abs(x_c.astype(np.float64)).reshape(sample, -1).max(1)
            out["cpu_baseline"] = {"value": iters / (dtc * B / sample), "unit": "iterations/s", "cores": cores, "kind": "port",
                                   "sample": f"{sample} problems, scaled linearly to {B}"}
            # problems whose bound is infeasible do not contract and amplify rounding differences: median and max
            out["rel_diff_vs_oracle_on_sample"] = {"median": float(np.median(d)), "max": float(np.max(d)),
                                                   "problems_above_1e-4": int(np.sum(d > 1e-4)), "sample": int(sample)}
        print(json.dumps(out))


# ---- iSLS.isls_admm: secondary workload, `--isls-admm` ---------------------------------------------------------
def isls_admm_main(args):
    """`bench.py --isls-admm`: the robust-control notebook's call (3R arm, chance constraint on the controls with respect to
    the initial joint angles, dim = 3, 10 ADMM iterations, 30 line-search candidates) for a batch of arms that differ in
    their initial configuration; outer iterations per second over the whole batch, the dense numpy oracle timed beside it
    on a few problems."""
    import isls
    import isls_problems as P
    from isls import models
    from isls.projections import chance_constraint_rows
    from scipy.stats import norm
    torch.cuda.set_device(0)
    B, N = (args.batch if args.batch != 4096 else 1024), args.horizon
    J, L, outer = 10, 30, max(1, args.steps)
    cfg = P.config3(batch=B, N=N, seed=0)
    cfg["u0"] = np.zeros_like(cfg["u0"])
    cs = chance_constraint_rows(3, 6.0, -6.0, 0.1, float(norm.ppf(0.82)), rho=10.0, max_iter=100, threshold=1e-4)

    def fresh(bsel):
        s = isls.iSLS(cfg["n"], cfg["m"], N, batch=len(bsel))
        s.forward_model = models.Planar3R(cfg["dt"])
        s.set_cost_variables(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
        xs, us = zip(*[P.initial_nominal(cfg, b) for b in bsel])
        s.reset()
        s.nominal_values = np.stack(xs), np.stack(us)
        return s
    kw = dict(max_line_search=L, project_u=cs, rho_u=1.0, max_admm_iter=J, threshold=0.0)
    s = fresh(range(B))
    s.isls_admm(3, None, k_max=1, **kw)                                         # warm-up

    # `value` is the steady state: the outer iterations after the first (whose ADMM set-up is per call), timed from a mark
    # the loop sets there to the return of the call, i.e. with the read-back of the results spread over them.  The loop
    # itself (t1 -> t2, device synchronised at both) and the read-back (t2 -> return) are reported separately; a call is
    # ~0.1 s, `value` is the best of three and all three are in `ms_per_outer_iteration_calls`
    best, calls = None, []
    for _ in range(3):
        s = fresh(range(B))
        s._bench_mark = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.isls_admm(3, None, k_max=outer + 1, **kw)
        torch.cuda.synchronize()
        t_end = time.perf_counter()
        ran_after = max(1.0, float(np.max(s.outer_iters)) - 1.0)
        cand = ((t_end - s._bench_mark["t1"]) / ran_after, t_end - t0, s._bench_mark["t1"] - t0, s,
                (s._bench_mark["t2"] - s._bench_mark["t1"]) / ran_after, t_end - s._bench_mark["t2"])
        calls.append(1e3 * cand[0])
        if best is None or cand[0] < best[0]:
            best = cand
    per_iter, dt, first, s, loop_iter, read_back = best
    first_call_overhead = first - per_iter
    short = 0
    # the same call once more with HIP events around the kernel families of the ADMM iteration (kept out of `value`: an
    # event pair per launch costs queue bubbles on launches this short)
    s2 = fresh(range(B))
    s2.engine.profile_events = {}
    s2.isls_admm(3, None, k_max=outer, **kw)
    fam = s2.engine.family_ms()
    s2.engine.profile_events = None
    done2 = float(np.max(s2.outer_iters))             # outer iterations of the event-timed call
    done = float(np.max(s.outer_iters))               # outer iterations the batch ran (problems that met the reference's stop rules idle)
    out = {"metric": "isls_admm outer iterations/sec (3R arm, robust control bounds)", "value": 1.0 / per_iter, "unit": "iterations/s",
           "n_gpus": 1, "dtype": "f64", "data": "synthetic", "higher_is_better": True,
           "config": {"workload": "isls_admm: 3R arm, chance constraint on u w.r.t. q0 (dim 3)", "batch": B, "horizon": N,
                      "admm_iters_J": J, "line_search_L": L, "outer_iterations_run": done, "outer_iterations_mean_per_problem": float(np.mean(s.outer_iters))},
           "ms_per_outer_iteration": 1e3 * per_iter, "problem_iterations_per_s": B / per_iter,
           "ms_per_outer_iteration_calls": calls,              # the three timed calls; `value` is from the smallest
           "loop_ms_per_outer_iteration": 1e3 * loop_iter,      # of that call: the loop alone, device synchronised at both ends
           "read_back_ms_per_call": 1e3 * read_back,            # of that call: status, logs and [d_u, phi_u] to the host
           "per_call_set_up_ms": 1e3 * first_call_overhead,     # first outer iteration minus a steady-state one, once per isls_admm call
           "whole_call_ms_per_outer_iteration": 1e3 * dt / (outer + 1),
           "final_cost_mean": float(np.mean(s.cost))}
    # roofline of the dominant kernel family (event-timed on the launch stream); algorithmic HBM bytes per launch, w = 8:
    #   project_rows   : the [B, N m, C] rows in and out (the sets are a few hundred shared bytes)
    #   riccati_ff     : one column's pass: packed records + c0, targets in, k out
    #   columns_rollout: A, B, K, k[C] in, dx[C], du[C] out ;  rollout_ls: the line search's 36 KB-per-trajectory figure at n = 9
    n, m, C, w = cfg["n"], cfg["m"], 4, 8
    rec = n * n + 2 * n * m + m * m
    abytes = {"project_rows": 2 * B * N * m * C * w, "riccati_ff": B * N * (rec + (n + m) + 3 * m + m) * w,
              "columns_rollout": B * N * (n * n + n * m + m * n + C * m + C * (n + m)) * w,
              "rollout_ls": B * N * (m + (n + m) + (n + m)) * w}
    if fam:
        dom = max(fam, key=lambda k: fam[k][0])
        avg = fam[dom][0] / max(1, fam[dom][1])
        ach = abytes[dom] / (avg * 1e-3) / 1e9
        out["roofline"] = {"bound": "hbm", "kernel": dom, "avg_launch_ms": avg, "achieved": ach, "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None,
                           "algorithmic_bytes_per_launch": abytes[dom],
                           "families": {k: {"ms_per_outer_iteration": v[0] / done2, "launches_per_outer_iteration": v[1] / done2,
                                            "avg_launch_ms": v[0] / max(1, v[1]),
                                            "frac": abytes[k] / (v[0] / max(1, v[1]) * 1e-3) / 1e9 / HBM_PEAK_GBS}
                                        for k, v in fam.items()}}
    if not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from helpers import problem_arrays
        from oracle import oracle as orc
        from oracle.isls_admm_dense import DenseIslsAdmm, shifted_sets_projection
        okern, olib = orc.load()
        orc.set_threads(olib, 1)
        sample = 2
        t0 = time.perf_counter()
        for b in range(sample):
            d = DenseIslsAdmm(okern, problem_arrays(cfg, [b]), 3, project_u=shifted_sets_projection(okern, cs), rho_u=1.0, threshold=0.0)
            d.solve(1, J, L)
        dtc = (time.perf_counter() - t0) / sample
        out["cpu_baseline"] = {"value": 1.0 / (dtc * B), "unit": "iterations/s", "cores": 1, "kind": "port",
                               "sample": f"{sample} problems x 1 outer iteration of the dense numpy restatement, scaled linearly to {B}"}
    print(json.dumps(out))


def host_cores():
    """Cores this process may really use: affinity mask, capped by the cgroup CPU quota when there is one."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return min(n, int(os.environ.get("ISLS_CPU_BASELINE_THREADS", "16")))


def cpu_baseline(cfg, args, B, N, n, m, J, L):
    """The CPU oracle (C port of the reference algorithm, OpenMP over trajectories) timed on this box's host
    cores on a bounded sample of the same workload.  A reported baseline only -- never the measured path."""
    from helpers import OracleDriver, problem_arrays
    from oracle import oracle as orc
    import isls_problems as P

    kern, lib = orc.load()
    cores = orc.set_threads(lib, host_cores())
    sample = args.cpu_sample or min(B, 4096)
    scfg = P.config2(batch=sample, N=N, seed=0)
    pa = problem_arrays(scfg, range(sample))
    d = OracleDriver(kern, pa, rho_u=scfg["rho_u"], relax=scfg["relax"])
    d.run_c(L, J)                                             # warm-up iteration
    reps, t0 = 0, time.perf_counter()
    while True:
        d.run_c(L, J)                                         # linearise+expand, C driver, accept
        reps += 1
        el = time.perf_counter() - t0
        if el > 12.0 or reps >= 2000:                         # ~12 s of CPU work on all host cores
            break
    traj_it_per_s = sample * reps / el
    return {"value": traj_it_per_s / B, "unit": "iterations/s", "cores": cores, "kind": "port",
            "sample": f"{reps} outer iterations (J={J}, L={L}) of {sample} trajectories of the same workload, "
                      f"{el:.1f} s, scaled linearly to batch {B} (trajectories are independent)",
            "trajectory_iterations_per_s": traj_it_per_s}


if __name__ == "__main__":
    sys.exit(main() or 0)
