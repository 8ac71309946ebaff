"""CPU-side checks of the boundary: the HIP library loads and exports every entry point include/isls_hip.h
declares (no compute call -- there is no GPU here), the ctypes structs mirror the header, the strided-view
marshaling and the sharding / reduction logic (world_size 2 over gloo)."""
import ctypes
import os
import re

import numpy as np
import pytest

from isls import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(ROOT, "include", "isls_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(isls_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = capi.load_hip_library()
    names = header_functions()
    assert len(names) >= 20
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert sorted(capi.EXPORTED) == names                      # the binding knows exactly the header's surface
    lib.isls_version.restype = ctypes.c_int
    assert lib.isls_version() == capi.ABI_VERSION == 107
    assert b"unsupported" in lib.isls_error_string(capi.ERR_UNSUPPORTED)


def test_struct_layouts_match_header():
    """sizeof of every argument struct as compiled from the header by gcc == ctypes' layout."""
    import subprocess
    import tempfile
    names = ["gain", "ff", "ff_prepare", "rollout", "admm", "project", "sls_admm", "expand", "linearize", "accept", "outer",
             "columns", "columns_admm", "dense_loop", "advance", "columns_iteration"]
    src = '#include <stdio.h>\n#include "isls_hip.h"\nint main(){' + "".join(
        f'printf("%zu\\n", sizeof(isls_{n}_args));' for n in names) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    structs = [capi.GainArgs, capi.FfArgs, capi.FfPrepareArgs, capi.RolloutArgs, capi.AdmmArgs, capi.ProjectArgs, capi.SlsAdmmArgs, capi.ExpandArgs, capi.LinearizeArgs,
               capi.AcceptArgs, capi.OuterArgs, capi.ColumnsArgs, capi.ColumnsAdmmArgs, capi.DenseLoopArgs, capi.AdvanceArgs, capi.ColumnsIterationArgs]
    assert sizes == [ctypes.sizeof(s) for s in structs]


def test_record_buffer_size_matches_the_library():
    """isls_ff_record_elems (the packed-record buffer is blocked by wavefront, so its size is padded to whole wavefronts)"""
    lib = capi.load_hip_library()
    lib.isls_ff_record_elems.restype = ctypes.c_int64
    for B, N, n, m in ((1, 2, 2, 1), (7, 100, 6, 3), (8, 100, 6, 3), (4096, 100, 6, 3), (33, 40, 9, 3), (5, 200, 4, 2)):
        got = lib.isls_ff_record_elems(ctypes.c_int32(B), ctypes.c_int32(N), ctypes.c_int32(n), ctypes.c_int32(m))
        assert got == capi.ff_record_elems(B, N, n, m) >= B * N * (n * n + 2 * n * m + m * m)


def test_make_view_strides():
    B, N, n = 5, 7, 3
    dense = np.zeros((B, N, n, n))
    v = capi.make_view(dense, B, N, (n, n), "A")
    assert (v.sb, v.st) == (N * n * n, n * n)
    v = capi.make_view(np.zeros((n, n)), B, N, (n, n), "A")
    assert (v.sb, v.st) == (0, 0)
    v = capi.make_view(np.zeros((N, n, n)), B, N, (n, n), "A")
    assert (v.sb, v.st) == (0, n * n)
    v = capi.make_view(np.zeros((B, 1, n, n)), B, N, (n, n), "A")          # per-trajectory LTI
    assert (v.sb, v.st) == (n * n, 0)
    v = capi.make_view(np.broadcast_to(np.zeros((1, 1, n, n)), (B, N, n, n)), B, N, (n, n), "A")
    assert (v.sb, v.st) == (0, 0)
    assert capi.make_view(None, B, N, (n,), "x").p is None
    with pytest.raises(ValueError):
        capi.make_view(np.zeros((B, N, n, n + 1)), B, N, (n, n), "A")
    with pytest.raises(ValueError):
        capi.make_view(np.zeros((B, N, n, n)).transpose(0, 1, 3, 2), B, N, (n, n), "A")


def test_argument_validation_without_gpu():
    """Bad arguments are rejected on the host side before anything touches a device."""
    lib = capi.load_hip_library()
    a = capi.GainArgs(B=4, N=10, n=6, m=3)
    lib.isls_riccati_gain_f64.restype = ctypes.c_int
    assert lib.isls_riccati_gain_f64(ctypes.byref(a), None) == capi.ERR_ARG            # null pointers
    assert lib.isls_riccati_gain_f64(None, None) == capi.ERR_ARG
    r = capi.RolloutArgs(B=1, N=10, n=6, m=3, L=65)
    lib.isls_rollout_ls_f64.restype = ctypes.c_int
    assert lib.isls_rollout_ls_f64(ctypes.byref(r), None) == capi.ERR_ARG               # L > 64
    k = capi.Kernels(lib)
    with pytest.raises(ValueError):
        k.gain_args(np.zeros((2, 2)), np.zeros((2, 1)), np.zeros((2, 2)), np.zeros((1, 1)), np.zeros((3, 5, 1, 2)),
                    np.zeros((3, 5, 1, 1)), np.zeros((3, 5, 1, 1)), np.zeros((3, 5, 2, 2)))   # Qux has the wrong shape


def test_sls_admm_refusals_without_gpu():
    """isls_sls_admm checks its argument block before it touches a device: an empty batch is ISLS_OK (and launches nothing); more
    rows than the largest workgroup (1025), no iterations, a penalty that is not positive, a set without its A -- each
    ISLS_ERR_ARG, in both precisions; an unknown set kind is ISLS_ERR_UNSUPPORTED."""
    k = capi.Kernels(capi.load_hip_library(), prefix="isls_", with_stream=True)
    for dtype in (np.float64, np.float32):
        def call(R=8, sets=None, P=3, **kw):
            z = lambda *shape: np.zeros(shape, dtype=dtype)                              # noqa: E731
            sets = [dict(kind=capi.SET_BOX, dim=2, A=z(2, 2), b=z(2), par=z(4))] if sets is None else sets
            return k.sls_admm(z(R, R), z(P, R, 2), z(R), sets, z(P, R, 2), **kw)
        # the block the refusals start from is itself accepted: with no problem in it every check runs and nothing is launched,
        # so each refusal below is the work of the one field it changes
        assert call(P=0) == capi.OK and call(P=0, R=1024) == capi.OK
        refused = pytest.raises(capi.IslsError, match=rf"-> {capi.ERR_ARG}\b")
        with refused:
            call(R=1025)
        with refused:
            call(max_iter=0)
        with refused:
            call(rho=0.0)
        with refused:
            call(sets=[dict(kind=capi.SET_BOX, dim=2, b=np.zeros(2, dtype=dtype), par=np.zeros(4, dtype=dtype))])
        with pytest.raises(capi.IslsError, match=rf"-> {capi.ERR_UNSUPPORTED}\b"):
            call(sets=[dict(kind=8, dim=2, A=np.zeros((2, 2), dtype=dtype), b=np.zeros(2, dtype=dtype), par=np.zeros(4, dtype=dtype))])


def test_shard_range():
    from isls.shard import shard_range
    for B, W in ((4096, 8), (10, 3), (7, 8)):
        cuts = [shard_range(B, r, W) for r in range(W)]
        assert cuts[0][0] == 0 and cuts[-1][1] == B
        assert all(cuts[i][1] == cuts[i + 1][0] for i in range(W - 1))
        assert max(h - l for l, h in cuts) - min(h - l for l, h in cuts) <= 1


def _rank_main(rank, world, port, B, ret):
    import torch
    import torch.distributed as dist

    import isls_problems as P
    from helpers import OracleDriver, problem_arrays
    from isls.shard import allreduce_convergence, shard_range
    from oracle import oracle as orc
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    kern, _ = orc.load()
    cfg = P.config2(batch=B, N=30, seed=0)
    lo, hi = shard_range(B, rank, world)
    d = OracleDriver(kern, problem_arrays(cfg, range(lo, hi)), rho_u=cfg["rho_u"])
    d.run_c(8, 2)
    out5 = np.zeros(5)
    kern.reduce_convergence(d.cost, d.res, d.outer_active, d.status, out5)
    total, table = allreduce_convergence(torch.from_numpy(out5), rank, world)
    ret[rank] = (total.numpy().copy(), table.numpy().copy(), d.xhat.copy())
    dist.destroy_process_group()


def test_two_rank_sharding_matches_single_process(oracle):
    """The N>1 path: two gloo ranks, each solving its shard with the same kernels' CPU oracle, exchange only the
    [W,5] convergence table; trajectories and the reduced summary equal the single-process run."""
    import torch.multiprocessing as mp

    import isls_problems as P
    from helpers import OracleDriver, problem_arrays
    B, world = 9, 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_rank_main, args=(world, 29517, B, ret), nprocs=world, join=True)
    cfg = P.config2(batch=B, N=30, seed=0)
    d = OracleDriver(oracle, problem_arrays(cfg, range(B)), rho_u=cfg["rho_u"])
    d.run_c(8, 2)
    full = np.zeros(5)
    oracle.reduce_convergence(d.cost, d.res, d.outer_active, d.status, full)
    x = np.concatenate([ret[r][2] for r in range(world)])
    assert np.array_equal(x, d.xhat)
    for r in range(world):
        total, table = ret[r][0], ret[r][1]
        assert table.shape == (world, 5)
        assert abs(total[0] - full[0]) < 1e-9 * max(1.0, abs(full[0]))
        assert np.allclose(total[1:], full[1:], rtol=1e-15, atol=0)


def test_timing_context_is_caller_owned():
    """isls_timing_*: create / reset / pause / read / destroy on a handle; nothing is recorded without launches, a NULL handle
    is rejected (the library keeps no timing state of its own)."""
    lib = capi.load_hip_library()
    h = lib.isls_timing_create()
    assert h
    assert lib.isls_timing_reset(h) == capi.OK and lib.isls_timing_pause(h, 1) == capi.OK
    cnt = ctypes.c_int(-1)
    assert lib.isls_timing_read_ms(h, 2, ctypes.byref(cnt)) == 0.0 and cnt.value == 0
    assert lib.isls_timing_read_ms(h, 9, ctypes.byref(cnt)) < 0
    assert lib.isls_timing_reset(None) == capi.ERR_ARG and lib.isls_timing_read_ms(None, 0, None) < 0
    lib.isls_timing_destroy(h)
    assert ctypes.sizeof(capi.OuterArgs) % 8 == 0 and capi.OuterArgs.timing.offset == ctypes.sizeof(capi.OuterArgs) - 8


def test_bench_refuses_more_gpus_than_devices():
    """`python bench.py --gpus N` must never print an N-GPU line from fewer devices: without N visible HIP devices (none at
    all in the build container) it exits non-zero with a message, before touching a GPU."""
    import subprocess
    import sys
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--gpus 64" in r.stderr and "device" in r.stderr
    assert not r.stdout.strip()


def test_hot_path_kernels_keep_their_registers():
    """Resource table of the built library (tools/scan_kernels.py reads the gfx950 code objects, no GPU): the kernels of
    the headline outer iteration (n = 6, m = 3, fp64) and of config 5 hold their per-step state in registers.  Scratch
    inside a step loop halves these kernels ('occupancy steps and spills'); the roll-out's few spilled words
    sit outside its time loops (stored before and reloaded behind the winner replay, which only a mispredicted winner
    runs), so it gets a small allowance instead of zero."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import scan_kernels
    finally:
        sys.path.pop(0)
    tab = scan_kernels.kernel_table(capi.library_path() if hasattr(capi, "library_path") else scan_kernels.DEFAULT_LIB)
    assert len(tab) > 600

    def pick(prefix):
        hit = {k: v for k, v in tab.items() if k.startswith("_ZN4isls" + prefix)}
        assert hit, prefix
        return hit
    for prefix in ("19riccati_gain_kernelIdLi6ELi3E", "21riccati_ffrec2_kernelIdLi6ELi3E", "20riccati_ffrec_kernelIdLi6ELi3E",
                   "17riccati_ff_kernelIdLi6ELi3E", "18admm_update_kernelId", "13expand_kernelId", "16linearize_kernelId",
                   "27columns_rollout_rows_kernel", "19columns_admm_kernel"):
        for k, v in pick(prefix).items():
            assert v["scratch"] == 0, (k, v)
    for k, v in pick("14rollout_kernelIdLi6ELi3ELi3E").items():        # the headline's double-integrator roll-out
        assert v["scratch"] <= 96 and v["vgpr"] <= (256 if k.endswith("Li2EEEvNS_3RoPIT_EE") else 512), (k, v)
    for prec, d in (("f", (1, 2, 3, 4)), ("d", (1,))):                 # config 5 in the widths that run at 256 threads
        for D in d:
            for fam in ("15sls_admm_kernelI", "19project_rows_kernelI"):
                v = pick(f"{fam}{prec}Li{D}ELi256E")
                (k, r), = v.items()
                # the fp32 forms for rows of 3-4 entries are held to 128 registers (four wavefronts per SIMD): a bounded spill is
                # the price (round 3: 188 B with the set operands read from LDS -- and 13-19 % faster than the 156 B form)
                assert r["scratch"] <= (192 if prec == "f" and D >= 3 and fam.startswith("15") else 0), (k, r)


def _exchange_rank(rank, world, port, posts, ret):
    import torch
    import torch.distributed as dist

    from isls.shard import TableExchange, summarize
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    xch = TableExchange(world, rank, torch.float64, "cpu")
    seen = []

    def fill_for(i):
        def fill(table, r):                                   # what Engine.reduce(table=, rank=) leaves: own row, zeros elsewhere
            table.fill_(99.0)                                 # stale contents of the rotating table must not survive
            table.zero_()
            table[r] = torch.tensor([10.0 * i + r, i + 0.5 * r, i + 0.25 * r, 3.0 + r, float(i == 2 and r == 1)], dtype=torch.float64)
        return fill
    assert xch.finish() is None and xch.latest() is None
    for i in range(posts):
        xch.post(fill_for(i))
        late = xch.latest(lag=1)                              # the host reads the table one iteration late
        seen.append(None if late is None else late.clone().numpy())
    last = xch.finish().clone()
    ret[rank] = (seen, last.numpy(), summarize(last).numpy())
    dist.destroy_process_group()


def test_asynchronous_table_exchange_two_ranks():
    """isls.shard.TableExchange (what bench.py posts after every outer iteration): the all-reduce is started without a wait,
    tables rotate, a table is waited for before it is refilled, the host reads one iteration late; world 2 over gloo."""
    import torch.multiprocessing as mp
    world, posts = 2, 5
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_exchange_rank, args=(world, 29531, posts, ret), nprocs=world, join=True)

    def expected(i):
        return np.array([[10.0 * i + r, i + 0.5 * r, i + 0.25 * r, 3.0 + r, float(i == 2 and r == 1)] for r in range(world)])
    for r in range(world):
        seen, last, total = ret[r]
        assert seen[0] is None
        for i in range(1, posts):
            assert np.array_equal(seen[i], expected(i - 1)), (r, i)
        assert np.array_equal(last, expected(posts - 1))
        e = expected(posts - 1)
        assert np.array_equal(total, [e[:, 0].sum(), e[:, 1].max(), e[:, 2].max(), e[:, 3].sum(), e[:, 4].sum()])


def test_table_exchange_single_rank_needs_no_process_group():
    import torch

    from isls.shard import TableExchange
    xch = TableExchange(1, 0, torch.float64, "cpu")
    for i in range(3):
        t = xch.post(lambda table, r, i=i: table.copy_(torch.full((1, 5), float(i), dtype=torch.float64)))
        assert float(t[0, 0]) == i
    assert float(xch.latest(lag=1)[0, 0]) == 1.0 and float(xch.finish()[0, 0]) == 2.0


def test_bench_byte_formulas():
    """bench.py's algorithmic byte counts: the SURVEY 8(d) figure with z, lambda counted for the constrained blocks only (config 2
    constrains u alone: 373.6 MB per outer iteration with the batch-shared Hessian tables), and the per-kernel
    figures the roofline fractions are quoted against."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    n, m, N, w, B = 6, 3, 100, 8, 4096
    assert b.iteration_bytes(n, m, N, w, True, has_x=False, has_u=True) * B == 373_555_200
    assert b.iteration_bytes(n, m, N, w, False, has_x=True, has_u=True) == w * N * (2 * n * n + 2 * n * m + m * m + m + 7 * (n + m))   # 146 400 B
    gain, ff, ro, admm, prep = b.algorithmic_bytes(n, m, N, w, has_x=False, has_u=True, lti=False, hess_shared=True, records=True, gain_ff=True)
    assert ro * B == 147_456_000 and ff * B == 334_233_600 and gain * B == 304_742_400
    # the double integrator recognised (isls_gain_args.lin_on / isls_ff_args.lin_on): no A, B for the gain pass (36 + 18 words per
    # step less), [K | fac] = 27 of a record's 81 words for a feed-forward pass, and no A, B in the iteration's figure
    gain_s, ff_s, ro_s, _, _ = b.algorithmic_bytes(n, m, N, w, has_x=False, has_u=True, lti=False, hess_shared=True, records=True, gain_ff=True,
                                                   structured=True)
    assert ro_s == ro and (ff - ff_s) == w * N * 54 and (gain - gain_s) == w * N * 54
    assert ff_s * B == 157_286_400 and gain_s * B == 127_795_200
    assert b.iteration_bytes(n, m, N, w, True, has_x=False, has_u=True, ab_shared=True) * B == 373_555_200 - w * N * 54 * B == 196_608_000
