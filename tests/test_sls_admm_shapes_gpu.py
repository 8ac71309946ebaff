"""isls_sls_admm_* and isls_sls_closed_loop_* (csrc/sls_admm.hip) at every row width D, every workgroup size BLOCK and every set
kind, on synthetic problems: against the C oracle, against a plain numpy loop, at the stop rules, and for the invariants of a
launch (one workgroup per problem, optional outputs, shared against per-problem set operands).

The golden config-5 cases have R = N m = 50 and 150 rows of width 2 and 4 and two ISLS_SET_SOC_UNIT sets: sls_admm_kernel<T, D, 256>
with one or three wavefronts and no parameter block.  Here R runs over both sides of every block boundary (threads = R rounded
up to a wavefront; BLOCK = 256 / 512 / 1024 for threads <= 256 / <= 512 / above), and the sets carry parameter blocks that
stage_sets_lds copies to LDS and project_primitive reads from there.

Inputs (one recipe, `_case`): G = randn(R, max(2, R // 8)) / sqrt(R), rr = 0.5 + rand(R), Linv = inv(I + G G' + diag(rr))
symmetrised exactly (the kernel reads column r as row r), r_side = randn(P, R, D), every set with A = 0.7 randn(P, dim, D) and
b = 0.2 randn(P, dim) (+ 1 on the last entry of a SOC image), parameter blocks as include/isls_hip.h lays them out with bounds
of a few tenths so that the constraints are active.  fp32 runs get the fp64 inputs rounded to fp32.
"""
import importlib

import numpy as np
import pytest

from isls import _capi as capi

pytestmark = pytest.mark.gpu

BOX, SOC, SQUARE, LINEAR, QUAD, SHELL, MLIN = (capi.SET_BOX, capi.SET_SOC_UNIT, capi.SET_SQUARE, capi.SET_LINEAR, capi.SET_QUADRATIC,
                                               capi.SET_SHELL, capi.SET_MULTILINEAR)
# fixed iteration counts: with tol = rel_tol = 0 no outer stop rule can fire, with threshold = 0 not the inner threshold rule --
# only the inner 1e-5 stall rule is left, and the result is a smooth function of the inputs (fp32 can be compared with fp64)
FIXED = dict(max_iter=6, inner_max_iter=4, rho=2.0, alpha=1.5, tol=0.0, rel_tol=0.0, threshold=0.0)


def _block(R):
    threads = (R + 63) // 64 * 64
    return 256 if threads <= 256 else (512 if threads <= 512 else 1024)


def _set(rng, kind, P, D, dim=None, q=None):
    """One set with per-problem operands [P, ...] in fp64 (`_operands` hands them over per problem, shared or tiled)."""
    dim = (min(D + 1, 5) if kind == SOC else D) if dim is None else dim
    A, b = 0.7 * rng.standard_normal((P, dim, D)), 0.2 * rng.standard_normal((P, dim))
    st = dict(kind=kind, dim=dim, A=A, b=b)
    col = lambda v: np.full((P, 1), float(v))                                            # noqa: E731
    if kind == SOC:
        b[:, -1] += 1.0
    elif kind == BOX:                                          # lo[dim], hi[dim]
        st["par"] = np.concatenate([-0.1 - 0.2 * rng.random((P, dim)), 0.1 + 0.2 * rng.random((P, dim))], axis=1)
    elif kind == LINEAR:                                       # l, u, a[dim]
        st["par"] = np.concatenate([col(-0.2) - 0.1 * rng.random((P, 1)), col(0.15) + 0.1 * rng.random((P, 1)),
                                    rng.standard_normal((P, dim))], axis=1)
    elif kind == QUAD:                                         # l, u: 0.1 <= |y| <= 0.24 .. 0.32 (no lower bound on a line: sign flips)
        st["par"] = np.concatenate([col(0.005 if dim > 1 else 0.0), col(0.03) + 0.02 * rng.random((P, 1))], axis=1)
    elif kind == SHELL:                                        # l, u, c[dim]
        st["par"] = np.concatenate([col(0.005 if dim > 1 else 0.0), col(0.04) + 0.02 * rng.random((P, 1)),
                                    0.2 * rng.standard_normal((P, dim))], axis=1)
    elif kind == MLIN:                                         # q, l[q], u[q], M[q * dim]
        q = 1 if q is None else q
        M = rng.standard_normal((P, q, dim)) * (0.3 if q == dim else 1.0) + (1.5 * np.eye(dim) if q == dim else 0.0)
        st["par"] = np.concatenate([col(q), -0.1 - 0.1 * rng.random((P, q)), 0.1 + 0.1 * rng.random((P, q)), M.reshape(P, -1)], axis=1)
    elif kind == SQUARE:                                       # q, l, u, c[q], W[q * q], Winv[q * q]
        q = dim if q is None else q
        W = np.eye(q) + 0.2 * rng.standard_normal((P, q, q))
        st["par"] = np.concatenate([col(q), col(0.05), col(0.25) + 0.1 * rng.random((P, 1)), 0.1 * rng.standard_normal((P, q)),
                                    W.reshape(P, -1), np.linalg.inv(W).reshape(P, -1)], axis=1)
    return st


_CASES = {}


def _case(R, D, kinds, P=4, seed=0, scale=None):
    """kinds: tuple of SET_* or (SET_*, dict(dim=, q=)).  scale [P]: factor on r_side per problem."""
    key = (R, D, kinds if all(isinstance(k, int) for k in kinds) else repr(kinds), P, seed, None if scale is None else tuple(scale))
    if key not in _CASES:
        rng = np.random.default_rng(1000 * R + 10 * D + seed)
        G = rng.standard_normal((R, max(2, R // 8))) / np.sqrt(R)
        rr = 0.5 + rng.random(R)
        Linv = np.linalg.inv(np.eye(R) + G @ G.T + np.diag(rr))
        Linv = 0.5 * (Linv + Linv.T)
        assert np.array_equal(Linv, Linv.T)
        r_side = rng.standard_normal((P, R, D))
        if scale is not None:
            r_side *= np.asarray(scale, dtype=np.float64)[:, None, None]
        sets = [_set(rng, *((k, P, D) if isinstance(k, int) else (k[0], P, D, k[1].get("dim"), k[1].get("q")))) for k in kinds]
        _CASES[key] = dict(R=R, D=D, P=P, Linv=Linv, rr=rr, r_side=r_side, sets=sets)
    return _CASES[key]


def _operands(sets, how, sel=None):
    """how: 'per' [P, ...] operands, 'shared' problem 0's for all ([...]: stride 0), 'tiled' problem 0's repeated to [P, ...]."""
    out = []
    for st in sets:
        o = dict(kind=st["kind"], dim=st["dim"])
        for k in ("A", "b", "par"):
            if k in st:
                v = st[k]
                if how == "shared":
                    v = v[0]
                elif how == "tiled":
                    v = np.repeat(v[:1], v.shape[0], axis=0)
                o[k] = v if sel is None or how == "shared" else v[sel]
        out.append(o)
    return out


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _solve(kern, c, how="per", dtype=np.float64, wrap=lambda a: a, sel=None, outputs=True, **kw):
    """kern.sls_admm on the problems `sel` (all: None) of case c; outputs NaN-filled before -> dict of numpy arrays."""
    par = dict(FIXED, **kw)
    idx = list(range(c["P"])) if sel is None else list(sel)
    P_, R, D = len(idx), c["R"], c["D"]
    mk = lambda a: wrap(np.ascontiguousarray(a, dtype=dtype))                            # noqa: E731
    sets = [{k: (mk(v) if isinstance(v, np.ndarray) else v) for k, v in st.items()} for st in _operands(c["sets"], how, idx)]
    out = dict(x_u=wrap(np.full((P_, R, D), np.nan, dtype=dtype)))
    if outputs:
        out.update(z=wrap(np.full((P_, R, D), np.nan, dtype=dtype)), lmb=wrap(np.full((P_, R, D), np.nan, dtype=dtype)),
                   logs=wrap(np.full((P_, par["max_iter"], 2), np.nan, dtype=dtype)), iters=wrap(np.full(P_, -1, dtype=np.int32)))
    kern.sls_admm(mk(c["Linv"]), mk(c["r_side"][idx]), mk(c["rr"]), sets, out["x_u"], z=out.get("z"), lmb=out.get("lmb"),
                  logs=out.get("logs"), iters=out.get("iters"), **par)
    return {k: _host(v) for k, v in out.items()}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def hip():
    from dual import hip_kernels
    return hip_kernels()


def _rel(a, ref):
    """largest difference relative to the largest entry of the reference (NaN = not written, on both sides)"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.shape != ref.shape or not np.array_equal(np.isnan(a), np.isnan(ref)):
        return np.inf
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(a[ok] - ref[ok])) / np.max(np.abs(ref[ok])))


def _rel_logs(a, ref):
    """the residual logs entry by entry, each relative to itself, as test_config5_sls_admm_kernels compares them in fp64"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.shape != ref.shape or not np.array_equal(np.isnan(a), np.isnan(ref)):
        return np.inf
    ok = ~np.isnan(ref)
    return float(np.max(np.abs(a[ok] - ref[ok]) / np.maximum(1e-6, np.abs(ref[ok]))))


# ---- 1. the instantiation grid against the C oracle ----------------------------------------------------------------------
# (R, D, sets, operands): every D meets every BLOCK; every kind appears with R > 256; 320 x 3 has ISLS_MAX_SETS sets; 257 x 4 has the
# two largest parameter blocks (MULTILINEAR q = dim = 5: 36 words, SQUARE q = dim = 5: 58 = kSetParMax); 1 x 1 has a single set
GRID = [
    (1, 1, (BOX,), "shared"),                                                            # BLOCK 256
    (63, 2, (SOC, LINEAR), "per"),
    (64, 4, (QUAD, BOX), "shared"),
    (65, 1, (LINEAR, BOX), "per"),
    (256, 3, (SHELL, SOC), "shared"),
    (257, 4, ((MLIN, dict(dim=5, q=5)), (SQUARE, dict(dim=5, q=5))), "per"),             # BLOCK 512
    (257, 1, (QUAD, LINEAR), "shared"),
    (320, 3, (BOX, SOC, LINEAR, SHELL), "per"),
    (512, 2, (QUAD, (MLIN, dict(q=1))), "shared"),
    (513, 2, (SQUARE, SHELL), "per"),                                                    # BLOCK 1024
    (513, 3, (LINEAR, QUAD, SOC), "shared"),
    (1000, 1, (BOX, SOC), "per"),
    (1024, 4, ((MLIN, dict(q=2)), BOX, (SQUARE, dict(q=2))), "shared"),
]
GRID_IDS = [f"R{R}-D{D}-{how}" for R, D, _, how in GRID]
FIELDS = ("x_u", "z", "lmb")
_REF = {}


def _grid_ref(oracle, i, dtype):
    """the oracle's outputs of grid case i, computed once per precision and read by every test that needs them"""
    if (i, dtype) not in _REF:
        R, D, kinds, how = GRID[i]
        out = _solve(oracle, _case(R, D, kinds), how, dtype)
        for v in out.values():
            v.setflags(write=False)
        _REF[(i, dtype)] = out
    return _REF[(i, dtype)]


def test_grid_covers_every_instantiation():
    """the table of the grid itself: D x BLOCK complete, every kind with R > 256, the set counts and the operand forms"""
    assert {R for R, *_ in GRID} == {1, 63, 64, 65, 256, 257, 320, 512, 513, 1000, 1024}
    assert {(D, _block(R)) for R, D, *_ in GRID} == {(D, B) for D in (1, 2, 3, 4) for B in (256, 512, 1024)}
    kind_of = lambda k: k if isinstance(k, int) else k[0]                                # noqa: E731
    assert {kind_of(k) for R, _, kinds, _ in GRID if R > 256 for k in kinds} == {BOX, SOC, SQUARE, LINEAR, QUAD, SHELL, MLIN}
    assert {len(kinds) for _, _, kinds, _ in GRID} >= {1, capi.MAX_SETS}
    hows = [how for *_, how in GRID]
    assert abs(hows.count("per") - hows.count("shared")) <= 1
    big = _case(*GRID[5][:3])["sets"]
    assert big[0]["par"].shape[1] == 1 + 2 * 5 + 5 * 5 and big[1]["par"].shape[1] == 3 + 5 + 2 * 5 * 5


@pytest.mark.parametrize("i", range(len(GRID)), ids=GRID_IDS)
def test_grid_fp64_against_oracle(oracle, hip, i):
    """fp64 HIP against the fp64 oracle: iters equal, x_u / z / lmb relative to their largest entry at 1e-9 and the logs entry
    by entry at 1e-6 (the bounds of test_config5_sls_admm_kernels).  The constraints bite: max|z - x_u| / max|x_u| > 1e-2 in the
    oracle's output (measured on the CPU: 0.054 .. 1.9 over the grid)."""
    R, D, kinds, how = GRID[i]
    ref = _grid_ref(oracle, i, np.float64)
    assert np.all(ref["iters"] == FIXED["max_iter"])
    bite = float(np.max(np.abs(ref["z"] - ref["x_u"])) / np.max(np.abs(ref["x_u"])))
    assert bite > 1e-2, bite
    got = _solve(hip, _case(R, D, kinds), how, np.float64, wrap=_dev)
    err = {k: _rel(got[k], ref[k]) for k in FIELDS}
    err["logs"] = _rel_logs(got["logs"], ref["logs"])
    print(f"grid fp64 {GRID_IDS[i]} BLOCK {_block(R)}: bite {bite:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.array_equal(got["iters"], ref["iters"])
    assert all(err[k] < 1e-9 for k in FIELDS) and err["logs"] < 1e-6, err


@pytest.mark.parametrize("i", range(len(GRID)), ids=GRID_IDS)
def test_grid_fp32_against_oracle(oracle, hip, i):
    """fp32 HIP against the fp32 oracle at the project's 1e-4 on x_u, z, lmb and the logs, each relative to its largest entry (in
    fp32 a residual that has fallen far below the first one is a difference of nearly equal numbers: its error scales with the
    iterates, not with itself, so the logs are taken like the other arrays here and entry by entry only in fp64).  Condition on
    the inputs, asserted here on the CPU: the fp32 oracle follows the fp64 oracle to 2e-5 on the same quantities, i.e. no case
    sits on a knife edge of the inner stall rule or of a non-convex primitive.  Measured over the grid: x_u 2.2e-7 .. 1.7e-6,
    z 1.7e-7 .. 1.4e-6, lmb 5.2e-8 .. 5.6e-7, logs 1.4e-7 .. 7.9e-7."""
    R, D, kinds, how = GRID[i]
    r64, r32 = _grid_ref(oracle, i, np.float64), _grid_ref(oracle, i, np.float32)
    cond = {k: _rel(r32[k], r64[k]) for k in FIELDS}
    cond["logs"] = _rel(r32["logs"], r64["logs"])
    print(f"grid fp32 {GRID_IDS[i]}: oracle fp32 vs fp64 " + " ".join(f"{k} {v:.2e}" for k, v in cond.items()))
    assert np.array_equal(r32["iters"], r64["iters"]) and all(v < 2e-5 for v in cond.values()), cond
    got = _solve(hip, _case(R, D, kinds), how, np.float32, wrap=_dev)
    err = {k: _rel(got[k], r32[k]) for k in FIELDS}
    err["logs"] = _rel(got["logs"], r32["logs"])
    print(f"grid fp32 {GRID_IDS[i]} BLOCK {_block(R)}: HIP vs oracle " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.array_equal(got["iters"], r32["iters"])
    assert all(v < 1e-4 for v in err.values()), err


# ---- 2. against a plain numpy loop -----------------------------------------------------------------------------------------
# one shape per BLOCK; all kinds between them (the multilinear slab only at 65 rows: its numpy form is a Python loop over rows)
LOOP = [(65, 3, (BOX, (MLIN, dict(q=2)), SOC)), (320, 2, (SQUARE, LINEAR, QUAD)), (513, 4, (SHELL, SOC, BOX))]
LOOP_IDS = [f"R{R}-D{D}" for R, D, _ in LOOP]
LOOP_P = 3
_LOOP_REF = {}


def _numpy_admm(c, max_iter, inner_max_iter, rho, alpha, threshold, **_):
    """ADMM_SLS restated: x = Linv (r_side + rr (z - lmb)); z+ = project(alpha x + (1 - alpha) z + lmb) with the numpy
    project_set_convex of isls/projections.py over all rows of a problem; lmb += x - z+; residuals weighted by rr (sls.py)."""
    pj = importlib.import_module("isls.projections")
    P, R, D = c["P"], c["R"], c["D"]
    x_u, zs, logs = np.zeros((P, R, D)), np.zeros((P, R, D)), np.zeros((P, max_iter, 2))
    w = c["rr"][:, None]
    for p in range(P):
        sets = [{k: (v[p] if isinstance(v, np.ndarray) else v) for k, v in st.items()} for st in c["sets"]]
        project = pj.ConvexSets(D, (0, D), sets, rho=rho, max_iter=inner_max_iter, threshold=threshold)
        z, lmb = np.zeros((R, D)), np.zeros((R, D))
        for j in range(max_iter):
            x = c["Linv"] @ (c["r_side"][p] + w * (z - lmb))
            zn = project((alpha * x + (1 - alpha) * z + lmb).ravel()).reshape(R, D)
            logs[p, j] = np.linalg.norm(w * (x - zn)), np.linalg.norm(w * (zn - z))
            lmb += x - zn
            z = zn
        x_u[p], zs[p] = x, z
    return dict(x_u=x_u, z=zs, logs=logs)


def _loop_ref(j):
    if j not in _LOOP_REF:
        R, D, kinds = LOOP[j]
        _LOOP_REF[j] = _numpy_admm(_case(R, D, kinds, P=LOOP_P, seed=2), **FIXED)
    return _LOOP_REF[j]


def _loop_err(out, ref):
    return dict(x_u=_rel(out["x_u"], ref["x_u"]), z=_rel(out["z"], ref["z"]), logs=_rel_logs(out["logs"], ref["logs"]))


def _numpy_gap(oracle):
    """the fp64 oracle against the numpy loop, per quantity the worst of the three shapes: both on the CPU, computed once"""
    if "gap" not in _LOOP_REF:
        gaps = [_loop_err(_solve(oracle, _case(R, D, kinds, P=LOOP_P, seed=2), "per", np.float64), _loop_ref(j))
                for j, (R, D, kinds) in enumerate(LOOP)]
        # not below 8 eps: a BLAS that happens to sum as the oracle does would leave no room for one rounding per operation
        _LOOP_REF["gap"] = {k: max(8 * np.finfo(np.float64).eps, *(g[k] for g in gaps)) for k in gaps[0]}
    return _LOOP_REF["gap"]


@pytest.mark.parametrize("j", range(len(LOOP)), ids=LOOP_IDS)
def test_fp64_against_numpy_loop(oracle, hip, j):
    """HIP fp64 x_u, z (relative to the largest entry) and logs (entry by entry) against the numpy loop, which shares no code with
    the oracle.  Bound: ten times the gap between the fp64 oracle and the numpy loop, both on the CPU, the worst of the three
    shapes per quantity and not below 8 eps = 1.8e-15 -- measured: x_u 1.6e-15, z 1.4e-15, logs 6.2e-15, i.e. bounds of 1.8e-14,
    1.8e-14 and 6.2e-14.  The
    test measures the gap again where it runs (another BLAS sums in another order) and refuses a gap above 1e-13, which would
    mean that the two references have come apart.  The margin of ten is for the summation order of the device's block_sum
    and the fused multiply-adds of its x-step."""
    R, D, kinds = LOOP[j]
    c, ref, gap = _case(R, D, kinds, P=LOOP_P, seed=2), _loop_ref(j), _numpy_gap(oracle)
    assert all(v < 1e-13 for v in gap.values()), gap
    got = _solve(hip, c, "per", np.float64, wrap=_dev)
    err = _loop_err(got, ref)
    print(f"numpy loop {LOOP_IDS[j]} BLOCK {_block(R)}: oracle-numpy gap " + " ".join(f"{k} {v:.2e}" for k, v in gap.items()) +
          " | HIP " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert np.all(got["iters"] == FIXED["max_iter"])
    assert all(err[k] <= 10 * gap[k] for k in err), (err, gap)


# ---- 3. the stop rules at the large blocks ---------------------------------------------------------------------------------
# r_side of problem b is scaled by STOP_SCALE[b]; of these eight problems each case runs the three whose every stop decision
# is clear.  (The residuals of this iteration fall by a factor 1.5 .. 2 per iteration after the first, so a residual that is a
# factor 2 above tol at one iteration and a factor 2 below it at the next exists only at the first two iterations: the later
# stops are decided by the relative-change rule, where a stalling residual makes the change drop by more than a factor 4.)
STOP_SCALE = (3, 2, 1, 0.5, 0.3, 0.1, 0.03, 0.01)
STOP = [  # R, D, sets, seed, problems, parameters, expected iters
    (320, 3, (SOC,), 3, (0, 1, 7), dict(max_iter=9, alpha=1.0, inner_max_iter=9, tol=0.631, rel_tol=0.05), (3, 9, 1)),
    (1024, 2, (SHELL, SOC), 4, (1, 5, 7), dict(max_iter=9, alpha=1.5, inner_max_iter=4, tol=2.512, rel_tol=0.08), (6, 2, 1)),
]


def _stop_decisions(lg, tol, rel_tol):
    """Replay of the two stop rules on one problem's log -> (iterations run, rule that stopped it: 1 residuals below tol,
    2 relative changes below rel_tol, 0 neither, smallest factor between a deciding quantity and its threshold over every
    decision taken: the larger residual against tol, the larger relative change against rel_tol)."""
    prev, clear = np.array([1e6, 1e6]), np.inf
    for j in range(len(lg)):
        m1 = float(np.max(lg[j])) / tol
        clear = min(clear, max(m1, 1.0 / m1))
        if m1 < 1:
            return j + 1, 1, clear
        m2 = float(np.max(np.abs(prev - lg[j]) / (prev + 1e-30))) / rel_tol
        clear = min(clear, max(m2, 1.0 / m2))
        if m2 < 1:
            return j + 1, 2, clear
        prev = lg[j]
    return len(lg), 0, clear


@pytest.mark.parametrize("k", range(len(STOP)), ids=[f"R{s[0]}-D{s[1]}" for s in STOP])
def test_stop_rules_at_the_large_blocks(oracle, hip, k):
    """fp64, BLOCK 512 and 1024: with tol and rel_tol set the problems of a launch stop at different outer iterations (one by the
    residual rule at the first or second iteration, one by the relative-change rule, one in between or never); iters equals the
    oracle's and the log rows behind a problem's stop keep their NaN fill.  Condition on the inputs, asserted on the CPU from the
    oracle's log with both rules off: at EVERY iteration up to a problem's stop -- the stop and the one before it among them --
    the larger residual and the larger relative change are at least a factor 2 from tol and rel_tol (measured: 3.8, 4.1, 4.1 at
    R = 320 and 2.9, 2.4, 7.7 at R = 1024), so the stop iteration does not hang on rounding."""
    R, D, kinds, seed, sel, par, expect = STOP[k]
    c = _case(R, D, kinds, P=len(STOP_SCALE), seed=seed, scale=STOP_SCALE)
    free = _solve(oracle, c, "per", np.float64, sel=sel, **dict(par, tol=0.0, rel_tol=0.0))
    dec = [_stop_decisions(free["logs"][b], par["tol"], par["rel_tol"]) for b in range(len(sel))]
    print(f"stop rules R {R}: (iters, rule, clearance) {dec}")
    assert tuple(d[0] for d in dec) == expect and {d[1] for d in dec} >= {1, 2} and all(d[2] >= 2.0 for d in dec), dec
    ref = _solve(oracle, c, "per", np.float64, sel=sel, **par)
    assert tuple(ref["iters"]) == expect
    got = _solve(hip, c, "per", np.float64, wrap=_dev, sel=sel, **par)
    assert np.array_equal(got["iters"], ref["iters"])
    for b, it in enumerate(expect):
        assert np.all(np.isfinite(got["logs"][b, :it])) and np.all(np.isnan(got["logs"][b, it:])), (b, got["logs"][b])
    assert _rel_logs(got["logs"], ref["logs"]) < 1e-6 and all(_rel(got[f], ref[f]) < 1e-9 for f in FIELDS)


# ---- 4. invariants of a launch: bit equality, both precisions, one shape per BLOCK -------------------------------------------
INV = [(65, 3, (BOX, SOC)), (320, 2, (SQUARE, LINEAR, QUAD)), (513, 4, (SHELL, (MLIN, dict(q=2)), BOX))]
INV_IDS = [f"R{R}-D{D}" for R, D, _ in INV]
both = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
shapes = pytest.mark.parametrize("j", range(len(INV)), ids=INV_IDS)
OUT = ("x_u", "z", "lmb", "logs", "iters")


def _same(a, b, keys=OUT):
    return all(np.array_equal(a[k], b[k], equal_nan=k == "logs") for k in keys)


@both
@shapes
def test_a_problem_alone_equals_the_problem_in_the_batch(hip, j, dtype):
    """one workgroup per problem: nothing of a problem depends on its place in the launch or on the other problems"""
    c = _case(*INV[j], seed=4)
    full = _solve(hip, c, "per", dtype, wrap=_dev)
    assert np.all(np.isfinite(full["x_u"])) and np.all(full["iters"] == FIXED["max_iter"])
    for b in (0, c["P"] - 1):
        alone = _solve(hip, c, "per", dtype, wrap=_dev, sel=[b])
        assert _same(alone, {k: v[b:b + 1] for k, v in full.items()}), b


@both
@shapes
def test_null_outputs_leave_x_u_unchanged(hip, j, dtype):
    """z, lmb, logs and iters are optional: without them the same x_u, bit for bit"""
    c = _case(*INV[j], seed=4)
    full, bare = _solve(hip, c, "per", dtype, wrap=_dev), _solve(hip, c, "per", dtype, wrap=_dev, outputs=False)
    assert set(bare) == {"x_u"} and np.all(np.isfinite(bare["x_u"])) and np.array_equal(bare["x_u"], full["x_u"])


@both
@shapes
def test_shared_operands_equal_tiled_operands(hip, j, dtype):
    """set operands with problem stride 0 against the same operands repeated to [P, ...]"""
    c = _case(*INV[j], seed=4)
    shared, tiled = _solve(hip, c, "shared", dtype, wrap=_dev), _solve(hip, c, "tiled", dtype, wrap=_dev)
    assert np.all(np.isfinite(shared["x_u"])) and _same(shared, tiled)
    assert not np.array_equal(shared["x_u"], _solve(hip, c, "per", dtype, wrap=_dev)["x_u"])     # the operands do matter


@both
def test_empty_batch_touches_nothing(hip, dtype):
    """P = 0 with every pointer set: ISLS_OK and no word of the output buffers written.  (An empty tensor has a null data
    pointer, which the entry point refuses: the argument block is built for two problems and P is set to 0 afterwards.)"""
    import torch
    c = _case(*INV[0], seed=4)
    R, D = c["R"], c["D"]
    buf = {k: _dev(np.full((2, R, D), np.nan, dtype=dtype)) for k in ("x_u", "z", "lmb")}
    logs, iters = _dev(np.full((2, FIXED["max_iter"], 2), np.nan, dtype=dtype)), _dev(np.full(2, -7, dtype=np.int32))
    mk = lambda a: _dev(np.ascontiguousarray(a, dtype=dtype))                            # noqa: E731
    sets = [{k: (mk(v) if isinstance(v, np.ndarray) else v) for k, v in st.items()} for st in _operands(c["sets"], "shared")]
    operands = (mk(c["Linv"]), mk(c["r_side"][:2]), mk(c["rr"]))
    a = capi.Kernels.sls_admm_args(*operands, sets, buf["x_u"], z=buf["z"], lmb=buf["lmb"], logs=logs, iters=iters, **FIXED)
    assert a.P == 2 and a.x_u and a.r_side
    a.P = 0
    assert hip._call("sls_admm", "f64" if dtype == np.float64 else "f32", a, None) == capi.OK
    torch.cuda.synchronize()
    assert all(np.all(np.isnan(_host(v))) for v in buf.values())
    assert np.all(np.isnan(_host(logs))) and np.all(_host(iters) == -7)


# ---- 5. isls_sls_closed_loop -------------------------------------------------------------------------------------------------
def _loop_inputs(M, N, n, m):
    rng = np.random.default_rng(100 * M + 10 * N + n)
    A = rng.standard_normal((n, n))
    A *= 0.9 / np.max(np.abs(np.linalg.eigvals(A)))            # contractive: spectral radius 0.9
    B = 0.5 * rng.standard_normal((n, m))
    K = 0.1 * rng.standard_normal((N * m, N * n))
    for i in range(N):
        K[i * m:(i + 1) * m, (i + 1) * n:] = 0.0              # causal: u_i sees x_0 .. x_i
    return A, B, K, 0.3 * rng.standard_normal(N * m), rng.standard_normal((M, n))


def _closed_loop(A, B, K, k, x0, dtype):
    """u_i = K_i x_{0:i} + k_i, x_{i+1} = A x_i + B u_i in numpy at `dtype`"""
    A, B, K, k, x0 = (np.asarray(a, dtype=dtype) for a in (A, B, K, k, x0))
    M, n, m = x0.shape[0], A.shape[0], B.shape[1]
    N = k.size // m
    x, u = np.zeros((M, N, n), dtype=dtype), np.zeros((M, N, m), dtype=dtype)
    x[:, 0] = x0
    for i in range(N):
        u[:, i] = x[:, :i + 1].reshape(M, -1) @ K[i * m:(i + 1) * m, :(i + 1) * n].T + k[i * m:(i + 1) * m]
        if i + 1 < N:
            x[:, i + 1] = x[:, i] @ A.T + u[:, i] @ B.T
    return x, u


@pytest.mark.parametrize("N", [1, 2, 7])
@pytest.mark.parametrize("nm", [(1, 1), (3, 2), (5, 3)], ids=lambda v: f"n{v[0]}m{v[1]}")
@pytest.mark.parametrize("M", [1, 64, 65, 130])
def test_closed_loop_against_numpy(hip, M, nm, N):
    """isls_sls_closed_loop at one thread, a full 64-thread block, one thread past it and three blocks, against a numpy fp64
    loop: fp64 at the project's 1e-10, fp32 at its 1e-4, relative to max(1, largest entry).  Condition on the inputs, asserted
    on the CPU: the same loop in numpy float32 stays within 1e-5 of the float64 one (measured: 2.4e-7 at most over the 36 cases).
    Every output starts as NaN: the last control is written, and with N = 1 only x_0 and u_0 are -- the words behind them stay."""
    import torch
    n, m = nm
    A, B, K, k, x0 = _loop_inputs(M, N, n, m)
    xr, ur = _closed_loop(A, B, K, k, x0, np.float64)
    x32, u32 = _closed_loop(A, B, K, k, x0, np.float32)
    rel = lambda a, r: float(np.max(np.abs(a.astype(np.float64) - r)) / max(1.0, np.max(np.abs(r))))   # noqa: E731
    cond = max(rel(x32, xr), rel(u32, ur))
    assert cond < 1e-5, cond
    for dtype, tol in ((np.float64, 1e-10), (np.float32, 1e-4)):
        guard = 7
        xb = torch.full((M * N * n + guard,), float("nan"), dtype=torch.from_numpy(np.zeros(1, dtype=dtype)).dtype, device="cuda")
        ub = torch.full_like(xb[:M * N * m + guard], float("nan"))
        xl, ul = xb[:M * N * n].view(M, N, n), ub[:M * N * m].view(M, N, m)
        hip.sls_closed_loop(*(_dev(a.astype(dtype)) for a in (A, B, K, k, x0)), xl, ul)
        xh, uh = _host(xl), _host(ul)
        assert np.all(np.isfinite(xh)) and np.all(np.isfinite(uh[:, N - 1]))           # the last control is written
        assert np.all(np.isnan(_host(xb[M * N * n:]))) and np.all(np.isnan(_host(ub[M * N * m:])))
        err = max(rel(xh, xr), rel(uh, ur))
        print(f"closed loop M {M} n {n} m {m} N {N} {np.dtype(dtype).name}: {err:.2e} (numpy fp32 vs fp64 {cond:.2e})")
        assert err < tol, err
        if N == 1:
            assert np.array_equal(xh[:, 0], x0.astype(dtype))
