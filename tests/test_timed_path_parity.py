"""The benchmarked path against the oracle at the size bench.py measures.

bench.py times `Engine.run_outer` + `Engine.advance` at B = 4096, N = 100, J = 5, L = 20 in fp64.  At that size the engine
takes forms no small-batch test reaches: sequential feed-forward passes on the double integrator's structure (lean records),
the first feed-forward pass inside the gain pass only while the gain pass's wavefronts fit the chip's SIMDs, and the
convergence reduction in its 1024-thread, several-trip form.  Here the same calls run next to the oracle's own driver
(`oracle_ilqr_admm_outer` + `oracle_outer_advance`) from the same nominal, and the state is compared after EVERY outer
iteration: per trajectory (helpers.compare_batched) at 1e-10 in fp64, the integer state (line-search winner, status,
activity flags, ADMM iteration counts) exactly.  The oracle runs on OMP_NUM_THREADS threads.

Line-search ties.  Once a trajectory's iLQR step has all but vanished (the double integrator is linear, so one outer
iteration solves its LQ subproblem), the L candidate costs can agree to the last few bits and the winner is decided by
rounding.  A trajectory that differs is left out only with proof from the oracle side (line_search_ties): its outer
iteration replayed kernel by kernel on the oracle (the replay must reproduce the driver's winner and x-step bit for bit)
shows a rollout whose best candidates lie within TIE_REL (1e-14) of each other, the device's final winner among them.  Such
trajectories are printed, counted, capped at TIE_CAP (0.5 %) of the batch and left out of that comparison and the later ones
only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import isls_problems as P
from helpers import ALPHAS, OracleDriver, compare_batched, compare_exact, problem_arrays
from isls import _capi as capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_HEAD, N, J, L = 4096, 100, 5, 20                  # bench.py's defaults
TOL = 1e-10
# candidate costs this close (relative) are a tie.  Measured at seed 0 (B = 4096 ... 8192, fp64): every trajectory whose winner
# or x-step differs has two candidates within 1.0e-15 of each other, all from outer iteration 2 on (iteration 1 agrees to
# 7.5e-13 everywhere); 0.18-0.32 % of the batch over three iterations.
TIE_REL = 1e-14
TIE_CAP = 5e-3                                      # at most 0.5 % of the batch may be exempted as ties
FLOATS = ("xhat", "uhat", "cost", "K", "k", "xx", "xu", "zu", "lu", "res", "cost_hist")
INTS = ("best", "status", "outer_active", "admm_active", "iters", "hist_len")
ENGINE_NAME = {"iters": "admm_iters"}


class TimedStepOracle:
    """bench.py's step() on the oracle: `oracle_ilqr_admm_outer` (the first call makes the ADMM restart itself, as
    Engine.begin_outer() does before bench.py's first step), then `oracle_outer_advance` (accept without stop rule, ADMM
    restart, linearisation and expansion about the new nominal).  The initial nominal is bench.py's: x0 repeated, u0."""

    def __init__(self, kern, cfg, B, dtype=np.float64):
        self.kern, self.sfx = kern, "f64" if dtype == np.float64 else "f32"
        pa = problem_arrays(cfg, range(B), dtype=dtype)
        assert np.array_equal(pa["xhat"], np.repeat(cfg["x0"][:B, None, :], cfg["N"], axis=1).astype(dtype))
        assert np.array_equal(pa["uhat"], cfg["u0"][:B].astype(dtype))
        o = self.o = OracleDriver(kern, pa, rho_u=cfg["rho_u"], relax=cfg["relax"], dtype=dtype)
        o.cost_hist = np.zeros((B, 8), dtype=dtype)        # Engine.set_nominal: cost_log = [initial cost]
        o.cost_hist[:, 0] = o.cost
        o.hist_len = np.ones(B, dtype=np.int32)
        o.linearize_expand()
        K = capi.Kernels
        self.alphas = ALPHAS[:L].astype(dtype)
        self.args = (
            K.gain_args(o.A, o.Bm, o.Cxx, o.Cuu, o.K, o.Quu, o.fac, o.Qux, status=o.status, active=o.admm_active),
            K.ff_args(o.A, o.Bm, o.c0x, o.c0u, o.K, o.Quu, o.fac, o.Qux, o.k, Rr=o.Rr, xhat=o.xhat, uhat=o.uhat, zu=o.zu, lu=o.lu,
                      active=o.admm_active),
            K.rollout_args(pa["model"], pa["model_par"], o.K, o.k, o.xhat, o.uhat, self.alphas, pa["Qtab"], pa["ztab"], pa["seq"],
                           pa["u_std"], o.xx, o.xu, best=o.best, cost_new=o.cost_new, wr=o.wr, zu=o.zu, lu=o.lu, cost_cur=o.cost,
                           status=o.status, active=o.admm_active),
            K.admm_args(o.xx, o.xu, o.res, zu=o.zu, lu=o.lu, u_lo=pa["u_lo"], u_hi=pa["u_hi"], relax=o.relax, tol_abs=0.0,
                        tol_rel=0.0, res_prev=o.res_prev, active=o.admm_active, iters=o.iters))
        acc = K.accept_args(o.xx, o.xu, o.cost_new, o.xhat, o.uhat, o.cost, cost_hist=o.cost_hist, hist_len=o.hist_len,
                            tol_cost=-1.0, tol_osc=-1.0, outer_active=o.outer_active)
        lin = K.linearize_args(pa["model"], pa["model_par"], o.xhat, o.uhat, o.A, o.Bm)
        exp = K.expand_args(pa["Qtab"], pa["ztab"], pa["seq"], pa["u_std"], o.c0x, o.c0u, xhat=o.xhat, uhat=o.uhat, Rr=o.Rr)
        self.adv = K.advance_args(acc, lin, exp, admm_active=o.admm_active, iters=o.iters, lu=o.lu, res_prev=o.res_prev)
        self.steps = 0
        self.history = [self.state()]                     # the state before the first step, then after each step

    def step(self):
        self.kern.outer(*self.args, J, self.sfx, outer_active=self.o.outer_active, begin_done=self.steps > 0)
        self.kern.outer_advance(self.adv, self.sfx)
        self.steps += 1
        self.history.append(self.state())

    def state(self):
        return {name: getattr(self.o, name).copy() for name in FLOATS + INTS}


def bench_engine(cfg, B, dtype="f64", structured=True):
    """An Engine set up as bench.py sets up its timed region (the double integrator recognised from the dense pair, shared
    cost tables, box on u, tolerances 0, begin_done), with the linearisation, expansion and ADMM restart of the first step
    made."""
    import torch
    from isls import models
    from isls.engine import Engine
    eng = Engine(B, cfg["N"], cfg["n"], cfg["m"], dtype=torch.float64 if dtype == "f64" else torch.float32, device="cuda")
    mdl = models.LTI(cfg["A"], cfg["B"])
    eng.set_model(mdl.model_id, mdl.params())
    eng.set_quadratic_cost(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    eng.set_nominal(np.repeat(cfg["x0"][:, None, :], cfg["N"], axis=1), cfg["u0"])
    eng.set_admm(rho_u=cfg["rho_u"], u_box=(cfg["u_lo"], cfg["u_hi"]), relax=cfg["relax"])
    if not structured:
        eng.use_model_structure = False                 # bench.py --full's general_ab leg
    eng.build_outer(L, J, tol_abs=0.0, tol_rel=0.0, begin_done=True)
    eng.linearize()
    eng.expand()
    eng.begin_outer()
    return eng


def engine_state(eng):
    return {name: getattr(eng, ENGINE_NAME.get(name, name)).cpu().numpy() for name in FLOATS + INTS}


def line_search_ties(kern, cfg, history, sel, dev_best=None):
    """Oracle-side proof of line-search ties for the trajectories `sel`: every outer iteration of `history` (oracle states,
    before and after each) is replayed for them with the oracle's single kernels (linearise + expand, gain, J x [ff, rollout
    with the candidate costs cost_all, ADMM update]); the replay must give the driver's winner and x-step bit for bit.  A
    trajectory is proven when some rollout had two candidates within TIE_REL (relative) of the minimum and, with `dev_best`,
    the device's final winner is one of the minimal candidates of the last rollout.  Returns the mask over `sel`."""
    sel = np.asarray(sel)
    proven = np.zeros(len(sel), dtype=bool)
    gap = np.full(len(sel), np.inf)                       # smallest relative gap between the two best candidates seen
    rows = np.arange(len(sel))
    for i in range(len(history) - 1):
        prev, after = history[i], history[i + 1]
        act = prev["outer_active"][sel].astype(np.int32)
        pa = problem_arrays(cfg, sel)
        pa["xhat"], pa["uhat"] = prev["xhat"][sel].copy(), prev["uhat"][sel].copy()
        d = OracleDriver(kern, pa, rho_u=cfg["rho_u"], relax=cfg["relax"])
        d.cost[:], d.zu[:], d.res_prev[:] = prev["cost"][sel], prev["zu"][sel], 1e6    # ADMM restart: lambda 0, z warm
        d.outer_active[:], d.admm_active[:] = act, act
        d.linearize_expand()
        d.gain()
        ca = np.zeros((len(sel), L))
        near = np.zeros(len(sel), dtype=bool)
        for _ in range(J):
            d.ff()
            d.rollout(L, cost_all=ca)
            d.update(0.0)
            lo = ca.min(axis=1, keepdims=True)
            within = np.abs(ca - lo) <= TIE_REL * np.abs(lo)
            near |= within.sum(axis=1) > 1
            two = np.sort(ca, axis=1)[:, :2]
            with np.errstate(invalid="ignore", divide="ignore"):
                gap = np.fmin(gap, (two[:, 1] - two[:, 0]) / np.abs(two[:, 0]))
        a = act == 1
        assert np.array_equal(d.best[a], after["best"][sel][a]) and np.array_equal(d.xx[a], after["xx"][sel][a]), \
            "the kernel-by-kernel replay does not reproduce the oracle driver"
        if dev_best is not None and i == len(history) - 2:
            near &= within[rows, dev_best]
        proven |= near & a
    if proven.any():
        print(f"    oracle: relative gap between the two best candidates of the proven ties: at most {gap[proven].max():.1e}")
    return proven


def compare_state(tag, got, ref, tol=TOL, ties=None, exempt=None):
    """Integer state exactly, every float array per trajectory at `tol`; returns (worst error, array it came from).
    ties(sel, dev_best) -> mask: the oracle's proof of line-search ties (line_search_ties) for the trajectories that differ;
    proven ones join `exempt` (a set, kept across calls) and are left out from here on, at most TIE_CAP of the batch."""
    exempt = set() if exempt is None else exempt
    for name in INTS:
        if name != "best":
            compare_exact(f"{tag}: {name}", got[name], ref[name])
    keep = tie_exemptions(tag, got, ref, FLOATS + ("best",), tol, ties, exempt)
    errs = {name: compare_batched(f"{tag}: {name}", got[name][keep], ref[name][keep], tol) for name in FLOATS}
    compare_exact(f"{tag}: best", got["best"][keep], ref["best"][keep])
    worst = max(errs, key=errs.get)
    return errs[worst], worst


def tie_exemptions(tag, got, ref, names, tol, ties, exempt):
    """Mask of the trajectories still compared: those in `exempt` and those of the differing ones (any of `names` above
    `tol` per trajectory, or another winner) that ties(sel, dev_best) proves are left out; `exempt` grows by the latter."""
    from helpers import batched_errors
    B = len(ref[names[0]])
    keep = np.ones(B, dtype=bool)
    keep[sorted(exempt)] = False
    if ties is not None:
        differs = np.zeros(B, dtype=bool)
        for name in names:
            differs |= (got[name] != ref[name]) if name == "best" else batched_errors(got[name], ref[name]) > tol
        sel = np.flatnonzero(differs & keep)
        if len(sel):
            dev_best = got["best"][sel] if "best" in got else None
            new = sel[ties(sel, dev_best)]
            exempt.update(int(b) for b in new)
            keep[new] = False
            print(f"{tag}: {len(sel)} trajectories differ, {len(new)} proven line-search ties; exempt from here on: {sorted(exempt)}")
            if "best" in got:
                print(f"    winners oracle/device: {list(zip(ref['best'][sel].tolist(), got['best'][sel].tolist()))}")
    assert len(exempt) <= TIE_CAP * B, f"{tag}: {len(exempt)} line-search ties exempted, more than {TIE_CAP:.1%} of {B}"
    return keep


class FeedForwardLaunches:
    """Counts the driver's feed-forward launches (isls_timing kind 1) of the outer iterations run while attached."""

    def __init__(self, eng):
        from isls.engine import library
        self.lib, self.eng = library(), eng
        self.h = self.lib.isls_timing_create()
        assert self.h
        self.lib.isls_timing_reset(self.h)
        eng._outer_args.timing = self.h

    def count(self, kind=1):
        cnt = ctypes.c_int(0)
        self.lib.isls_timing_read_ms(self.h, kind, ctypes.byref(cnt))
        return cnt.value

    def close(self):
        self.eng._outer_args.timing = None
        self.lib.isls_timing_destroy(self.h)


def fused_limit(cfg):
    """Largest batch whose gain pass runs the first feed-forward pass inside (capi.hip: one wavefront of the fused pass per
    SIMD, floor(64 / (n + m)) trajectories per wavefront)."""
    import torch
    simds = torch.cuda.get_device_properties(0).multi_processor_count * 4
    return (64 // (cfg["n"] + cfg["m"])) * simds


def assert_structured_sequential(eng):
    """(after a run_outer: the driver's block gets its model hint once A, B are the model's own linearisation)"""
    a = eng._outer_args
    assert a.gain.lin_on == 1 and a.ff.lin_on == 1, "the timed region's form: passes on the model's structure"
    assert eng._outer_seg is None and int(a.ff.seg.nseg) <= 1, "sequential feed-forward passes, no time-parallel segments"
    assert eng._outer_rec is not None


def run_and_compare(tag, eng, kern, cfg, iters, ff_per_iter=None, orc=None, history=None, check_form=None, tol=TOL):
    """`iters` outer iterations (run_outer + advance) on the device, compared after each with the oracle: `orc` (a
    TimedStepOracle) stepped alongside, or `history` (TimedStepOracle.history of an earlier identical run).  check_form(eng)
    runs after the first run_outer; ff_per_iter: the feed-forward launches each outer iteration must make."""
    import torch
    cnt = FeedForwardLaunches(eng) if ff_per_iter is not None else None
    worst, exempt = (0.0, ""), set()
    try:
        for it in range(iters):
            eng.run_outer()
            if it == 0 and check_form is not None:
                check_form(eng)
            eng.advance()
            torch.cuda.synchronize()
            if orc is not None:
                orc.step()
            hist = (orc.history if orc is not None else history)[:it + 2]
            ties = lambda sel, best, h=hist: line_search_ties(kern, cfg, h, sel, best)   # noqa: E731
            e = compare_state(f"{tag}, outer iteration {it + 1}", engine_state(eng), hist[-1], tol, ties=ties, exempt=exempt)
            print(f"{tag}: outer iteration {it + 1}: worst per-trajectory error {e[0]:.2e} ({e[1]})")
            worst = max(worst, e)
            if cnt is not None:
                ff, gain = cnt.count(1), cnt.count(0)
                assert ff == (it + 1) * ff_per_iter and gain == it + 1, \
                    f"{tag}: {ff} feed-forward and {gain} gain launches after {it + 1} iterations, expected {ff_per_iter} + 1 per iteration"
    finally:
        if cnt is not None:
            cnt.close()
    return worst


@pytest.fixture(scope="module")
def headline_oracle(oracle):
    """config 2 (seed 0) at bench.py's size on the oracle: its state before and after each of four outer iterations of bench.py's step."""
    cfg = P.config2(batch=B_HEAD, N=N, seed=0)
    orc = TimedStepOracle(oracle, cfg, B_HEAD)
    for _ in range(4):
        orc.step()
    return cfg, orc.history


def test_timed_path_at_headline_size(oracle, headline_oracle):
    """B = 4096 exactly as bench.py times it: structured sequential passes, the first feed-forward pass inside the gain pass
    (J - 1 feed-forward launches per outer iteration), three outer iterations against the oracle."""
    cfg, history = headline_oracle
    eng = bench_engine(cfg, B_HEAD)
    assert B_HEAD <= fused_limit(cfg)
    run_and_compare("B=4096 structured", eng, oracle, cfg, 3, ff_per_iter=J - 1, history=history,
                    check_form=assert_structured_sequential)


@pytest.mark.parametrize("where", ["fused_edge", "split_edge", "b8192"])
def test_fused_gain_feedforward_switch(oracle, where):
    """Either side of the batch size where the driver stops running the first feed-forward pass inside the gain pass
    (7 trajectories per wavefront x SIMDs: fused up to it, a feed-forward launch of its own above it), and B = 8192."""
    cfg0 = P.config2(batch=1, N=N, seed=0)
    lim = fused_limit(cfg0)
    B = {"fused_edge": lim, "split_edge": lim + 1, "b8192": 8192}[where]
    cfg = P.config2(batch=B, N=N, seed=0)
    eng = bench_engine(cfg, B)
    fused = B <= lim
    run_and_compare(f"B={B} ({'fused' if fused else 'separate'} first feed-forward pass)", eng, oracle, cfg, 3,
                    ff_per_iter=J - 1 if fused else J, orc=TimedStepOracle(oracle, cfg, B), check_form=assert_structured_sequential)


def test_general_layout_at_headline_size(oracle, headline_oracle):
    """B = 4096 in the general layout (bench.py --full's general_ab leg): dense records, A_t, B_t read per trajectory and
    rewritten by every advance."""
    cfg, history = headline_oracle
    eng = bench_engine(cfg, B_HEAD, structured=False)

    def general(e):
        a = e._outer_args
        assert a.gain.lin_on == 0 and a.ff.lin_on == 0 and e._outer_rec is not None and int(a.ff.seg.nseg) <= 1
    run_and_compare("B=4096 general layout", eng, oracle, cfg, 3, ff_per_iter=J - 1, history=history, check_form=general)


def test_fp32_at_headline_size(oracle, headline_oracle):
    """B = 4096 in fp32, one outer iteration.  The device's fp32 result is held to the fp64 oracle with a bound per trajectory
    and array of max(1e-4, 3 x the fp32 oracle's own per-trajectory distance from the fp64 oracle) -- the precision the
    problem leaves in fp32, as config 5 bounds its fp32 comparison.  The integer state equals the fp32 oracle's."""
    from helpers import batched_errors
    cfg, history = headline_oracle
    eng = bench_engine(cfg, B_HEAD, dtype="f32")
    orc = TimedStepOracle(oracle, cfg, B_HEAD, dtype=np.float32)
    orc.step()
    ref32, ref64 = orc.state(), history[1]
    eng.run_outer()
    assert_structured_sequential(eng)
    eng.advance()
    got = engine_state(eng)
    for name in INTS:
        if name != "best":
            compare_exact(f"fp32 {name}", got[name], ref32[name])
    # winners decided by fp32 rounding (near-equal candidates) are counted and capped; every trajectory, these included,
    # must still meet the bound below
    nb = int((got["best"] != ref32["best"]).sum())
    print(f"B=4096 fp32: {nb} line-search winners differ from the fp32 oracle's")
    assert nb <= TIE_CAP * B_HEAD
    worst = (0.0, "")
    for name in FLOATS:
        bound = np.maximum(1e-4, 3.0 * batched_errors(ref32[name], ref64[name]))
        err = batched_errors(got[name], ref64[name])
        b = int(np.argmax(err / bound))
        assert err[b] <= bound[b], f"fp32 {name}: trajectory {b}: {err[b]:.3e} > bound {bound[b]:.3e}"
        worst = max(worst, (float(err.max()), name))
        print(f"B=4096 fp32 {name}: worst per-trajectory error {err.max():.2e}, at most {np.max(err / bound):.2f} of its bound")
    print(f"B=4096 fp32: worst per-trajectory error {worst[0]:.2e} ({worst[1]})")


def test_class_surface_at_headline_size(oracle, monkeypatch):
    """iSLS.ilqr_admm(project_u=Box, max_iter=3, tol=0) at B = 4096 with no segment override picks the structured sequential
    form; its final nominal, gains, ADMM state and cost equal the oracle's three outer iterations of the same loop (linearise,
    expand, driver, accept with the stop rules |dcost| < 1e-3 / oscillation < 1e-3)."""
    from isls import Box
    from test_isls_api import make_isls
    monkeypatch.delenv("ISLS_FF_NSEG", raising=False)
    cfg = P.config2(batch=B_HEAD, N=N, seed=0)
    s = make_isls(cfg, range(B_HEAD))
    s.ilqr_admm(project_u=Box(cfg["u_lo"], cfg["u_hi"]), max_iter=3, max_line_search_iter=L, max_admm_iter=J, rho_u=cfg["rho_u"],
                alpha=cfg["relax"], tol=0.0)
    e = s.engine
    assert_structured_sequential(e)

    o = OracleDriver(oracle, problem_arrays(cfg, range(B_HEAD)), rho_u=cfg["rho_u"], relax=cfg["relax"])
    o.cost_hist = np.zeros((B_HEAD, 8))
    o.cost_hist[:, 0] = o.cost
    o.hist_len = np.ones(B_HEAD, dtype=np.int32)
    stop_rules = dict(cost_hist=o.cost_hist, hist_len=o.hist_len, tol_cost=1e-3, tol_osc=1e-3)
    snap = lambda: {name: getattr(o, name).copy() for name in FLOATS + INTS}   # noqa: E731
    history = [snap()]
    for _ in range(3):
        if not o.outer_active.any():
            break
        o.run_c(L, J, accept_kw=stop_rules)             # linearise + expand, driver (ADMM restart inside), accept
        history.append(snap())
    compare_exact("ilqr_admm outer_active", e.outer_active.cpu().numpy(), o.outer_active)
    compare_exact("ilqr_admm status", e.status.cpu().numpy(), o.status)
    names = ("xhat", "uhat", "K", "k", "zu", "lu", "cost")
    got = {name: getattr(e, name).cpu().numpy() for name in names + ("best",)}
    ref = history[-1]
    keep = tie_exemptions("ilqr_admm", got, ref, names + ("best",), TOL,
                          lambda sel, best: line_search_ties(oracle, cfg, history, sel, best), set())
    worst = max((compare_batched(f"ilqr_admm {name}", got[name][keep], ref[name][keep], TOL), name) for name in names)
    compare_exact("ilqr_admm best", got["best"][keep], ref["best"][keep])
    print(f"iSLS.ilqr_admm B=4096: worst per-trajectory error {worst[0]:.2e} ({worst[1]})")


def test_bench_dump_against_oracle(tmp_path, oracle, headline_oracle):
    """bench.py --steps 3 --warmup 1 --dump-outputs at its defaults (B = 4096, N = 100) as a child process: what the last of
    its four steps left equals the oracle's fourth outer iteration from bench.py's own initial nominal, per trajectory at 1e-10;
    its convergence table is the reduction of that state."""
    cfg, history = headline_oracle
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    ld = lambda name: np.load(out / f"{name}.npy")          # noqa: E731
    idx = ld("trajectory_index").astype(np.int64)
    assert len(idx) > 0 and np.array_equal(idx, np.unique(idx)) and idx[-1] < B_HEAD
    ref = history[4]                                                # after bench.py's warm-up step and three timed steps
    pairs = (("x", "xhat"), ("u", "uhat"), ("cost", "cost"), ("z_u", "zu"), ("admm_residuals", "res"))
    got = {key: ld(name) for name, key in pairs}
    sub = {key: ref[key][idx] for _, key in pairs}
    keep = tie_exemptions("bench", got, sub, tuple(sub), TOL,
                          lambda sel, best: line_search_ties(oracle, cfg, history, idx[sel]), set())
    worst = max((compare_batched(f"bench {name}", got[key][keep], sub[key][keep], TOL), name) for name, key in pairs)
    st = ld("status")
    assert np.array_equal(st, ref["status"][idx].astype(np.float64))
    table = ld("convergence_table")
    assert table.shape == (1, 5)
    red = np.zeros(5)
    oracle.reduce_convergence(ref["cost"], ref["res"], ref["outer_active"], ref["status"], red)
    assert abs(table[0, 0] - red[0]) <= 1e-12 * abs(red[0]), (table[0], red)
    assert table[0, 3] == red[3] and table[0, 4] == red[4], (table[0], red)
    if len(idx) == B_HEAD:                                          # the whole batch dumped: the maxima are its residuals'
        assert table[0, 1] == max(0.0, ld("admm_residuals")[:, 0].max()) and table[0, 2] == max(0.0, ld("admm_residuals")[:, 1].max())
    for j in (1, 2):
        assert abs(table[0, j] - red[j]) <= TOL * max(1.0, abs(red[j])), (table[0], red)
    print(f"bench.py --dump-outputs ({len(idx)} trajectories): worst per-trajectory error {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("B", [1, 255, 256, 257, 4095, 4096, 4097, 8192, 12289])
def test_reduce_convergence_against_oracle(oracle, B):
    """isls_reduce_convergence / _table (one workgroup: 256 threads up to B = 256, 1024 above, several trips above 4096)
    against the oracle's reduction with random activity and status masks: the cost sum to 1e-13 relative, the maxima and
    the counts exactly, the table's other rows zeroed."""
    import torch
    from dual import hip_kernels
    hip = hip_kernels()
    rng = np.random.default_rng(B)
    cost = rng.uniform(0.5, 2.0, B) * 10.0 ** rng.integers(-3, 4, B)
    res = np.abs(rng.standard_normal((B, 2))) * 10.0 ** rng.integers(-6, 1, (B, 1))
    res[rng.random(B) < 0.1] = 0.0
    for p_act, p_st in ((0.5, 0.1), (1.0, 0.0), (0.0, 1.0), (0.97, 0.003)):
        active = (rng.random(B) < p_act).astype(np.int32)
        status = np.where(rng.random(B) < p_st, rng.integers(1, 8, B), 0).astype(np.int32)
        ref = np.zeros(5)
        oracle.reduce_convergence(cost, res, active, status, ref)
        dev = [torch.from_numpy(a).cuda() for a in (cost, res, active, status)]

        def check(got, what):
            assert abs(got[0] - ref[0]) <= 1e-13 * abs(ref[0]), (what, got, ref)
            assert np.array_equal(got[1:], ref[1:]), (what, got, ref)
        out5 = torch.full((5,), float("nan"), dtype=torch.float64, device="cuda")
        hip.reduce_convergence(*dev, out5)
        torch.cuda.synchronize()
        check(out5.cpu().numpy(), "out5")
        for rank, world in ((0, 1), (0, 2), (1, 2), (2, 3), (7, 8), (5, 300)):
            table = torch.full((world, 5), 7.0, dtype=torch.float64, device="cuda")
            hip.reduce_convergence_table(*dev, table, rank)
            torch.cuda.synchronize()
            t = table.cpu().numpy()
            check(t[rank], f"table row {rank} of {world}")
            assert not np.delete(t, rank, axis=0).any(), f"rows other than {rank} of {world} not zeroed"
