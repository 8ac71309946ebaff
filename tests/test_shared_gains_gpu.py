"""One set of Riccati records for a batch that shares the inputs of the gain recursion.

On the double integrator with one parameter row, batch-shared Hessian tables and the sequential recursion, the outer driver
(csrc/capi.hip) keeps ONE set of lean records [K | fac] for the whole batch: the gain pass writes them from its first
wavefront only, the feed-forward passes and the line search read that table.  Nothing of the arithmetic changes, so every
result must equal, bit for bit, what the same engine computes with per-trajectory Hessians (`allow_shared_hessian = False`:
the driver then sees a batch stride on Cxx / Cuu and takes the per-trajectory path).

The reference engine cannot use `Engine.advance()` (it serves the shared tables only) and ends an outer iteration with the
single launches that make it up: accept_x_step, the ADMM restart, expand.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import isls_problems as P                                  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("xhat", "uhat", "cost", "zu", "lu", "res", "best", "status", "K", "k")
J, ITERS = 3, 2


def problem(d, B, N, seed=0):
    rng = np.random.default_rng(seed)
    n, m = 2 * d, d
    A, Bm = P.double_integrator_AB(d, 2, 0.01)
    x0 = np.zeros((B, n))
    x0[:, :d] = rng.uniform(-0.5, 0.5, size=(B, d))
    zs = np.zeros((B, 2, n))
    zs[:, 1, :d] = rng.uniform(0.5, 1.5, size=(B, d))
    seq = np.zeros(N, dtype=np.int32)
    seq[N - 1] = 1
    return dict(n=n, m=m, N=N, A=A, B=Bm, zs=zs, Qs=np.stack([np.zeros((n, n)), 1e3 * np.eye(n)]), seq=seq, u_std=1e-3,
                x0=x0, u0=np.zeros((B, N, m)))


def make_engine(cfg, B, L, dtype, shared, par_rows=False, caller_ab=False, dense=False, inactive=None, wrong_best=False):
    from isls import models
    from isls.engine import Engine
    eng = Engine(B, cfg["N"], cfg["n"], cfg["m"], dtype=dtype, device="cuda")
    eng.allow_shared_hessian = shared
    mdl = models.LTI(cfg["A"], cfg["B"])
    par = np.asarray(mdl.params())
    eng.set_model(mdl.model_id, np.tile(par, (B, 1)) if par_rows else par)
    eng.set_quadratic_cost(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    eng.set_nominal(np.repeat(cfg["x0"][:, None, :], cfg["N"], axis=1), cfg["u0"])
    eng.set_admm(rho_u=1e-2, u_box=(-3.0, 3.0), relax=1.0)
    if dense:
        eng.use_model_structure = False
    if inactive is not None:
        eng.outer_active.copy_(torch.as_tensor(1 - inactive, dtype=torch.int32))
        eng.K.fill_(7.0)                                   # what an untouched trajectory must still hold afterwards
        eng.k.fill_(-7.0)
    if wrong_best:
        eng.best.fill_(L - 1)                              # the search records the smallest step and replays the real winner
    eng.linearize()
    if caller_ab:
        eng.ab_from_caller()
    # small batches: the sequential recursion all the same (the engine's own plan cuts them into time-parallel segments)
    eng.build_outer(L, J, tol_abs=0.0, tol_rel=0.0, begin_done=True, ff_nseg=None if B >= 512 else 1)
    eng.expand()
    eng.begin_outer()
    return eng


def iterate(eng, iters=ITERS):
    for _ in range(iters):
        eng.run_outer()
        if eng.allow_shared_hessian and eng.B > 1:
            # a caller's A, B stay the caller's: advance() must not linearise the model over them (they would be the model's
            # own from then on, and the second iteration would rightly take the structured, shared form)
            eng.advance(linearize=eng._ab_src != "caller")
        else:                                              # Engine.advance() in its parts
            eng.accept_x_step()
            eng.begin_outer()
            eng.expand()
    torch.cuda.synchronize()
    return {name: getattr(eng, name).cpu().numpy() for name in NAMES}


def assert_same_bits(got, ref, tag):
    for name in NAMES:
        a, b = got[name], ref[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, name)
        same = a.view(np.uint8) == b.view(np.uint8)
        assert same.all(), f"{tag}: {name} differs in {np.count_nonzero(~same.reshape(a.shape[0], -1).all(1))} of {a.shape[0]} trajectories"


def run_pair(d, B, N, L, dtype, **kw):
    cfg = problem(d, B, N)
    eng = make_engine(cfg, B, L, dtype, True, **kw)
    got = iterate(eng)
    ref_eng = make_engine(cfg, B, L, dtype, False, **kw)
    ref = iterate(ref_eng)
    assert ref_eng.records_shared == (B == 1)              # a batch of one declares no batch stride at all: shared, trivially
    return eng, got, ref


# d = 3: 7 trajectories per gain wavefront, 3 per line-search wavefront at L = 20; d = 1: 21 per gain wavefront.
# N = 7 is shorter than two ring groups of the search (its tail path alone runs).  B = 512: the engine's own sequential plan.
SHAPES = [(3, 1, 7, 5), (3, 5, 23, 20), (3, 8, 7, 20), (3, 22, 23, 5), (3, 512, 23, 5), (3, 512, 7, 20),
          (1, 5, 23, 20), (1, 8, 23, 5), (1, 22, 7, 20), (1, 512, 7, 5)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d,B,N,L", SHAPES)
def test_shared_records_bit_exact(d, B, N, L, dtype):
    eng, got, ref = run_pair(d, B, N, L, dtype)
    assert eng.records_shared
    assert eng._outer_args.gain.lin_on != 0
    assert_same_bits(got, ref, f"d={d} B={B} N={N} L={L}")
    assert np.isfinite(got["cost"]).all() and (got["K"] != 0).any()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_dense_form_keeps_records_per_trajectory(dtype):
    eng, got, ref = run_pair(3, 8, 23, 5, dtype, dense=True)
    assert not eng.records_shared and eng._outer_args.gain.lin_on == 0
    assert_same_bits(got, ref, "dense form")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("d,B", [(3, 22), (1, 64)])
def test_first_wavefront_inactive(d, B, dtype):
    """No trajectory of the first gain wavefront (and a scattered third of the others) is active: the records are written all
    the same, on fresh engines whose record buffers hold zeros, and an inactive trajectory keeps what it had."""
    tpw = 64 // (3 * d)
    inactive = np.zeros(B, dtype=np.int32)
    inactive[:tpw] = 1
    inactive[tpw + 1::3] = 1
    eng, got, ref = run_pair(d, B, 23, 20, dtype, inactive=inactive)
    assert eng.records_shared
    assert_same_bits(got, ref, f"masked d={d}")
    off = inactive != 0
    assert (got["K"][off] == 7.0).all() and (got["k"][off] == -7.0).all()
    assert (got["K"][~off] != 7.0).any(axis=(1, 2, 3)).all()
    assert (got["xhat"][off] == np.repeat(problem(d, B, 23)["x0"][off][:, None, :], 23, axis=1).astype(got["xhat"].dtype)).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_mispredicted_winner_replays_shared_gains(dtype):
    eng, got, ref = run_pair(3, 22, 23, 20, dtype, wrong_best=True)
    assert eng.records_shared
    assert_same_bits(got, ref, "wrong prediction")
    assert (got["best"] != 19).any()


@pytest.mark.parametrize("kw", [dict(par_rows=True), dict(caller_ab=True)], ids=["par_rows", "caller_ab"])
def test_not_shared_when_inputs_are_per_trajectory(kw):
    eng, got, ref = run_pair(3, 22, 23, 5, torch.float64, **kw)
    assert not eng.records_shared
    assert_same_bits(got, ref, str(kw))


def test_feedforward_refuses_shared_records():
    from isls import _capi as capi
    cfg = problem(3, 22, 23)
    eng = make_engine(cfg, 22, 5, torch.float64, True)
    eng.run_outer()
    assert eng.records_shared
    with pytest.raises(capi.IslsError):
        eng.feedforward(rec=eng.ff_record())
    with pytest.raises(capi.IslsError):
        eng.rec_lin(eng.ff_record())
    eng.gain(rec=eng.ff_record())                           # a gain pass of its own writes a record per trajectory again
    assert not eng.records_shared
    eng.feedforward(rec=eng.ff_record())
    torch.cuda.synchronize()
