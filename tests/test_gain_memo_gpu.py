"""The gain memo of the outer driver (csrc/gain_memo.hip, include/isls_hip.h): the batch-shared table of Riccati records is kept
across outer iterations and its validity is decided on the device, from the CONTENT of the recursion's inputs.

The comparator is the path without the memo: the same engine on per-trajectory Hessian tables (`allow_shared_hessian = False`,
as tests/test_shared_gains_gpu.py selects it), whose driver sees a batch stride on Cxx / Cuu and keeps a record per trajectory.
Everything is compared bit for bit (K, k, the nominal, cost, z, lambda, best, the residuals, status), after every outer
iteration, and `isls_gain_memo_stats` tells which iterations the device found their inputs unchanged.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import isls_problems as P                                  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("xhat", "uhat", "cost", "zu", "lu", "res", "best", "status", "K", "k")
X_NAMES = ("zx", "lx")                                     # with a state box
N, L, J = 12, 4, 2
F64, F32 = torch.float64, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])


@pytest.fixture(autouse=True)
def fresh_memo():
    from isls import _capi as capi
    capi.gain_memo_clear()
    yield
    capi.gain_memo_clear()


def matches():
    from isls import _capi as capi
    return capi.gain_memo_stats()[1]


def problem(d, B, N=N, seed=0):
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


def build(eng, J=J):
    # the sequential recursion (the engine's own plan cuts small batches into time-parallel segments, which share no records)
    eng.build_outer(L, J, tol_abs=0.0, tol_rel=0.0, begin_done=True, ff_nseg=1)


def make_engine(cfg, B, dtype, shared, inactive=None, J=J, rho_u=1e-2, solve_mode=None, x_box=None):
    from isls import models
    from isls.engine import Engine
    eng = Engine(B, cfg["N"], cfg["n"], cfg["m"], dtype=dtype, device="cuda")
    eng.allow_shared_hessian = shared
    mdl = models.LTI(cfg["A"], cfg["B"])
    eng.set_model(mdl.model_id, np.asarray(mdl.params()))
    eng.set_quadratic_cost(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    eng.set_nominal(np.repeat(cfg["x0"][:, None, :], cfg["N"], axis=1), cfg["u0"])
    if solve_mode is not None:
        eng.solve_mode = solve_mode
    if x_box is None:
        eng.set_admm(rho_u=rho_u, u_box=(-3.0, 3.0), relax=1.0)
    else:                                                  # a state block as well: Qr rows and the xhat / zx / lx terms in the passes
        eng.set_admm(rho_x=5e-2, rho_u=rho_u, x_box=x_box, u_box=(-3.0, 3.0), relax=1.0)
    if inactive is not None:
        eng.outer_active.copy_(torch.as_tensor(1 - inactive, dtype=torch.int32))
        eng.K.fill_(7.0)
        eng.k.fill_(-7.0)
    eng.linearize()
    build(eng, J)
    eng.expand()
    eng.begin_outer()
    return eng


def finish(eng):
    """End of an outer iteration: Engine.advance() on the shared tables, its parts for the comparator."""
    if eng.allow_shared_hessian:
        eng.advance(linearize=eng._ab_src != "caller")
    else:
        eng.accept_x_step()
        eng.begin_outer()
        eng.expand()


def state(eng):
    torch.cuda.synchronize()
    names = NAMES + (X_NAMES if eng.zx is not None else ())
    return {name: getattr(eng, name).cpu().numpy() for name in names}


def assert_same_bits(eng, ref, tag):
    got, want = state(eng), state(ref)
    assert got.keys() == want.keys()
    for name in got:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, name)
        same = a.view(np.uint8) == b.view(np.uint8)
        assert same.all(), f"{tag}: {name} differs in {np.count_nonzero(~same.reshape(a.shape[0], -1).all(1))} of {a.shape[0]} trajectories"


class Pair:
    """The engine with the memo and its comparator, run in lockstep.  `between(eng, shared)` is applied to both ahead of an
    iteration; every iteration is compared and its number of device matches recorded."""

    def __init__(self, d, B, dtype, N=N, **kw):
        self.cfg = problem(d, B, N)
        self.eng = make_engine(self.cfg, B, dtype, True, **kw)
        self.ref = make_engine(self.cfg, B, dtype, False, **kw)
        self.hits = []
        self.it = 0

    def step(self, between=None, compare=True):
        for e in (self.eng, self.ref):
            if between is not None:
                between(e, e is self.eng)
        m0 = matches()
        self.eng.run_outer()
        self.ref.run_outer()
        self.it += 1
        self.hits.append(matches() - m0)
        if compare:
            assert_same_bits(self.eng, self.ref, f"iteration {self.it}")
        for e in (self.eng, self.ref):
            finish(e)
        return self


def first_wave_inactive(d, B):
    inactive = np.zeros(B, dtype=np.int32)
    inactive[:64 // (3 * d)] = 1
    return inactive


# B = 5: a partial wavefront; 15: three wavefronts at d = 3, the last partial; 22: the first wavefront without a trajectory
@DTYPES
@pytest.mark.parametrize("d,B,masked", [(3, 5, False), (3, 15, False), (3, 22, True), (1, 5, False), (1, 15, False), (1, 22, True)])
def test_hit_path(d, B, masked, dtype):
    inactive = first_wave_inactive(d, B) if masked else None
    p = Pair(d, B, dtype, inactive=inactive)
    assert p.eng._outer_shares_records() and not p.ref._outer_shares_records()
    p.step().step().step()
    assert p.hits == [0, 1, 1]
    got = state(p.eng)
    assert np.isfinite(got["cost"]).all()
    if masked:
        off = inactive != 0
        assert (got["K"][off] == 7.0).all() and (got["k"][off] == -7.0).all()
        assert (got["K"][~off] != 7.0).any(axis=(1, 2, 3)).all()
    else:
        assert (got["K"][:, :-1] != 0).any(axis=(1, 2, 3)).all()


def scale_cuu(f, comparator=True):
    def change(eng, shared):
        # in place on the device, no engine call.  (The comparator writes its per-trajectory tables anew at the end of every
        # iteration: it takes the change on top of them, and nothing to have them restored.)
        if shared or comparator:
            (eng._Cuu_sh[0] if shared else eng.Cuu)[..., 3, 0, 0] *= f
    return change


def new_rho(rho):
    def change(eng, shared):
        eng.set_admm(rho_u=rho, u_box=(-3.0, 3.0), relax=1.0)
        build(eng)
        eng.expand()
    return change


def scale_par(f):
    def change(eng, shared):
        eng.model_par[1] *= f                              # b0 of the double integrator's parameter row
    return change


@DTYPES
@pytest.mark.parametrize("kind", ["cuu", "rho", "par"])
def test_content_invalidation(kind, dtype):
    change, restore = {"cuu": (scale_cuu(2.0), scale_cuu(0.5, comparator=False)), "rho": (new_rho(4e-2), new_rho(1e-2)),
                       "par": (scale_par(2.0), scale_par(0.5))}[kind]              # powers of two: restored exactly
    p = Pair(3, 15, dtype)
    p.step().step()
    p.step(change)                                         # the inputs differ from the snapshot: recomputed
    p.step(restore)                                        # ... and differ again (the snapshot holds the changed ones)
    p.step()
    assert p.hits == [0, 1, 0, 0, 1]


@DTYPES
def test_k_refreshed_on_a_hit(dtype):
    p = Pair(3, 15, dtype)
    p.step()
    p.step(lambda eng, shared: eng.K.zero_())
    assert p.hits == [0, 1]
    assert (state(p.eng)["K"][:, :-1] != 0).any(axis=(1, 2, 3)).all()


@DTYPES
def test_mask_changes_on_a_hit(dtype):
    B = 22
    inactive = first_wave_inactive(3, B)
    p = Pair(3, B, dtype, inactive=inactive)
    p.step().step()
    off = inactive != 0
    got = state(p.eng)
    assert (got["K"][off] == 7.0).all() and (got["k"][off] == -7.0).all()

    def wake(eng, shared):
        eng.outer_active.fill_(1)
        eng.begin_outer()
        eng.expand()
    p.step(wake)
    assert p.hits == [0, 1, 1]
    got = state(p.eng)
    assert (got["K"][off] != 7.0).any(axis=(1, 2, 3)).all() and (got["k"][off] != -7.0).any(axis=(1, 2)).all()


@DTYPES
def test_not_pd_is_never_committed(dtype):
    from isls import _capi as capi
    p = Pair(3, 15, dtype)
    keep = p.eng._Cuu_sh.clone()

    def indefinite(eng, shared):
        (eng._Cuu_sh[0] if shared else eng.Cuu)[..., 0, 0] = -1e6
    for _ in range(3):
        p.step(indefinite, compare=False)
        assert ((state(p.eng)["status"] & capi.ST_NOT_PD) != 0).all()
    assert p.hits == [0, 0, 0]                             # the same indefinite inputs three times: `filled` stayed 0

    def definite(eng, shared):
        if shared:
            eng._Cuu_sh.copy_(keep)
        cfg = p.cfg
        eng.set_nominal(np.repeat(cfg["x0"][:, None, :], cfg["N"], axis=1), cfg["u0"])
        eng.zu.zero_()
        eng.begin_outer()
        eng.expand()
    p.step(definite)
    p.step()
    assert p.hits[3:] == [0, 1]
    assert (state(p.eng)["status"] & capi.ST_NOT_PD == 0).all()


@DTYPES
def test_layout_toggles(dtype):
    p = Pair(3, 15, dtype)
    p.step().step()

    def dense(eng, shared):
        eng.use_model_structure = False
    def structured(eng, shared):
        eng.use_model_structure = True
    def caller_ab(eng, shared):
        eng.A = eng.A.clone()
        eng.Bm = eng.Bm.clone()
        build(eng)
    p.step(dense)                                          # the general layout: no shared records, the memo is not consulted
    p.step(structured)                                     # the kept table's inputs are what they were
    p.step(caller_ab)
    assert p.hits == [0, 1, 0, 1, 0]


def test_two_engines_of_different_horizon_interleaved():
    a, b = Pair(3, 15, F64, N=12), Pair(3, 15, F64, N=10)
    for _ in range(3):
        a.step()
        b.step()
    assert a.hits == [0, 1, 1] and b.hits == [0, 1, 1]


@DTYPES
@pytest.mark.parametrize("x_box", [None, (-0.4, 1.2)], ids=["u_box", "x_and_u_box"])
@pytest.mark.parametrize("mode", ["chol", "inv"])
@pytest.mark.parametrize("d,N_", [(3, 2), (3, 12), (1, 12)])
def test_first_pass_identity(d, N_, mode, x_box, dtype):
    """J = 1: k is the first feed-forward pass alone -- on a miss the recursion inside the gain launch (isls_riccati_gain_ff_*'s
    kernel), on a hit the stand-in pass on the kept table.  Both against the comparator's gain launch, bit for bit, in both
    solve modes, with and without a state block (its weight rows and targets enter the recursion's gradient sums)."""
    from isls import _capi as capi
    p = Pair(d, 15, dtype, N=N_, J=1, solve_mode=capi.SOLVE_INV if mode == "inv" else capi.SOLVE_CHOL, x_box=x_box)
    assert p.eng._outer_shares_records()
    p.step().step().step()
    assert p.hits == [0, 1, 1]
    assert (state(p.eng)["k"] != 0).any()


@DTYPES
def test_empty_batch_leaves_the_memo_alone(dtype):
    """B = 0 in every block of an argument list that otherwise declares the shared form: ISLS_OK, nothing launched, no check
    counted and the entry untouched -- the next real call still finds its table and matches."""
    from isls import _capi as capi
    p = Pair(3, 15, dtype)
    p.step()
    a = p.eng._outer_args
    before = capi.gain_memo_stats()
    for blk in (a.gain, a.ff, a.ro, a.admm):
        blk.B = 0
    p.eng.run_outer()                                      # raises on anything but ISLS_OK
    torch.cuda.synchronize()
    assert capi.gain_memo_stats() == before
    for blk in (a.gain, a.ff, a.ro, a.admm):
        blk.B = 15
    p.step()
    assert p.hits == [0, 1]
