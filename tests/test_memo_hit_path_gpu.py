"""The launches of a gain-memo call (csrc/capi.hip, csrc/gain_memo.hip): check -> gain launch -> stand-in first pass.

On a miss block 0 of the gain launch writes the entry's table itself and marks it filled (no commit launch); on a hit the
stand-in pass (riccati_ffrec2_kernel, FU) writes the K array from the records it stages (no broadcast launch, except for a call
whose first pass does not ride on the gain launch).  The comparator is the one tests/test_gain_memo_gpu.py uses -- the same engine
on per-trajectory Hessian tables, which never consults the memo -- and everything is compared bit for bit after every call:
K, k, the nominal, cost, z, lambda, best, the residuals and status (the engine exposes no view of the shared records: K and the
k they produce stand for them), together with what `isls_gain_memo_stats` counted for the call.

Shapes: d = 3 packs 7 trajectories into a gain wavefront (B = 1, 7, 8, 15, 600: one slot, a full wavefront, full plus one, two
with a partial last, many), d = 1 packs 21 (B = 21, 22); N = 2 is the horizon of one step, 7 and 12 an odd and an even number of
steps behind the first.  The sequential recursion is forced (ff_nseg = 1), as the shared form needs it.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gain_memo_gpu as base                          # noqa: E402  (helpers only: its engines, its comparator, its lockstep pair)

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
HORIZONS = pytest.mark.parametrize("N", [2, 7, 12])
SHAPES = [(3, 1), (3, 7), (3, 8), (3, 15), (3, 600), (1, 21), (1, 22)]


@pytest.fixture(autouse=True)
def fresh_memo():
    from isls import _capi as capi
    capi.gain_memo_clear()
    yield
    capi.gain_memo_clear()


def finish(eng):
    """End of an outer iteration: Engine.advance() where the engine keeps batch-shared Hessian tables, its parts elsewhere."""
    if eng._shared_hessian():
        eng.advance(linearize=eng._ab_src != "caller")
    else:
        eng.accept_x_step()
        eng.begin_outer()
        eng.expand()


class Pair(base.Pair):
    """base.Pair with the memo's two counters recorded per call.  `between(eng, tables_shared, first)` is applied to both engines
    ahead of a call: tables_shared tells whether the engine keeps the batch-shared Hessian tables (written once) or a table per
    trajectory (written anew at the end of every iteration), first whether it is the engine under test."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.checks = []

    def step(self, between=None, compare=True):
        from isls import _capi as capi
        for e in (self.eng, self.ref):
            if between is not None:
                between(e, e._shared_hessian(), e is self.eng)
        c0, m0 = capi.gain_memo_stats()
        self.eng.run_outer()
        self.ref.run_outer()
        self.it += 1
        c1, m1 = capi.gain_memo_stats()
        self.checks.append(c1 - c0)
        self.hits.append(m1 - m0)
        if compare:
            base.assert_same_bits(self.eng, self.ref, f"iteration {self.it}")
        for e in (self.eng, self.ref):
            finish(e)
        return self


def change_cuu(f, every=True):
    """One word of the Cuu table of step 0, in place on the device.  A batch-shared table keeps the change; an engine with a table
    per trajectory writes it anew at the end of every iteration and takes the change again ahead of every later call
    (every = False: those engines only)."""
    def change(eng, tables_shared, first):
        if every or not tables_shared:
            (eng._Cuu_sh[0] if tables_shared else eng.Cuu)[..., 0, 0, 0] *= f
    return change


def clear_memo(eng, tables_shared, first):
    change_cuu(2.0, every=False)(eng, tables_shared, first)
    if first:
        from isls import _capi as capi
        capi.gain_memo_clear()


@DTYPES
@HORIZONS
@pytest.mark.parametrize("d,B", SHAPES)
def test_miss_hit_sequences(d, B, N, dtype):
    p = Pair(d, B, dtype, N=N)
    # a batch of one declares no batch stride at all: its comparator shares records as well and takes the same memo entry right
    # behind the engine (same inputs, bit for bit), so every call of the comparator is one more check and one more match
    both = 1 if B == 1 else 0
    assert p.eng._outer_shares_records() and p.ref._outer_shares_records() == bool(both)
    p.step().step().step()                                     # miss, hit, hit
    p.step(change_cuu(2.0))                                    # one Cuu word changed in place: miss
    p.step(change_cuu(2.0, every=False))                  # hit on the table block 0 wrote in the call before
    p.step(clear_memo)                                         # entries freed: a new entry, filled by this call
    p.step(change_cuu(2.0, every=False))
    assert p.hits == [h + both for h in (0, 1, 1, 0, 1, 0, 1)]
    assert p.checks == [1 + both] * 7
    got = base.state(p.eng)
    assert np.isfinite(got["cost"]).all() and np.isfinite(got["K"]).all()
    assert (got["K"][:, :-1] != 0).any(axis=(1, 2, 3)).all() and (got["K"][:, -1] == 0).all()


def masks(d, B):
    tpw = 64 // (3 * d)
    first = np.zeros(B, dtype=np.int32)
    first[:tpw] = 1                                            # block 0 of the gain launch has no trajectory of its own
    scattered = np.zeros(B, dtype=np.int32)
    scattered[1::3] = 1
    scattered[tpw:2 * tpw] = 1                                 # ... and a whole wavefront in the middle has none
    both = np.maximum(first, scattered)
    return {"first_wavefront": first, "scattered": scattered, "both": both}


@DTYPES
@pytest.mark.parametrize("kind", ["first_wavefront", "scattered", "both"])
@pytest.mark.parametrize("d,B,N", [(3, 22, 7), (3, 600, 12), (1, 22, 2), (1, 64, 7)])
def test_masked_trajectories_keep_their_k(d, B, N, kind, dtype):
    inactive = masks(d, B)[kind]
    p = Pair(d, B, dtype, N=N, inactive=inactive)              # K, k pre-filled with 7 / -7
    p.step().step().step()
    assert p.hits == [0, 1, 1] and p.checks == [1, 1, 1]
    off = inactive != 0
    got, want = base.state(p.eng), base.state(p.ref)
    assert (got["K"][off] == 7.0).all() and (got["k"][off] == -7.0).all()
    assert np.array_equal(got["K"][~off].view(np.uint8), want["K"][~off].view(np.uint8))
    assert (got["K"][~off] != 7.0).all()


@DTYPES
@pytest.mark.parametrize("d,B,N", [(3, 15, 7), (3, 600, 12), (1, 22, 2)])
def test_k_array_replaced_between_two_hits(d, B, N, dtype):
    p = Pair(d, B, dtype, N=N)
    p.step().step()

    def new_k(eng, tables_shared, first):
        eng.K = torch.full_like(eng.K, float("nan"))           # another allocation: the argument block is marshalled again
        base.build(eng)
    p.step(new_k)
    assert p.hits == [0, 1, 1]
    assert np.isfinite(base.state(p.eng)["K"]).all()           # (and equal to the comparator's, bit for bit: step() compared)


@DTYPES
@pytest.mark.parametrize("d,B,N", [(3, 15, 7), (1, 21, 12), (3, 8, 2)])
def test_not_pd_miss_leaves_the_entry_unfilled(d, B, N, dtype):
    from isls import _capi as capi
    p = Pair(d, B, dtype, N=N)
    p.step()
    keep = p.eng._Cuu_sh.clone()

    def indefinite(eng, tables_shared, first):
        (eng._Cuu_sh[0] if tables_shared else eng.Cuu)[..., 0, 0] = -1e6
    p.step(indefinite, compare=False)
    p.step(indefinite, compare=False)                          # the same indefinite inputs again: recomputed, `filled` stayed clear
    assert ((base.state(p.eng)["status"] & capi.ST_NOT_PD) != 0).all()

    def definite(eng, tables_shared, first):
        if tables_shared:
            eng._Cuu_sh.copy_(keep)
        cfg = p.cfg
        eng.set_nominal(np.repeat(cfg["x0"][:, None, :], cfg["N"], axis=1), cfg["u0"])
        eng.zu.zero_()
        eng.begin_outer()
        eng.expand()
    p.step(definite)
    p.step()
    assert p.hits == [0, 0, 0, 0, 1] and p.checks == [1] * 5
    assert (base.state(p.eng)["status"] & capi.ST_NOT_PD == 0).all()


def test_hit_without_a_stand_in_pass():
    """More gain wavefronts than the device has SIMDs (21 trajectories per wavefront at d = 1): the first pass does not ride on the
    gain launch, so a hit has no stand-in pass and the K broadcast launch fills the K array."""
    sm = torch.cuda.get_device_properties(0).multi_processor_count
    B = 21 * 4 * sm + 1
    p = Pair(1, B, F64, N=2)
    def nan_k(eng, tables_shared, first):
        eng.K.fill_(float("nan"))
    p.step(nan_k).step(nan_k)
    assert p.hits == [0, 1] and p.checks == [1, 1]
    assert np.isfinite(base.state(p.eng)["K"]).all()


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 4096])
def test_reduce_convergence_table(B, world):
    """isls_reduce_convergence_table against numpy, random activity and status masks, at the tolerances of
    test_reduce_convergence_against_oracle: the cost sum to 1e-13 relative, maxima and counts exactly; the other ranks' rows,
    pre-filled with a sentinel, read zero afterwards (the kernel zeroes them)."""
    from dual import hip_kernels
    hip = hip_kernels()
    rng = np.random.default_rng(1000 * world + B)
    cost = rng.uniform(0.5, 2.0, B) * 10.0 ** rng.integers(-3, 4, B)
    res = np.abs(rng.standard_normal((B, 2))) * 10.0 ** rng.integers(-6, 1, (B, 1))
    res[rng.random(B) < 0.1] = 0.0
    for p_act, p_st in ((0.5, 0.1), (1.0, 0.0), (0.0, 1.0)):
        active = (rng.random(B) < p_act).astype(np.int32)
        status = np.where(rng.random(B) < p_st, rng.integers(1, 8, B), 0).astype(np.int32)
        ref = np.array([cost.sum(), max(0.0, res[:, 0].max()), max(0.0, res[:, 1].max()), float((active != 0).sum()),
                        float((status != 0).sum())])
        dev = [torch.from_numpy(a).cuda() for a in (cost, res, active, status)]
        for rank in range(world):
            table = torch.full((world, 5), -3.0, dtype=torch.float64, device="cuda")
            hip.reduce_convergence_table(*dev, table, rank)
            torch.cuda.synchronize()
            t = table.cpu().numpy()
            assert abs(t[rank, 0] - ref[0]) <= 1e-13 * abs(ref[0]), (rank, t[rank], ref)
            assert np.array_equal(t[rank, 1:], ref[1:]), (rank, t[rank], ref)
            assert not np.delete(t, rank, axis=0).any(), f"rows other than {rank} of {world} not zeroed"
