"""The comparison helpers the GPU parity tests rest on (tests/helpers.py, tests/dual.py), on the CPU: a NaN in any compared
array, a wrong slot whose values are small next to the batch maximum and a wrong integer state must all fail; identical
non-finite values must agree."""
import numpy as np
import pytest

from helpers import compare_batched, compare_exact, rel_err

ARRAYS = ("K", "k", "xx", "xu", "zu", "lu", "res", "xhat", "uhat", "cost")


def _batch(seed=0, B=64, N=10, d=3):
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((B, N, d)) * 100.0
    return ref


def test_nan_in_the_last_compared_array_is_caught():
    """The outer-driver comparison walks K, k, ..., cost: a NaN in the LAST one (after finite errors in the others) must fail,
    which `max(generator)` does not guarantee (max([0.0, nan]) == 0.0)."""
    assert max([0.0, float("nan")]) == 0.0                       # the trap the helper must not fall into
    ref = {name: _batch(i) for i, name in enumerate(ARRAYS)}
    got = {name: v.copy() for name, v in ref.items()}
    got["cost"][17, 4, 1] = np.nan
    for name in ARRAYS[:-1]:
        assert compare_batched(name, got[name], ref[name], 1e-10) == 0.0
    with pytest.raises(AssertionError, match=r"cost: trajectory 17, index \(4, 1\)"):
        compare_batched("cost", got["cost"], ref["cost"], np.inf)
    got["cost"][17, 4, 1] = np.inf
    with pytest.raises(AssertionError, match="non-finite"):
        compare_batched("cost", got["cost"], ref["cost"], np.inf)


def test_small_trajectory_error_is_caught():
    """A 1e-8 relative error in a trajectory whose values are 1e-4 of the batch maximum: invisible to the whole-batch scale of
    rel_err (1e-12 there), caught by the per-trajectory one."""
    ref = _batch(1)
    ref[5] *= 1e-4 * np.abs(ref).max() / np.abs(ref[5]).max()
    got = ref.copy()
    got[5, 3, 2] += 1e-8 * np.abs(ref[5]).max()
    assert rel_err(got, ref) < 1e-10
    with pytest.raises(AssertionError, match=r"trajectory 5, index \(3, 2\)"):
        compare_batched("xx", got, ref, 1e-10)
    # this trajectory sits below the floor (1e-3 of the batch maximum): measured against the floor, 1e-8 * 1e-4 / 1e-3
    assert compare_batched("xx", got, ref, 1e-7) == pytest.approx(1e-9, rel=1e-6)


def test_floor_bounds_the_scale_of_vanishing_trajectories():
    """A trajectory of zeros is measured against floor * max(1, max|ref|), never against zero; the scale is never larger
    than rel_err's, so no assertion gets looser."""
    ref = _batch(2)
    ref[9] = 0.0
    got = ref.copy()
    got[9, 0, 0] = 1e-12
    e = compare_batched("lu", got, ref, np.inf)
    assert e == pytest.approx(1e-12 / (1e-3 * np.abs(ref).max()))
    assert e >= rel_err(got, ref)
    small = ref * 1e-6                                           # a batch far below 1: the floor is 1e-3 of 1
    got = small.copy()
    got[9, 0, 0] = 1e-14
    assert compare_batched("lu", got, small, np.inf) == pytest.approx(1e-11)


def test_identical_infinities_and_nans_agree():
    ref = _batch(3)
    ref[2, 1, 0], ref[40, 9, 2], ref[41, 0, 0] = np.nan, np.inf, -np.inf
    got = ref.copy()
    assert compare_batched("k", got, ref, 1e-15) == 0.0
    got[41, 0, 0] = np.inf                                       # the other sign: not the same value
    with pytest.raises(AssertionError, match=r"trajectory 41"):
        compare_batched("k", got, ref, np.inf)
    got = ref.copy()
    got[2, 1, 0] = 0.0                                           # a finite value where the oracle has a NaN
    with pytest.raises(AssertionError, match=r"trajectory 2"):
        compare_batched("k", got, ref, np.inf)


def test_shapes_one_dimensional_and_float32():
    ref = np.linspace(1.0, 2.0, 7) / 3.0
    got = ref.astype(np.float32)                                  # one trajectory per element, fp32 against fp64
    assert 0 < compare_batched("cost", got, ref, 1e-6) < 1e-7
    assert compare_batched("cost", got, got, 0.0) == 0.0
    with pytest.raises(AssertionError, match="shape"):
        compare_batched("cost", ref[:6], ref, 1.0)
    assert compare_batched("empty", np.zeros((0, 3)), np.zeros((0, 3)), 0.0) == 0.0


def test_integer_state_is_compared_exactly():
    best = np.arange(4096, dtype=np.int32) % 20
    compare_exact("best", best.copy(), best)
    got = best.copy()
    got[4095] = 3
    with pytest.raises(AssertionError, match=r"best: 1 mismatches, first at \(4095,\)"):
        compare_exact("best", got, best)
    with pytest.raises(AssertionError, match="shape"):
        compare_exact("status", best[:-1], best)
