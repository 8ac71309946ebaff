#!/usr/bin/env python3
"""Generate tests/golden/g15_moving_sets.npz by RUNNING THE REFERENCE (build container only), the way make_golden.py does:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg PYTHONPATH=<the reference checkout> python3 tests/golden/make_moving_sets.py

The reference is imported, never copied; only inputs and outputs of its own functions are stored.  Its set projections take
closures over all rows of a call at once, so a closure over an [R, d] array of per-row parameters is a constraint set that
moves from row to row (numpy broadcasting).  Three cases, R = 24 rows each:

  a  two spherical keep-out shells with linearly moving centres: project_set_convex(rho=1, max_iter=5, threshold=1e-2), then
     project_set_convex_dykstra(max_iter=50, tol=1e-5) -- the chain of the obstacle notebook (cell 12)
  b  two moving rotated keep-out squares through project_set_convex(rho=10, max_iter=15, threshold=1e-3) on rows of
     dimension 4 (the car's state, the squares act on its first two coordinates): Car notebook cell 18 with c per row
  c  a box with per-row bounds through project_bound

The iterations run are counted through the closures (one call per set and iteration).  The generator asserts that no count
changes when the threshold is scaled by 1 +- 1e-6 (no borderline stop), and that case a ends feasible.
"""
import os
import sys

import numpy as np

import isls as ref                                    # noqa: F401  (the REFERENCE package)
refproj = sys.modules["isls.projections"]             # `isls.projections` the attribute is shadowed by a dict

HERE = os.path.dirname(os.path.abspath(__file__))
assert "ilqr-admm_amd" not in refproj.__file__, refproj.__file__
R = 24


class Counted:
    """a projection closure that counts its calls"""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, v):
        self.calls += 1
        return self.fn(v)


def case_a(scale=1.0):
    rng = np.random.default_rng(15)
    t = np.arange(R)[:, None]
    centres = np.stack([np.array([0.2, 0.3]) + t * np.array([0.02, 0.0]),
                        np.array([1.1, 0.9]) + t * np.array([-0.01, -0.005])], axis=1)         # [R, 2, 2]
    radii, margin, upper = np.array([0.25, 0.2]), 1.1, 1e2
    x0 = np.linspace([0.0, 0.0], [1.2, 1.0], R) + 0.05 * rng.standard_normal((R, 2))
    shells = lambda: [Counted(lambda v, i=i: refproj.project_quadratic_batch(v - centres[:, i], 0.5 * (margin * radii[i]) ** 2, upper)   # noqa: E731
                              + centres[:, i]) for i in range(2)]
    p1, p2 = shells(), shells()
    y1 = refproj.project_set_convex(x0, As=[np.eye(2)] * 2, bs=[np.zeros(2)] * 2, projections=p1, rho=1, max_iter=5,
                                    threshold=1e-2 * scale)
    y2 = refproj.project_set_convex_dykstra(y1, projections=p2, max_iter=50, tol=1e-5 * scale)
    return dict(x0=x0, centres=centres, radii=radii, margin=margin, upper=upper, y_admm=y1, y=y2,
                iters=np.array([p1[0].calls, p2[0].calls]))


def case_b(scale=1.0):
    rng = np.random.default_rng(16)
    t = np.arange(R)[:, None]
    centres = np.stack([np.array([0.5, 0.4]) + t * np.array([0.04, 0.0]),
                        np.array([2.0, 1.2]) + t * np.array([-0.03, 0.02])], axis=1)           # [R, 2, 2]
    sizes, angle, margin, upper = np.array([[0.6, 0.3], [0.4, 0.5]]), 0.4, 0.5, 1e5
    x0 = np.concatenate([np.linspace([0.0, 0.2], [2.4, 1.6], R) + 0.05 * rng.standard_normal((R, 2)),
                         rng.standard_normal((R, 2))], axis=1)                               # [R, 4]
    Rm = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    prims = []
    for i in range(2):
        a_safe = sizes[i] + margin
        W = np.diag(a_safe[0] / a_safe) @ Rm.T
        Wi = np.linalg.inv(W)

        def square(v, i=i, W=W, Wi=Wi, l=a_safe[0] / 2):
            out = v.copy()
            out[:, :2] = refproj.project_square_batch((v[:, :2] - centres[:, i]) @ W.T, l, upper) @ Wi.T + centres[:, i]
            return out
        prims.append(Counted(square))
    y = refproj.project_set_convex(x0, As=[np.eye(4)] * 2, bs=[np.zeros(4)] * 2, projections=prims, rho=10, max_iter=15,
                                   threshold=1e-3 * scale)
    return dict(x0=x0, centres=centres, sizes=sizes, angle=angle, margin=margin, upper=upper, y=y, iters=np.array([prims[0].calls]))


def case_c():
    rng = np.random.default_rng(17)
    x0 = 2.0 * rng.standard_normal((R, 3))
    lo = -1.0 + 0.05 * np.arange(R)[:, None] * np.array([1.0, -0.5, 0.25])
    hi = lo + 0.5 + rng.uniform(size=(R, 3))
    return dict(x0=x0, lo=lo, hi=hi, y=refproj.project_bound(x0, lo, hi))


def main():
    a, b, c = case_a(), case_b(), case_c()
    for s in (1 - 1e-6, 1 + 1e-6):                              # no stop of a recorded run is borderline
        assert np.array_equal(case_a(s)["iters"], a["iters"]) and np.array_equal(case_b(s)["iters"], b["iters"])
    gap = min(np.min(np.linalg.norm(a["y"] - a["centres"][:, i], axis=1) / (a["margin"] * a["radii"][i])) for i in range(2))
    assert gap >= 1.0 - 1e-9, gap                               # every row ends on or outside its own step's balls
    moved = max(np.max(np.abs(d["y"] - d["x0"])) for d in (a, b, c))
    assert moved > 1e-2 and 1 < a["iters"][0] <= 5 and 1 < a["iters"][1] <= 51 and 1 < b["iters"][0] <= 15
    out = {f"{k}_{name}": np.asarray(v) for k, d in (("a", a), ("b", b), ("c", c)) for name, v in d.items()}
    path = os.path.join(HERE, "g15_moving_sets.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {os.path.basename(path)}: {os.path.getsize(path) / 1024:.1f} KiB; iterations a {a['iters'].tolist()} "
          f"b {b['iters'].tolist()}; case a feasibility {gap:.12f}")


if __name__ == "__main__":
    main()
