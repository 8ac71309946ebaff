"""Costs with nonlinear path constraints (isls.costs.Custom(constraints=K)) on the CPU: registration keys on the constraint count,
the row limit W + K + 1 <= 16 is checked ahead of any compile, a source without `constraint` (or with another arity) comes back with
the compiler's log, the programs compile for gfx950 in both precisions with the update kernel inside, the numpy restatement's
derivatives agree with central differences, and the restatement itself converges on the end-to-end problem of the GPU test."""
import numpy as np
import pytest

from isls import _capi as capi
from isls import costs, models

import al_reference as al
from test_user_model_host import kernels_of


def test_registration_keys_on_constraints():
    src = al.full_source(4, 2, 0, 2)
    a = costs.Custom(4, 2, al.PAR, src, constraints=2)
    b = costs.Custom(4, 2, al.PAR, src, constraints=2)
    c = costs.Custom(4, 2, al.PAR, al.full_source(4, 2, 0, 1), constraints=1)
    d = costs.Custom(4, 2, al.PAR, al.full_source(4, 2, 0, 2, constraints=False))
    assert a.cost_model == b.cost_model and len({a.cost_model, c.cost_model, d.cost_model}) == 3
    lib = capi.library()
    assert lib.isls_user_cost_n_con(a.cost_model) == 2 and lib.isls_user_cost_n_con(d.cost_model) == 0
    assert capi.user_cost_n_tab(a.cost_model) == 3 and capi.user_cost_n_tab(c.cost_model) == 2 and a.n_tab == 0 and a.n_con == 2
    t = costs.Custom(4, 2, al.PAR, al.full_source(4, 2, 12, 3), table=np.zeros((5, 12)), constraints=3)
    assert capi.user_cost_n_tab(t.cost_model) == 16 and t.n_tab == 12


def test_row_limit_is_checked_before_any_compile():
    with pytest.raises(ValueError, match=r"W = 13.*K = 3.*17"):
        costs.Custom(4, 2, al.PAR, "this is not C++", table=np.zeros((5, 13)), constraints=3)
    with pytest.raises(ValueError, match=r"W = 0.*K = 16.*17"):
        costs.Custom(4, 2, al.PAR, "this is not C++", constraints=16)
    uid = np.zeros(1, dtype=np.int32)
    lib = capi.library()
    rc = lib.isls_user_cost_create_con(al.full_source(4, 2, 0, 2).encode(), 4, 2, 10, 2, 2, uid.ctypes.data_as(capi.C.POINTER(capi.C.c_int32)))
    assert rc == capi.ERR_UNSUPPORTED                            # n_tab < n_con + 1


def test_bad_sources_come_back_with_the_log():
    with pytest.raises(capi.IslsError, match="constraint"):      # no `constraint` at all
        costs.Custom(4, 2, al.PAR, al.full_source(4, 2, 0, 2, constraints=False) + "\n// k2", constraints=2)
    with pytest.raises(capi.IslsError, match="no matching function"):   # the forms with a row, registered without a table
        costs.Custom(4, 2, al.PAR, al.full_source(4, 2, 3, 2), constraints=2)


@pytest.mark.parametrize("n, m, mdl", [(4, 2, "car"), (6, 3, "lti"), (9, 3, "arm")])
@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_programs_compile_with_the_update_kernel(n, m, mdl, dtype, T):
    cst = costs.Custom(n, m, al.PAR, al.full_source(n, m, 0, 3), constraints=3)
    model = {"car": models.CarSimple(0.1), "arm": models.Planar3R(0.05),
             "lti": models.LTI(np.eye(6) + 0.01 * np.arange(36).reshape(6, 6), np.ones((6, 3)))}[mdl]
    for code in (cst.code(None, dtype), cst.code(model, dtype)):
        ks = kernels_of(code)
        upd = [v for k, v in ks.items() if k.startswith(f"_ZN4isls29user_constraint_update_kernelI{T}Li{n}ELi{m}E")]
        assert len(upd) == 1, sorted(ks)
        assert upd[0][".private_segment_fixed_size"] == 0 and upd[0][".group_segment_fixed_size"] == 0, upd[0]
    plain = kernels_of(costs.Custom(n, m, al.PAR, al.full_source(n, m, 0, 3, constraints=False)).code(None, dtype))
    assert not any("user_constraint_update" in k for k in plain)


@pytest.fixture(scope="module")
def library_table():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import scan_kernels
    sys.path.pop(0)
    return scan_kernels.kernel_table(scan_kernels.DEFAULT_LIB)


@pytest.mark.parametrize("n, m, mdl", [(4, 2, "car"), (6, 3, "lti"), (9, 3, "arm")])
@pytest.mark.parametrize("dtype, T", [(np.float64, "d"), (np.float32, "f")])
def test_constraints_add_no_scratch_to_the_line_search_and_the_expansion(library_table, n, m, mdl, dtype, T):
    """Scratch bytes of every rollout variant with K = 3 constraints, next to the same stage without them and to the built-in
    family's kernel: never more than the built-in's (the bound test_user_cost_host.py holds every user cost to); the expansion and
    the update kernel stay in registers."""
    from test_user_model_host import rollout_variants
    model, tid = {"car": (models.CarSimple(0.1), capi.MODEL_CAR), "arm": (models.Planar3R(0.05), capi.MODEL_ARM3R),
                  "lti": (models.LTI(np.eye(6) + 0.01 * np.arange(36).reshape(6, 6), np.ones((6, 3))), capi.MODEL_LTI)}[mdl]
    ks = {lab: kernels_of(c.code(model, dtype)) for lab, c in
          (("plain", costs.Custom(n, m, al.PAR, al.full_source(n, m, 0, 3, constraints=False))),
           ("con", costs.Custom(n, m, al.PAR, al.full_source(n, m, 0, 3), constraints=3)))}
    rv = {lab: rollout_variants(k, T, n, m, tid) for lab, k in ks.items()}
    ref = rollout_variants(library_table, T, n, m, tid)
    assert ref and set(rv["con"]) == set(ref) == set(rv["plain"])
    for jo in sorted(ref):
        sc = {lab: ks[lab][rv[lab][jo]][".private_segment_fixed_size"] for lab in ks}
        print(f"({n},{m}) {T} rollout (JM, OCC) = {jo}: scratch bytes plain {sc['plain']}, K = 3 {sc['con']}, built-in {library_table[ref[jo]]['scratch']}")
        assert sc["con"] <= library_table[ref[jo]]["scratch"], (jo, sc)
    for name in ("user_expand_kernel", "user_constraint_update_kernel"):
        k = [v for kk, v in ks["con"].items() if name in kk]
        assert len(k) == 1 and k[0][".private_segment_fixed_size"] == 0 and k[0].get(".vgpr_spill_count", 0) == 0, (name, k)


@pytest.mark.parametrize("W, K", [(0, 1), (0, 3), (1, 2), (12, 3)])
def test_restatement_derivatives_against_central_differences(W, K):
    rng = np.random.default_rng(W + K)
    N, n, m = 4, 4, 2
    x, u = rng.normal(size=(N, n)), rng.normal(size=(N, m))
    row = rng.normal(size=(N, W)) * 0.1 if W else None
    lam, mu = np.abs(rng.normal(size=(N, K))), 3.0
    lam[::2] = 0.0
    c, gr, H, h = al.augmented(x, u, al.PAR, row, lam, mu, W, K)
    assert np.abs(h).min() > 1e-3 and (h > 0).any() and (h <= 0).any()
    z, eps = np.concatenate([x, u], -1), 1e-6
    f = lambda zz: al.augmented(zz[:, :n], zz[:, n:], al.PAR, row, lam, mu, W, K)   # noqa: E731
    for i in range(n + m):
        dz = np.zeros_like(z)
        dz[:, i] = eps
        (cp, gp, _, _), (cm, gm, _, _) = f(z + dz), f(z - dz)
        assert np.abs((cp - cm) / (2 * eps) - gr[:, i]).max() < 1e-6
        assert np.abs((gp - gm) / (2 * eps) - H[:, i]).max() < 1e-6


def e2e_numpy():
    """The end-to-end problem of the GPU test through the restatement with the numpy iLQR"""
    p = al.E2E
    A, Bm = al.double_integrator()
    N, B, K = p["N"], p["B"], p["K"]
    x0 = al.e2e_starts()
    state = dict(x=np.stack([al.rollout(A, Bm, x0[b], np.zeros((N, 2))) for b in range(B)]), u=np.zeros((B, N, 2)))

    def solve(lam, mu):
        for b in range(B):
            cost = lambda x, u: float(al.augmented(x, u, al.PAR, None, lam[b], mu[b], 0, K)[0].sum())   # noqa: E731
            expand = lambda x, u: al.augmented(x, u, al.PAR, None, lam[b], mu[b], 0, K)[1:3]             # noqa: E731
            state["x"][b], state["u"][b] = al.numpy_solve(A, Bm, state["x"][b], state["u"][b], cost, expand, p["max_iter"])
        return state["x"].copy(), state["u"].copy()

    evaluate = lambda x, u: al.constraint(x, u, al.PAR, None, 0, K)[0]   # noqa: E731
    return al.outer_loop(solve, evaluate, np.zeros((B, N, K)), np.full(B, p["mu0"]), p["max_outer"], p["tol_con"], p["eta"], p["phi"],
                         p["mu_max"])


def test_restatement_converges_on_the_end_to_end_problem():
    x, u, lam, mu, viol, rounds = e2e_numpy()
    p = al.E2E
    print("viol per round:\n", viol, "\nmu", mu, "rounds", rounds)
    assert (viol[:, -1] <= p["tol_con"]).all() and viol.shape[1] <= p["max_outer"]
    assert (viol[:, 0] > p["tol_con"]).all()                    # the constraints bind: the unconstrained optimum violates them
    assert lam.max() > 0 and (al.constraint(x, u, al.PAR, None, 0, p["K"])[0] <= p["tol_con"]).all()
