"""numpy check of isls_columns_rollout_* (the closed loop of every feedback column on the linear model and the dense identity
dx = Su du + Sx of isls/isls.py:589-590), shared by tests/test_isls_admm.py and tests/test_riccati_slot_edges_gpu.py."""
import numpy as np


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, float(np.max(np.abs(b)))))


def check_columns_rollout(n, m, C, N, dtype, tol, active=None):
    """active: int32 [B] mask of the batch; None: five problems with problem 3 inactive."""
    import torch
    from isls.engine import kernels
    from oracle.isls_admm_dense import transfer_matrices
    rng = np.random.default_rng(n * 10 + m)
    if active is None:
        active = np.ones(5, dtype=np.int32)
        active[3] = 0
    active = np.ascontiguousarray(active, dtype=np.int32)
    B = int(active.shape[0])
    A = (np.eye(n) + 0.1 * rng.standard_normal((B, N, n, n))).astype(dtype)
    Bm = (0.3 * rng.standard_normal((B, N, n, m))).astype(dtype)
    K = (0.2 * rng.standard_normal((B, N, m, n))).astype(dtype)
    k = rng.standard_normal((C, B, N, m)).astype(dtype)
    Rr = (np.eye(m) * 0.7 + 0.05 * np.ones((m, m))).astype(dtype)[None]
    Cuu = (2 * 0.3 * np.eye(m) + 2 * Rr).astype(dtype)                         # [1,m,m]: shared over batch and time
    c0u = rng.standard_normal((B, N, m)).astype(dtype)
    zu, lu = rng.standard_normal((C, B, N, m)).astype(dtype), rng.standard_normal((C, B, N, m)).astype(dtype)
    dev = lambda a: torch.as_tensor(a, device="cuda")                          # noqa: E731
    dx, du = torch.full((C, B, N, n), 7.0, dtype=dev(A).dtype, device="cuda"), torch.full((C, B, N, m), 7.0, dtype=dev(A).dtype, device="cuda")
    kernels().columns_rollout(dev(A), dev(Bm), dev(Cuu), dev(c0u), dev(K), dev(k), dx, du, Rr=dev(Rr), zu=dev(zu), lu=dev(lu),
                              active=dev(active))
    torch.cuda.synchronize()
    dx, du = dx.cpu().numpy(), du.cpu().numpy()
    off = np.flatnonzero(active == 0)
    assert (dx[:, off] == 7).all() and (du[:, off] == 7).all()                 # inactive problems untouched
    for b in np.flatnonzero(active):
        Sw, Su = transfer_matrices(A[b].astype(np.float64), Bm[b].astype(np.float64))
        for c in range(C):
            x0 = np.zeros(n)
            if c:
                x0[c - 1] = 1.0
            # closed loop on the linear model, then the dense identity dx = Su du + Sx (isls.py:589-590)
            x, us = x0.copy(), []
            for t in range(N - 1):
                us.append(K[b, t].astype(np.float64) @ x + k[c, b, t])
                x = A[b, t].astype(np.float64) @ x + Bm[b, t].astype(np.float64) @ us[-1]
            g = (c == 0) * c0u[b, N - 1].astype(np.float64) - 2 * Rr[0].astype(np.float64) @ (zu[c, b, N - 1].astype(np.float64) - lu[c, b, N - 1])
            us.append(-np.linalg.solve(Cuu[0].astype(np.float64), g))
            us = np.array(us)
            assert np.isfinite(du[c, b]).all() and np.isfinite(dx[c, b]).all()
            assert rel(du[c, b], us) < tol, (int(b), c)
            assert rel(dx[c, b].reshape(-1), Sw[:, :n] @ x0 + Su @ us.reshape(-1)) < tol * 10, (int(b), c)
