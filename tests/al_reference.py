"""Numpy restatement of the augmented Lagrangian of isls.costs.Custom(constraints=K): the test costs and constraints (as HIP C++
source and as numpy, with analytic gradients and Hessians), the augmented stage in the PHR form, the multiplier and penalty update,
a plain numpy iLQR for linear dynamics (the CPU tests have no device) and the outer loop over any `solve` callback -- the numpy
iLQR, or the host route of iSLS.solve (a cost and a get_Cs given as Python callables, one iSLS of batch 1 per trajectory: the
host route's callbacks do not know which trajectory they serve, and the multipliers are per trajectory).

The test problem, for any (n, m) with n >= 4, m >= 1; par = [wu, wx, wT, cx, cy, r, vmax, c, goal0, goal1]:
    stage      = wu |u|^2 + w_t ((x0 - goal0 - row[0])^2 + (x1 - goal1)^2 + 0.1 sum_{i >= 2} x_i^2),  w_t = wx, or wT at t = N - 1
    g0         = r^2 - ((x0 - cx - row[W-1])^2 + (x1 - cy)^2)         stay outside a disc
    g1         = x2^2 + x3^2 - vmax^2                                  a speed limit
    g2         = x0 u0 - c                                             couples x and u
(row: the user's W table words; absent for W = 0).  A cost with K constraints takes the first K."""
import numpy as np

PAR = np.array([0.05, 0.2, 20.0, 1.0, 0.1, 0.4, 0.9, 0.3, 2.0, 0.0])


def source(W, K, constraints=True):
    row = "const P *row, " if W else ""
    r0, rl = ("row[0]", f"row[{W - 1}]") if W else ("P(0)", "P(0)")
    g = ["g[0] = par[5] * par[5] - (dx * dx + dy * dy);", "g[1] = x[2] * x[2] + x[3] * x[3] - par[6] * par[6];",
         "g[2] = x[0] * u[0] - par[7];"]
    src = f"""
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, {row}int t, int N) {{
    S cu = S(P(0)), cr = S(P(0));
    for (int i = 0; i < ISLS_TEST_M; ++i) cu += u[i] * u[i];
    for (int i = 2; i < ISLS_TEST_N; ++i) cr += x[i] * x[i];
    const S d0 = x[0] - par[8] - {r0}, d1 = x[1] - par[9];
    const P w = t == N - 1 ? par[2] : par[1];
    return par[0] * cu + w * (d0 * d0 + d1 * d1 + P(0.1) * cr);
}}
"""
    if constraints:
        src += f"""
template <typename S, typename P>
__device__ void constraint(const S *x, const S *u, const P *par, {row}int t, int N, S *g) {{
    const S dx = x[0] - par[3] - {rl}, dy = x[1] - par[4];
    {' '.join(g[:K])}
}}
"""
    return src


def full_source(n, m, W, K, constraints=True):
    return f"#define ISLS_TEST_N {n}\n#define ISLS_TEST_M {m}\n" + source(W, K, constraints) + "#undef ISLS_TEST_N\n#undef ISLS_TEST_M\n"


def _rows(row, W, shape):
    if W == 0:
        z = np.zeros(shape)
        return z, z
    return np.broadcast_to(row[..., 0], shape), np.broadcast_to(row[..., W - 1], shape)


def stage(x, u, par, row, W):
    """[..., N] stage costs, with gradient [..., N, n+m] and Hessian [..., N, n+m, n+m]"""
    N, n, m = x.shape[-2], x.shape[-1], u.shape[-1]
    r0, _ = _rows(row, W, x.shape[:-1])
    w = np.where(np.arange(N) == N - 1, par[2], par[1])
    d0, d1 = x[..., 0] - par[8] - r0, x[..., 1] - par[9]
    c = par[0] * np.sum(u * u, -1) + w * (d0 * d0 + d1 * d1 + 0.1 * np.sum(x[..., 2:] ** 2, -1))
    g = np.zeros(x.shape[:-1] + (n + m,))
    g[..., 0], g[..., 1] = 2 * w * d0, 2 * w * d1
    g[..., 2:n] = 0.2 * w[:, None] * x[..., 2:]
    g[..., n:] = 2 * par[0] * u
    H = np.zeros(x.shape[:-1] + (n + m, n + m))
    H[..., 0, 0] = H[..., 1, 1] = np.broadcast_to(2 * w, x.shape[:-1])
    for i in range(2, n):
        H[..., i, i] = np.broadcast_to(0.2 * w, x.shape[:-1])
    for i in range(m):
        H[..., n + i, n + i] = 2 * par[0]
    return c, g, H


def constraint(x, u, par, row, W, K):
    """g [..., N, K] with gradients [..., N, K, n+m] and Hessians [..., N, K, n+m, n+m]"""
    n, m = x.shape[-1], u.shape[-1]
    _, rl = _rows(row, W, x.shape[:-1])
    lead = x.shape[:-1]
    g, J, H = np.zeros(lead + (K,)), np.zeros(lead + (K, n + m)), np.zeros(lead + (K, n + m, n + m))
    dx, dy = x[..., 0] - par[3] - rl, x[..., 1] - par[4]
    g[..., 0] = par[5] ** 2 - (dx * dx + dy * dy)
    J[..., 0, 0], J[..., 0, 1] = -2 * dx, -2 * dy
    H[..., 0, 0, 0] = H[..., 0, 1, 1] = -2.0
    if K > 1:
        g[..., 1] = x[..., 2] ** 2 + x[..., 3] ** 2 - par[6] ** 2
        J[..., 1, 2], J[..., 1, 3] = 2 * x[..., 2], 2 * x[..., 3]
        H[..., 1, 2, 2] = H[..., 1, 3, 3] = 2.0
    if K > 2:
        g[..., 2] = x[..., 0] * u[..., 0] - par[7]
        J[..., 2, 0], J[..., 2, n] = u[..., 0], x[..., 0]
        H[..., 2, 0, n] = H[..., 2, n, 0] = 1.0
    return g, J, H


def augmented(x, u, par, row, lam, mu, W, K):
    """The augmented stage per step [..., N], gradient, Hessian, and h = lam + mu g [..., N, K].  lam [..., N, K], mu [...]"""
    c, gr, H = stage(x, u, par, row, W)
    g, J, Hg = constraint(x, u, par, row, W, K)
    mu_ = np.asarray(mu, dtype=np.float64)[..., None, None]
    h = lam + mu_ * g
    on = h > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        off_term = np.where(mu_ > 0, lam * lam / (2 * mu_), 0.0)
    c = c + np.sum(np.where(on, lam * g + 0.5 * mu_ * g * g, -off_term), -1)
    hon = np.where(on, h, 0.0)
    gr = gr + np.einsum("...k,...ki->...i", hon, J)
    H = H + np.einsum("...k,...kij->...ij", hon, Hg) + np.einsum("...k,...ki,...kj->...ij", np.where(on, mu_, 0.0) * np.ones_like(g), J, J)
    return c, gr, H, h


def update(g, lam, mu, viol_prev, eta, phi, mu_max, do_update=True, active=None):
    """The multiplier and penalty update along one nominal: g [B, N, K], lam [B, N, K], mu [B], viol_prev [B] ->
    (lam', mu', viol, viol_prev')"""
    B = g.shape[0]
    act = np.ones(B, dtype=bool) if active is None else np.asarray(active).astype(bool)
    nan = np.isnan(g)
    v = np.where(nan, np.inf, np.maximum(g, 0.0)).reshape(B, -1).max(-1)
    lam2, mu2 = lam.copy(), mu.copy()
    if do_update:
        new = np.maximum(0.0, lam + mu[:, None, None] * np.where(nan, 0.0, g))
        lam2 = np.where(nan | ~act[:, None, None], lam, new)
        with np.errstate(invalid="ignore"):
            grow = act & (v > eta * viol_prev)
        mu2 = np.where(grow, np.minimum(phi * mu, mu_max), mu)
    return lam2, mu2, np.where(act, v, np.nan), np.where(act, v, viol_prev)


# ---- a numpy iLQR for x+ = A x + B u (the reference's loop: Riccati pass, line search over alphas with the acceptance test) -------
ALPHAS = 10 ** np.linspace(0, -5, 50)


def rollout(A, Bm, x0, u):
    x = np.zeros((u.shape[0], A.shape[0]))
    x[0] = x0
    for t in range(u.shape[0] - 1):
        x[t + 1] = A @ x[t] + Bm @ u[t]
    return x


def numpy_solve(A, Bm, x, u, cost, expand, max_iter, L=25, tol_fun=1e-5):
    """iLQR on one trajectory: cost(x, u) -> float, expand(x, u) -> (grad [N, n+m], Hess [N, n+m, n+m]).  Returns (x, u)."""
    N, n = x.shape
    m = u.shape[1]
    prev = cost(x, u)
    for _ in range(max_iter):
        gr, H = expand(x, u)
        Vx, Vxx = gr[-1, :n].copy(), H[-1, :n, :n].copy()       # u_{N-1} does not move the states: its own minimiser
        K, k = np.zeros((N, m, n)), np.zeros((N, m))
        k[-1] = -np.linalg.solve(H[-1, n:, n:], gr[-1, n:])
        for t in range(N - 2, -1, -1):
            Qx, Qu = gr[t, :n] + A.T @ Vx, gr[t, n:] + Bm.T @ Vx
            Qxx, Quu, Qux = H[t, :n, :n] + A.T @ Vxx @ A, H[t, n:, n:] + Bm.T @ Vxx @ Bm, H[t, n:, :n] + Bm.T @ Vxx @ A
            K[t], k[t] = -np.linalg.solve(Quu, Qux), -np.linalg.solve(Quu, Qu)
            Vx = Qx + K[t].T @ Quu @ k[t] + K[t].T @ Qu + Qux.T @ k[t]
            Vxx = Qxx + K[t].T @ Quu @ K[t] + K[t].T @ Qux + Qux.T @ K[t]
            Vxx = 0.5 * (Vxx + Vxx.T)
        best = (np.inf, None, None)
        for a in ALPHAS[:L]:
            xs, us = np.zeros_like(x), np.zeros_like(u)
            xs[0] = x[0]
            for t in range(N):
                us[t] = K[t] @ (xs[t] - x[t]) + a * k[t] + u[t]
                if t < N - 1:
                    xs[t + 1] = A @ xs[t] + Bm @ us[t]
            c = cost(xs, us)
            if c < best[0]:
                best = (c, xs, us)
        if not best[0] < prev:
            break
        x, u, small = best[1], best[2], abs(best[0] - prev) < tol_fun
        prev = best[0]
        if small:
            break
    return x, u


def outer_loop(solve, evaluate, lam, mu, max_outer, tol_con, eta, phi, mu_max, stop=True):
    """The augmented-Lagrangian outer loop of iSLS.solve_al over B trajectories: solve(lam, mu) -> nominal (x [B,N,n], u [B,N,m])
    under these multipliers, evaluate(x, u) -> g [B,N,K].  Returns (x, u, lam, mu, viol [B, rounds], rounds [B])."""
    B = lam.shape[0]
    prev, last, rounds, log = np.full(B, np.inf), np.full(B, np.inf), np.zeros(B, dtype=np.int64), []
    for _ in range(max_outer):
        x, u = solve(lam, mu)
        on = last > tol_con
        lam, mu, v, prev = update(evaluate(x, u), lam, mu, prev, eta, phi, mu_max, active=on)
        last = np.where(on, v, last)
        rounds += on
        log.append(last.copy())
        if stop and (last <= tol_con).all():
            break
    return x, u, lam, mu, np.stack(log, axis=1), rounds


# ---- the end-to-end problem: planar double integrator, a disc between start and goal, a speed limit --------------------------------
def double_integrator(dt=0.1):
    A = np.block([[np.eye(2), dt * np.eye(2)], [np.zeros((2, 2)), np.eye(2)]])
    Bm = np.vstack([0.5 * dt * dt * np.eye(2), dt * np.eye(2)])
    return A, Bm


E2E = dict(N=20, B=5, K=2, W=0, max_outer=10, max_iter=20, tol_con=1e-4, mu0=1.0, phi=10.0, mu_max=1e8, eta=0.25)


def e2e_starts():
    """x0 [B, 4] on either side of the line from start to goal (the disc at (1.0, 0.1), r = 0.4, lies on it), at rest"""
    return np.array([[0.0, 0.3, 0, 0], [0.0, -0.2, 0, 0], [-0.2, 0.5, 0, 0], [0.1, -0.4, 0, 0], [-0.1, 0.7, 0, 0]], dtype=np.float64)
