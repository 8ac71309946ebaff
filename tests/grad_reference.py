"""numpy restatement of iSLS.gradient: the adjoint sweep and the parameter / table directions of one trajectory.

J = sum_t c(x_t, u_t, cpar, crow_t, t, N), x_0 given, x_{t+1} = f(x_t, u_t, mpar, mrow_t) for t <= N-2.  f and c are numpy twins of
the device sources written on generic scalars; their partial derivatives are taken by the complex step (Im f(v + i h e_j) / h,
h = 1e-30: exact to rounding for the analytic functions of the AD contract, no truncation and no cancellation), so the twins must
branch on the real part of what they compare (`re`).  test_gradient_host.py pins the whole of it against central finite differences
of J itself.
"""
import numpy as np

H = 1e-30


def re(v):
    return np.real(v)


def jac(fun, v):
    """d fun / d v [p, k] of fun: R^k -> R^p (p = 1 for a scalar) at the real point v, by the complex step"""
    v = np.asarray(v, dtype=np.float64)
    cols = []
    for j in range(v.size):
        z = v.astype(np.complex128)
        z[j] += 1j * H
        cols.append(np.imag(np.atleast_1d(np.asarray(fun(z), dtype=np.complex128))) / H)
    return np.stack(cols, axis=1) if cols else np.zeros((np.atleast_1d(np.asarray(fun(v))).size, 0))


def _rows(tab, N):
    return np.zeros((N, 0)) if tab is None else np.asarray(tab, dtype=np.float64)


def rollout(f, x0, u, mpar, mtab=None):
    u = np.asarray(u, dtype=np.float64)
    N, mt = u.shape[0], _rows(mtab, u.shape[0])
    x = np.zeros((N, np.size(x0)))
    x[0] = x0
    for t in range(N - 1):
        x[t + 1] = np.asarray(f(x[t], u[t], mpar, mt[t]))
    return x


def total_cost(f, c, x0, u, mpar, cpar, mtab=None, ctab=None):
    """J of the rollout from x0 under u"""
    N, ct = np.shape(u)[0], _rows(ctab, np.shape(u)[0])
    x = rollout(f, x0, u, mpar, mtab)
    return sum(c(x[t], u[t], cpar, ct[t], t, N) for t in range(N))


def gradient(f, c, x, u, mpar, cpar, mtab=None, ctab=None, A=None, Bm=None):
    """All of iSLS.gradient for the trajectory (x [N, n], u [N, m]) as a dict: cost, costate, u, x0, model_params, model_table,
    cost_params, cost_table.  A, Bm [N, n, n], [N, n, m]: a caller's linearisation in the place of f's own."""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    mpar, cpar = np.asarray(mpar, dtype=np.float64), np.asarray(cpar, dtype=np.float64)
    N, n = x.shape
    mt, ct = _rows(mtab, N), _rows(ctab, N)
    cost = sum(c(x[t], u[t], cpar, ct[t], t, N) for t in range(N))
    cx = np.stack([jac(lambda v, t=t: c(v, u[t], cpar, ct[t], t, N), x[t])[0] for t in range(N)])
    cu = np.stack([jac(lambda v, t=t: c(x[t], v, cpar, ct[t], t, N), u[t])[0] for t in range(N)])
    lam, gu = np.zeros_like(x), np.zeros_like(u)
    lam[N - 1], gu[N - 1] = cx[N - 1], cu[N - 1]
    g_mp, g_mt = np.zeros(mpar.size), np.zeros_like(mt)
    for t in range(N - 2, -1, -1):
        At = jac(lambda v: f(v, u[t], mpar, mt[t]), x[t]) if A is None else A[t]
        Bt = jac(lambda v: f(x[t], v, mpar, mt[t]), u[t]) if Bm is None else Bm[t]
        lam[t] = cx[t] + At.T @ lam[t + 1]
        gu[t] = cu[t] + Bt.T @ lam[t + 1]
        g_mp += lam[t + 1] @ jac(lambda v: f(x[t], u[t], v, mt[t]), mpar)
        g_mt[t] = lam[t + 1] @ jac(lambda v: f(x[t], u[t], mpar, v), mt[t])
    g_cp = sum(jac(lambda v, t=t: c(x[t], u[t], v, ct[t], t, N), cpar)[0] for t in range(N))
    g_ct = np.stack([jac(lambda v, t=t: c(x[t], u[t], cpar, v, t, N), ct[t])[0] for t in range(N)])
    return dict(cost=float(np.real(cost)), costate=lam, u=gu, x0=lam[0].copy(), model_params=g_mp, model_table=g_mt,
                cost_params=g_cp, cost_table=g_ct)


def batch(f, c, x, u, mpar, cpar, mtab=None, ctab=None, A=None, Bm=None):
    """gradient() per trajectory of x [B, N, n], u [B, N, m], stacked; parameters [P] or [B, P], tables [N, W] or [B, N, W], A / Bm
    [N, ...] or [B, N, ...] (None: f's own)"""
    B = x.shape[0]

    def pick(v, nd, b):
        return None if v is None else (np.asarray(v)[b] if np.ndim(v) == nd + 1 else np.asarray(v))
    rows = [gradient(f, c, x[b], u[b], pick(mpar, 1, b), pick(cpar, 1, b), pick(mtab, 2, b), pick(ctab, 2, b), pick(A, 3, b),
                     pick(Bm, 3, b)) for b in range(B)]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# ---- numpy twins on generic scalars of the sources the gradient tests use ----------------------------------------------------
def quad_f(x, u, par, row):
    """tests/user_models.py QUAD"""
    dt, mass, inertia, arm, g = par
    f = u[0] + u[1]
    s, c = np.sin(x[2]), np.cos(x[2])
    return np.array([x[0] + dt * x[3], x[1] + dt * x[4], x[2] + dt * x[5], x[3] + dt * (-(f * s) / mass),
                     x[4] + dt * ((f * c) / mass - g), x[5] + dt * (arm * (u[0] - u[1]) / inertia)])


def car_f(x, u, par, row):
    """models.CarSimple(dt) (isls/models.py): [x, y, theta, v], [omega, a]; theta wraps to [0, 2 pi) (derivative 1)"""
    dt = par[0]
    th = x[2] + dt * x[3] * u[0]
    return np.array([x[0] + dt * x[3] * np.cos(x[2]), x[1] + dt * x[3] * np.sin(x[2]),
                     th - 2 * np.pi * np.floor(re(th) / (2 * np.pi)), x[3] + dt * u[1]])


def ltv_f(x, u, par, row):
    """tests/table_models.py LTV (4, 2), W = 16"""
    return np.array([x[i] + row[2 * i] * x[(i + 1) % 4] + row[2 * i + 1] * x[(i + 2) % 4] + row[8 + 2 * i] * u[0] + row[9 + 2 * i] * u[1]
                     for i in range(4)])


def windy_f(x, u, par, row):
    """the README's quadrotor in wind: QUAD with the horizontal acceleration row[0] (W = 1)"""
    e3 = np.zeros(6)
    e3[3] = 1.0
    return quad_f(x, u, par, row) + (par[0] * row[0]) * e3


def track_cost(x, u, par, row, t, N):
    """the README's tracking cost at (6, 2), W = 8: par = [w_u, w_x], row = [x_ref (6) | u_ref (2)]"""
    return par[1] * np.sum((x - row[:6]) ** 2) + par[0] * np.sum((u - row[6:8]) ** 2)


def al_cost(W, K, lam=None, mu=None):
    """tests/al_reference.py source(W, K) in its PHR-augmented form at the multipliers lam [N, K], penalty mu (None: the plain stage);
    the branch follows the real part, as the device's comparisons follow the value part"""
    def c(x, u, par, row, t, N):
        r0, rl = (row[0], row[W - 1]) if W else (0.0, 0.0)
        d0, d1 = x[0] - par[8] - r0, x[1] - par[9]
        w = par[2] if t == N - 1 else par[1]
        val = par[0] * np.sum(u * u) + w * (d0 * d0 + d1 * d1 + 0.1 * np.sum(x[2:] * x[2:]))
        if lam is None:
            return val
        dx, dy = x[0] - par[3] - rl, x[1] - par[4]
        g = [par[5] * par[5] - (dx * dx + dy * dy), x[2] * x[2] + x[3] * x[3] - par[6] * par[6], x[0] * u[0] - par[7]][:K]
        for i in range(K):
            h = lam[t, i] + mu * g[i]
            if re(h) > 0:
                val = val + lam[t, i] * g[i] + 0.5 * mu * g[i] * g[i]
            else:
                val = val - (lam[t, i] ** 2 / (2 * mu) if mu > 0 else 0.0)
        return val
    return c


def lti_f(A, Bm):
    return lambda x, u, par, row: A @ x + Bm @ u


def via_cost(zs, Qs, seq, u_std):
    """the via-point cost of set_cost_variables: (x - z)' Q (x - z) + u_std u'u, no 1/2"""
    def c(x, u, par, row, t, N):
        d = x - zs[seq[t]]
        return d @ (Qs[seq[t]] @ d) + u_std * (u @ u)
    return c
