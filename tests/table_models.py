"""User models with a per-step table (isls.models.Custom(..., table=)): the sources the tests compile and their numpy restatements."""
import numpy as np

# x+ = A_t x + B_t u at (4, 2), W = 16: A_t = I + two off-diagonals per row (row[2i], row[2i+1]), B_t row i = row[8+2i : 10+2i]
LTV = """template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, const P *row, S *xn)
{
    for (int i = 0; i < 4; ++i)
        xn[i] = x[i] + row[2 * i] * x[(i + 1) % 4] + row[2 * i + 1] * x[(i + 2) % 4] + row[8 + 2 * i] * u[0] + row[9 + 2 * i] * u[1];
}"""


def ltv_AB(row):
    """row [..., 16] -> A [..., 4, 4], B [..., 4, 2]"""
    row = np.asarray(row, dtype=np.float64)
    A = np.zeros(row.shape[:-1] + (4, 4))
    B = np.zeros(row.shape[:-1] + (4, 2))
    for i in range(4):
        A[..., i, i] += 1.0
        A[..., i, (i + 1) % 4] += row[..., 2 * i]
        A[..., i, (i + 2) % 4] += row[..., 2 * i + 1]
        B[..., i, 0], B[..., i, 1] = row[..., 8 + 2 * i], row[..., 9 + 2 * i]
    return A, B


def ltv_step(x, u, row):
    A, B = ltv_AB(row)
    return np.einsum("...ij,...j->...i", A, x) + np.einsum("...ij,...j->...i", B, u)


def ltv_table(rng, N, B=None, scale=0.1):
    return scale * rng.standard_normal(((N, 16) if B is None else (B, N, 16)))


# the car of models.CarSimple with the time step row[0] and a lateral push row[1] (W = 2); no parameters used (par[0] unused)
CAR = """template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, const P *row, S *xn)
{
    const P dt = row[0];
    xn[0] = x[0] + dt * x[3] * cos(x[2]);
    xn[1] = x[1] + dt * x[3] * sin(x[2]) + row[1];
    xn[2] = x[2] + dt * x[3] * u[0];
    xn[3] = x[3] + dt * u[1];
}"""


def car_step(x, u, row):
    dt, push = row[..., 0], row[..., 1]
    return np.stack([x[..., 0] + dt * x[..., 3] * np.cos(x[..., 2]), x[..., 1] + dt * x[..., 3] * np.sin(x[..., 2]) + push,
                     x[..., 2] + dt * x[..., 3] * u[..., 0], x[..., 3] + dt * u[..., 1]], axis=-1)


def car_AB(x, u, row):
    dt = row[..., 0]
    A = np.zeros(x.shape[:-1] + (4, 4))
    B = np.zeros(x.shape[:-1] + (4, 2))
    for i in range(4):
        A[..., i, i] = 1.0
    th, v = x[..., 2], x[..., 3]
    A[..., 0, 2], A[..., 1, 2] = -dt * v * np.sin(th), dt * v * np.cos(th)
    A[..., 0, 3], A[..., 1, 3], A[..., 2, 3] = dt * np.cos(th), dt * np.sin(th), dt * u[..., 0]
    B[..., 2, 0], B[..., 3, 1] = dt * v, dt
    return A, B


def car_table(rng, N, B=None):
    shape = (N, 2) if B is None else (B, N, 2)
    t = np.empty(shape)
    t[..., 0] = 0.05 + 0.1 * rng.random(shape[:-1])
    t[..., 1] = 0.02 * rng.standard_normal(shape[:-1])
    return t


def generic_source(n, m, W, table):
    """A mildly nonlinear model at any (n, m) whose W constants c_k come from `row` (table=True) or from `par`: the same
    arithmetic either way, so a table whose every row repeats the constants must give the bits of the `par` form."""
    c = "row" if table else "par"
    sig = "const P *par, const P *row, S *xn" if table else "const P *par, S *xn"
    return f"""template <typename S, typename P>
__device__ void step(const S *x, const S *u, {sig})
{{
    for (int i = 0; i < {n}; ++i)
        xn[i] = x[i] + {c}[i % {W}] * sin(x[(i + 1) % {n}]) + {c}[(i + 1) % {W}] * u[i % {m}] + {c}[{W} - 1] * x[(i + 2) % {n}];
}}"""


def generic_consts(W):
    return 0.05 + 0.01 * np.arange(W)


def generic_step(n, m, W):
    """numpy restatement of generic_source(n, m, W, True): step(x [..., n], u [..., m], row [..., W])"""
    def step(x, u, row):
        return np.stack([x[..., i] + row[..., i % W] * np.sin(x[..., (i + 1) % n]) + row[..., (i + 1) % W] * u[..., i % m]
                         + row[..., W - 1] * x[..., (i + 2) % n] for i in range(n)], axis=-1)
    return step


def generic_table(rng, N, W, B=None):
    """rows that really differ, step to step and trajectory to trajectory, about generic_consts"""
    return generic_consts(W) * (1.0 + 0.5 * rng.standard_normal(((N, W) if B is None else (B, N, W))))


def candidates(step, table, xhat, uhat, K, k, alphas):
    """Every candidate of the line search of a batch at once: x [B, L, N, n], u [B, L, N, m]; table [N, W] or [B, N, W]"""
    B, N, n = xhat.shape
    L = len(alphas)
    tab = np.broadcast_to(table, (B,) + table.shape[-2:])
    x = np.broadcast_to(xhat[:, None, 0], (B, L, n)).copy()
    xs, us = [], []
    for t in range(N):
        u = (np.einsum("bij,blj->bli", K[:, t], x - xhat[:, None, t]) + alphas[None, :, None] * k[:, None, t]) + uhat[:, None, t]
        xs.append(x), us.append(u)
        x = step(x, u, tab[:, None, t])
    return np.stack(xs, axis=2), np.stack(us, axis=2)


def sample_rollouts(step, table, xhat, uhat, eps, K=None):
    """The samples of one sampling round: x [B, S, N, n], u [B, S, N, m] from xhat_0 with u_t = uhat_t + eps_t (open loop) or
    u_t = (uhat_t + K_t (x_t - xhat_t)) + eps_t (closed loop about the gains K [B, N, m, n]), stepping with row t at step t."""
    B, N, n = xhat.shape
    S = eps.shape[1]
    tab = np.broadcast_to(table, (B,) + table.shape[-2:])
    x = np.broadcast_to(xhat[:, None, 0], (B, S, n)).copy()
    xs, us = [], []
    for t in range(N):
        base = uhat[:, None, t] if K is None else uhat[:, None, t] + np.einsum("bij,bsj->bsi", K[:, t], x - xhat[:, None, t])
        u = base + eps[:, :, t]
        xs.append(x), us.append(u)
        x = step(x, u, tab[:, None, t])
    return np.stack(xs, axis=2), np.stack(us, axis=2)


def rollout(step, table, x0, K, k, xhat, uhat, alpha):
    """The closed-loop candidate of the line search: u_t = K_t (x_t - xhat_t) + alpha k_t + uhat_t, x_{t+1} = step(x_t, u_t, row_t)."""
    N = k.shape[0]
    x = np.array(x0, dtype=np.float64)
    xs, us = [], []
    for t in range(N):
        u = K[t] @ (x - xhat[t]) + alpha * k[t] + uhat[t]
        xs.append(x), us.append(u)
        x = step(x, u, table[t])
    return np.array(xs), np.array(us)
