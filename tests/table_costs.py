"""A tracking cost as a user cost with a per-step table (isls.costs.Custom(..., table=)), shared by the table-cost tests and
tools/user_cost_bench.py: the built-in via-point cost with one via point per step,

    sum_t (x_t - z_t)' Q_t (x_t - z_t) + u_std |u_t|^2,   Q_t diagonal,

restated as a six-argument `stage`.  Row t of the table holds z_t and the diagonal of Q_t over the first NZ states, par = [u_std]:
NZ = n where the 2 n words fit a row (16 at most), and 4 for the arm's nine states -- its joint angles and the first joint
velocity.  (The nine-state kernels compiled for two waves per SIMD sit at the register cap and spill already; the reads of a
16-word row in one step push one variant or another a few bytes past the built-in family's scratch: DESIGN section 7.)
With it: the tables of the built-in cost it restates, and its numpy value, gradient and Hessian."""
import numpy as np


def nz_of(n):
    return int(n) if 2 * int(n) <= 16 else 4


def width(n):
    return 2 * nz_of(n)


def tracking_source(n, m):
    nz = nz_of(n)
    return f'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, const P *row, int t, int N) {{
    S c = S(0);
    for (int j = 0; j < {nz}; ++j) {{
        const S d = x[j] - row[j];
        c += d * (row[{nz} + j] * d);
    }}
    for (int r = 0; r < {m}; ++r) c += u[r] * (par[0] * u[r]);
    return c;
}}
'''


def params_source(n, m, row):
    """The same cost with ONE row, the same at every step, folded into the parameters: par = [u_std, z (NZ <= 7), q (NZ <= 7)]
    (what a cost without a table can hold; tools/user_cost_bench.py measures the table against it)."""
    nz = len(row) // 2
    assert 1 + 2 * nz <= 16
    return f'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {{
    S c = S(0);
    for (int j = 0; j < {nz}; ++j) {{
        const S d = x[j] - par[1 + j];
        c += d * (par[{1 + nz} + j] * d);
    }}
    for (int r = 0; r < {m}; ++r) c += u[r] * (par[0] * u[r]);
    return c;
}}
'''


def generic_source(n, m, W, table):
    """A cost at any (n, m) whose W constants c_k come from `row` (table=True) or from `par`, every one of them used: the same
    arithmetic either way, so a table whose every row repeats the constants must give the bits of the `par` form."""
    c = "row" if table else "par"
    sig = "const P *par, const P *row, int t, int N" if table else "const P *par, int t, int N"
    return f'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, {sig}) {{
    S c = S(0);
    for (int k = 0; k < {W}; ++k) {{
        const S d = x[k % {n}] - {c}[k];
        c += d * ({c}[(k + 1) % {W}] * d);
    }}
    for (int r = 0; r < {m}; ++r) c += u[r] * ({c}[{W} - 1] * u[r]);
    return c;
}}
'''


def generic_consts(W):
    return 0.3 + 0.1 * np.arange(W)


def make_table(rng, N, n, B=None, terminal=20.0, shared_weights=False):
    """[N, W] (B None) or [B, N, W]: every row of every trajectory distinct, the last row's weights `terminal` times heavier;
    shared_weights: the trajectories differ in z_t only (iSLS.set_cost_variables takes per-trajectory via points with one Q table)"""
    nz = nz_of(n)
    lead = (N,) if B is None else (B, N)
    z = rng.uniform(-1.0, 1.0, size=lead + (nz,))
    q = rng.uniform(0.5, 1.5, size=lead + (nz,))
    if shared_weights and B is not None:
        q = np.broadcast_to(q[0], q.shape).copy()
    q[..., -1, :] *= terminal
    return np.concatenate([z, q], axis=-1)


def via_tables(table, n):
    """(zs [., N, n], Qs [., N, n, n], seq = arange(N)) of the built-in via-point cost the table restates"""
    table = np.asarray(table, dtype=np.float64)
    nz, N = nz_of(n), table.shape[-2]
    zs, Qs = np.zeros(table.shape[:-1] + (n,)), np.zeros(table.shape[:-1] + (n, n))
    zs[..., :nz] = table[..., :nz]
    idx = np.arange(nz)
    Qs[..., idx, idx] = table[..., nz:]
    if shared_weights_of(table):
        Qs = Qs[0]
    return zs, Qs, np.arange(N, dtype=np.int32)


def shared_weights_of(table):
    """True for a [B, N, W] table whose weights are the same for every trajectory"""
    nz = table.shape[-1] // 2
    return table.ndim == 3 and table.shape[0] > 1 and bool((table[..., nz:] == table[:1, :, nz:]).all())


def tracking_numpy(x, u, table, u_std):
    """(cost [...], cs [..., N, n+m], Cs [..., N, n+m, n+m]); x [..., N, n], u [..., N, m], table [N, W] or [B, N, W] with B the
    leading axis of x"""
    x, u, table = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64), np.asarray(table, dtype=np.float64)
    n, m = x.shape[-1], u.shape[-1]
    nz, K = nz_of(n), n + m
    if table.ndim == 3 and x.ndim > 3:                          # [B, L, N, n] against [B, N, W]
        table = table.reshape((table.shape[0],) + (1,) * (x.ndim - 3) + table.shape[1:])
    z, q = table[..., :nz], table[..., nz:]
    d = x[..., :nz] - z
    val = (q * d * d).sum(-1) + u_std * (u * u).sum(-1)
    g, H = np.zeros(x.shape[:-1] + (K,)), np.zeros(x.shape[:-1] + (K, K))
    g[..., :nz] = 2 * q * d
    g[..., n:] = 2 * u_std * u
    idx = np.arange(nz)
    H[..., idx, idx] = np.broadcast_to(2 * q, d.shape)
    iu = n + np.arange(m)
    H[..., iu, iu] = 2 * u_std
    return val.sum(-1), g, H
