"""numpy restatement of the Monte-Carlo closed loop's generator and loop (csrc/philox.hpp, csrc/monte_carlo.hpp), written from
the contract in include/isls_hip.h -- what tests/test_monte_carlo_*.py compare the library with."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint32 arrays of counters (broadcast together) and an integer key -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & 0xffffffff for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xffffffff),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xffffffff)]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [v.astype(np.uint32) for v in c]


def normals(seed, problem, sample, step, n):
    """standard normals [..., n] of the counters (sample, problem, step, coordinate / 4): Box-Muller pairs in fp64"""
    problem, sample, step = np.broadcast_arrays(np.asarray(problem), np.asarray(sample), np.asarray(step))
    out = np.zeros(problem.shape + (4 * ((n + 3) // 4),))
    for q in range((n + 3) // 4):
        r = philox4x32_10(sample, problem, step, np.full(problem.shape, q), seed & 0xffffffff, seed >> 32)
        u = [(v.astype(np.float64) + 0.5) * 2.0 ** -32 for v in r]
        for h in range(2):
            rad, ang = np.sqrt(-2.0 * np.log(u[2 * h])), 2.0 * np.pi * u[2 * h + 1]
            out[..., 4 * q + 2 * h], out[..., 4 * q + 2 * h + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out[..., :n]


def dense_loop(f, K, k, x0s, w=None, xhat=None, uhat=None):
    """x_{i+1} = f(x_i, u_i) + w_i with u_i = (K [dx_0 .. dx_i, 0 ..] + k)_i + uhat_i for the samples x0s [M,n] (numpy, fp64)"""
    M, n = x0s.shape
    Nm, Nn = K.shape
    N, m = Nn // n, Nm // (Nn // n)
    xhat = np.zeros((N, n)) if xhat is None else xhat
    uhat = np.zeros((N, m)) if uhat is None else uhat
    x_log, u_log = np.zeros((M, N, n)), np.zeros((M, N, m))
    x = x0s.copy()
    for i in range(N):
        x_log[:, i] = x
        dx = np.zeros((M, Nn))
        dx[:, :(i + 1) * n] = (x_log[:, :i + 1] - xhat[None, :i + 1]).reshape(M, -1)
        u_log[:, i] = (dx @ K.T + k)[:, i * m:(i + 1) * m] + uhat[i]
        x = f(x, u_log[:, i]) + (0.0 if w is None else w[:, i])
    return x_log, u_log
