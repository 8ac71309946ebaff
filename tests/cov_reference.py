"""numpy restatement of isls_cov_closed_loop_* (include/isls_hip.h; the summation order is written out in csrc/covariance.hip):
mean and covariance of the linearised closed loop of a batch of stage-local controllers.  Every sum runs over its inner index
ascending, one product added at a time (numpy has no fused multiply-add: the kernel agrees to rounding, not to the bit).  The whole
recursion runs in `dtype` (float64, or float32 to see what that format alone costs); the probabilities use math.erfc."""
import math

import numpy as np


def _full(x, shape, dtype, fill=0.0):
    return np.full(shape, fill, dtype=dtype) if x is None else np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dtype), shape))


def prob_outside(mu, var, lo, hi):
    """Gaussian probability of lying outside [lo, hi] (arrays of one shape; +-inf = free side); var <= 0: the indicator of the mean
    lying outside"""
    p = np.zeros(mu.shape, dtype=mu.dtype)
    for idx in np.ndindex(mu.shape):
        m_, v, l, h = float(mu[idx]), float(var[idx]), float(lo[idx]), float(hi[idx])
        sd = math.sqrt(v) if v > 0.0 else 0.0
        if sd > 0.0:
            den = sd * 1.4142135623730951
            p[idx] = 0.5 * math.erfc((m_ - l) / den) + 0.5 * math.erfc((h - m_) / den)
        else:
            p[idx] = 1.0 if (m_ < l or m_ > h) else 0.0
    return p


def closed_loop(A, B, K, S0, k=None, W=None, xhat=None, uhat=None, dx0=None, u_bounds=None, x_bounds=None, P=None, dtype=np.float64):
    """A [.,.,n,n], B [.,.,n,m] (anything that broadcasts to [P,N,..]), K [P,N,m,n] / [N,m,n], S0 [P,n,n] / [n,n], k, W ([n,n],
    [P,1,n,n], [P,N,n,n]), xhat, uhat, dx0 or None (zero), bounds = (lo, hi) that broadcast to [P,N,d] or None.
    Returns a dict of x_mean, u_mean, x_var, u_var, x_cov, u_cov, p_x, p_u (p: None without bounds)."""
    K = np.asarray(K)
    N, m, n = K.shape[-3:]
    if P is None:
        P = K.shape[0] if K.ndim == 4 else 1
    f = lambda x, *s: _full(x, (P,) + s, dtype)                                          # noqa: E731
    A, B, K, W = f(A, N, n, n), f(B, N, n, m), f(K, N, m, n), f(W, N, n, n)
    k, xhat, uhat, d = f(k, N, m), f(xhat, N, n), f(uhat, N, m), f(dx0, n)
    S0 = f(S0, n, n)
    half = dtype(0.5)
    Sig = half * (S0 + np.swapaxes(S0, -1, -2))
    out = dict(x_mean=np.zeros((P, N, n), dtype), u_mean=np.zeros((P, N, m), dtype), x_cov=np.zeros((P, N, n, n), dtype),
               u_cov=np.zeros((P, N, m, m), dtype))
    for t in range(N):
        At, Bt, Kt, kt = A[:, t], B[:, t], K[:, t], k[:, t]
        out["x_cov"][:, t] = Sig
        out["x_mean"][:, t] = xhat[:, t] + d
        Phi = At.copy()
        for r in range(m):
            Phi = Phi + Bt[:, :, r, None] * Kt[:, None, r, :]
        M, KS = np.zeros((P, n, n), dtype), np.zeros((P, m, n), dtype)
        for c in range(n):
            M = M + Phi[:, :, c, None] * Sig[:, None, c, :]
            KS = KS + Kt[:, :, c, None] * Sig[:, None, c, :]
        SU = np.zeros((P, m, m), dtype)
        for j in range(n):
            SU = SU + KS[:, :, j, None] * Kt[:, None, :, j]
        out["u_cov"][:, t] = half * (SU + np.swapaxes(SU, -1, -2))
        a = kt.copy()
        dn = np.zeros((P, n), dtype)
        for j in range(n):
            a = a + Kt[:, :, j] * d[:, None, j]
            dn = dn + Phi[:, :, j] * d[:, None, j]
        for r in range(m):
            dn = dn + Bt[:, :, r] * kt[:, None, r]
        out["u_mean"][:, t] = uhat[:, t] + a
        S = np.zeros((P, n, n), dtype)
        for c in range(n):
            S = S + M[:, :, c, None] * Phi[:, None, :, c]
        S = S + W[:, t]
        Sig, d = half * (S + np.swapaxes(S, -1, -2)), dn
    out["x_var"] = np.ascontiguousarray(np.diagonal(out["x_cov"], axis1=-2, axis2=-1))
    out["u_var"] = np.ascontiguousarray(np.diagonal(out["u_cov"], axis1=-2, axis2=-1))
    for name, bounds, mean, var, dd in (("p_u", u_bounds, "u_mean", "u_var", m), ("p_x", x_bounds, "x_mean", "x_var", n)):
        out[name] = None
        if bounds is not None and (bounds[0] is not None or bounds[1] is not None):
            lo = _full(bounds[0], (P, N, dd), dtype, -np.inf)
            hi = _full(bounds[1], (P, N, dd), dtype, np.inf)
            out[name] = prob_outside(out[mean], out[var], lo, hi)
    return out
