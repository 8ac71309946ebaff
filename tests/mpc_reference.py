"""numpy restatement of one receding-horizon control step (isls_mpc_step_*, csrc/mpc.hpp), written from the contract in
include/isls_hip.h -- what tests/test_mpc_*.py compare the library with.  `f(x [B,n], u [B,m], par [B,P]) -> [B,n]` is a
forward model on numpy (model_f: the numpy __call__ of isls.models, or a twin of tests/user_models.py)."""
import numpy as np

from mc_reference import normals


def shift_hold(a):
    """a~[t] = a[t+1] for t < N-1, a~[N-1] = a[N-1] along axis -2 ... of an array [..., N, d] (axis 1 of [B, N, ...])"""
    a = np.asarray(a)
    out = a.copy()
    out[:, :-1] = a[:, 1:]
    return out


def shift_naive(a):
    """the same by np.roll and a fixed last row"""
    a = np.asarray(a)
    out = np.roll(a, -1, axis=1)
    out[:, -1] = a[:, -1]
    return out


def model_f(model):
    """f(x, u, par) of an isls.models descriptor class through its numpy __call__, one parameter row per trajectory"""
    def f(x, u, par):
        par = np.broadcast_to(par, (x.shape[0], par.shape[-1]))
        return np.stack([np.asarray(model(par[b])(x[b], u[b]), dtype=np.float64).reshape(-1) for b in range(x.shape[0])])
    return f


def mpc_step(f, par, xhat, uhat, K=None, zx=None, zu=None, plant_par=None, tab=None, tab_next=None, u_lo=None, u_hi=None,
             w=None, noise_std=None, seed=0, problem0=0, step=0, dtype=np.float64):
    """One control step in fp64 on copies; returns a dict with the new xhat, uhat, K, zx, zu, tab and x_meas, u_app, x_next.
    dtype: the precision of the entry point compared with -- std * z is rounded once to it, as the library does."""
    xhat, uhat = np.array(xhat, dtype=np.float64), np.array(uhat, dtype=np.float64)
    B, N, n = xhat.shape
    par = np.asarray(par, dtype=np.float64)
    plant_par = par if plant_par is None else np.asarray(plant_par, dtype=np.float64)
    x_m, u_a = xhat[:, 0].copy(), uhat[:, 0].copy()
    if u_lo is not None:
        u_a = np.maximum(u_a, u_lo)
    if u_hi is not None:
        u_a = np.minimum(u_a, u_hi)
    x_next = f(x_m, u_a, plant_par)
    if w is not None:
        x_next = x_next + np.asarray(w, dtype=np.float64)
    elif noise_std is not None:
        z = normals(seed, problem0 + np.arange(B), 0, step, n)
        x_next = x_next + (np.asarray(noise_std, dtype=np.float64) * z).astype(dtype).astype(np.float64)
    xs, us = shift_hold(xhat), shift_hold(uhat)
    out = dict(x_meas=x_m, u_app=u_a, x_next=x_next, K=None if K is None else shift_hold(K),
               zx=None if zx is None else shift_hold(zx), zu=None if zu is None else shift_hold(zu), tab=None)
    if tab is not None:
        t = np.asarray(tab)
        nt = shift_hold(t[None] if t.ndim == 2 else t)
        if tab_next is not None:
            nt[:, -1] = tab_next
        out["tab"] = nt[0] if t.ndim == 2 else nt
    x = x_next.copy()
    for t in range(N):
        u = us[:, t].copy()
        if K is not None:
            dx = x - xs[:, t]
            acc = np.zeros_like(u)
            for j in range(n):                                  # j ascending
                acc = acc + out["K"][:, t, :, j] * dx[:, j:j + 1]
            u = acc + us[:, t]
        xhat[:, t], uhat[:, t] = x, u
        if t < N - 1:
            x = f(x, u, par)
    out["xhat"], out["uhat"] = xhat, uhat
    return out
