"""Sources of user costs (isls.costs.Custom) shared by the user-cost tests and tools/user_cost_bench.py: the pseudo-Huber cost and
a via-point cost restated as `stage` functions, and a coupled cost (x-u cross terms, an off-diagonal state Hessian, a terminal
term) with its numpy value, gradient and Hessian written out by hand."""
import ctypes
import itertools

import numpy as np

_FRESH = itertools.count()


def fresh(source):
    """`source` with a trailing comment no other source of this process has: the same code under an id of its own (the binding
    registers one text once)"""
    return source + f"// registration {next(_FRESH)} of this process\n"


def same_id_pair(model_args, cost_args):
    """(models.Custom, costs.Custom) from (x_dim, u_dim, params, source) each, registered anew so that the model's id and the
    cost's id are the same number.  The two kinds count their ids independently, and a source gets its id even when its compile
    fails: the kind that is behind is padded with sources that stop the compiler at their first line."""
    from isls import _capi as capi
    from isls import costs, models
    lib = capi.load_hip_library()

    def pad(kind):
        uid = ctypes.c_int32(-1)
        rc = getattr(lib, f"isls_user_{kind}_create")(b'#include "no_such_header.hpp"\n', 2, 1, 0, ctypes.byref(uid))
        assert rc == capi.ERR_COMPILE and uid.value >= 1024
        return uid.value
    last = {kind: pad(kind) for kind in ("model", "cost")}
    behind = min(last, key=last.get)
    while last[behind] < max(last.values()):
        last[behind] = pad(behind)
    mdl = models.Custom(*model_args[:3], fresh(model_args[3]))
    cst = costs.Custom(*cost_args[:3], fresh(cost_args[3]))
    assert mdl.model_id == cst.cost_model == last[behind] + 1
    return mdl, cst


def _lit(v):
    return "{" + ", ".join(f"P({float(x)!r})" for x in v) + "}"


def phuber_source(n, m, px, pf):
    """costs.PseudoHuber as a stage cost; par = [cu (m), cx (n), cf (n)], the widths px, pf are constants of the source (the
    five vectors together would be m + 4 n > 16 parameters)."""
    return f'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {{
    const P px[{n}] = {_lit(px)}, pf[{n}] = {_lit(pf)};
    const P *cu = par, *cx = par + {m}, *cf = par + {m + n};
    S c = S(0);
    for (int j = 0; j < {n}; ++j) c += cx[j] * (sqrt(x[j] * x[j] + px[j] * px[j]) - px[j]);
    if (t == N - 1)
        for (int j = 0; j < {n}; ++j) c += cf[j] * (sqrt(x[j] * x[j] + pf[j] * pf[j]) - pf[j]);
    for (int r = 0; r < {m}; ++r) c += cu[r] * (u[r] * u[r]);
    return c;
}}
'''


def phuber_params(cu, cx, cf):
    return np.concatenate([np.ravel(cu), np.ravel(cx), np.ravel(cf)]).astype(np.float64)


def via_arm_source(q1, qf, u_std, t1):
    """A via-point cost on the 3R arm's end effector (state [q, qd, ee]): weight q1 on |ee - z1|^2 at step t1, qf on |ee - zf|^2
    at the last step, u_std |u|^2 at every step; par = [z1x, z1y, zfx, zfy] (the targets: what varies per trajectory), the
    weights and t1 are constants of the source.  (Every parameter is a register of the line search for the whole horizon.)"""
    return f'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {{
    S c = S(0);
    if (t == {int(t1)}) c += P({float(q1)!r}) * ((x[6] - par[0]) * (x[6] - par[0]) + (x[7] - par[1]) * (x[7] - par[1]));
    if (t == N - 1) c += P({float(qf)!r}) * ((x[6] - par[2]) * (x[6] - par[2]) + (x[7] - par[3]) * (x[7] - par[3]));
    for (int r = 0; r < 3; ++r) c += u[r] * (P({float(u_std)!r}) * u[r]);
    return c;
}}
'''


VIA_ARM_W = dict(q1=50.0, qf=100.0, u_std=1e-2, t1=17)
VIA_ARM_PAR = np.array([1.2, 1.1, 0.5, 1.9])


def via_arm_tables(par, N, q1, qf, u_std, t1):
    """(zs [3,9], Qs [3,9,9], seq [N], u_std) of the built-in via-point cost that via_arm_source restates"""
    zs, Qs = np.zeros((3, 9)), np.zeros((3, 9, 9))
    zs[1, 6:8], zs[2, 6:8] = par[0:2], par[2:4]
    Qs[1, 6, 6] = Qs[1, 7, 7] = q1
    Qs[2, 6, 6] = Qs[2, 7, 7] = qf
    seq = np.zeros(N, dtype=np.int32)
    seq[int(t1)], seq[N - 1] = 1, 2
    return zs, Qs, seq, float(u_std)


def coupled_source(n, m):
    """par = [w_u, w_c, w_o, cx, cy, s, w_x, w_f, gx, gy]:
    w_u |u|^2 + w_c sum_r (x_{n-1-r} u_r)^2 + w_o exp(-|p - c|^2 / s^2) + w_x |x - g|^2  (+ w_f |x - g|^2 at the last step),
    p = x[0:2], g = [gx, gy, 0, ...]"""
    return f'''
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {{
    const P w_u = par[0], w_c = par[1], w_o = par[2], s = par[5], w_x = par[6], w_f = par[7];
    S c = S(0), d2 = S(0);
    for (int r = 0; r < {m}; ++r) {{
        const S a = x[{n} - 1 - r] * u[r];
        c += w_u * (u[r] * u[r]) + w_c * (a * a);
    }}
    const S dx = x[0] - par[3], dy = x[1] - par[4];
    c += w_o * exp(-(dx * dx + dy * dy) / (s * s));
    for (int i = 0; i < {n}; ++i) {{
        const S e = i < 2 ? x[i] - par[8 + (i < 2 ? i : 0)] : x[i];
        d2 += e * e;
    }}
    c += w_x * d2;
    if (t == N - 1) c += w_f * d2;
    return c;
}}
'''


COUPLED_PAR = np.array([0.05, 0.01, 0.3, 0.4, -0.3, 1.0, 0.5, 4.0, 1.0, 0.5])


def _par_rows(par, lead):
    """par [P] or [B, P] -> columns broadcastable against arrays [..., N] (a batch's rows are its leading axis)"""
    par = np.asarray(par, dtype=np.float64)
    if par.ndim == 1:
        return [par[k] for k in range(par.shape[0])]
    return [par[:, k].reshape((par.shape[0],) + (1,) * (len(lead) - 1)) for k in range(par.shape[1])]


def coupled_numpy(x, u, par=COUPLED_PAR):
    """(cost [...], cs [..., N, n+m], Cs [..., N, n+m, n+m]) of coupled_source on numpy, derivatives written out by hand.
    x [..., N, n], u [..., N, m]; par [P], or [B, P] with B the leading axis of x."""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    n, m, N = x.shape[-1], u.shape[-1], x.shape[-2]
    lead = x.shape[:-1]                                        # [..., N]
    w_u, w_c, w_o, cx, cy, s, w_x, w_f, gx, gy = _par_rows(par, lead)
    K = n + m
    g, H = np.zeros(lead + (K,)), np.zeros(lead + (K, K))
    val = np.zeros(lead)
    for r in range(m):
        i, ur, xi = n - 1 - r, u[..., r], x[..., n - 1 - r]
        val += w_u * ur ** 2 + w_c * (xi * ur) ** 2
        g[..., n + r] += 2 * w_u * ur + 2 * w_c * xi ** 2 * ur
        g[..., i] += 2 * w_c * xi * ur ** 2
        H[..., n + r, n + r] += 2 * w_u + 2 * w_c * xi ** 2
        H[..., i, i] += 2 * w_c * ur ** 2
        H[..., n + r, i] += 4 * w_c * xi * ur
        H[..., i, n + r] += 4 * w_c * xi * ur
    d = np.stack([x[..., 0] - cx, x[..., 1] - cy], axis=-1)
    E = w_o * np.exp(-(d ** 2).sum(-1) / s ** 2)
    val += E
    g[..., :2] += (E * (-2 / s ** 2))[..., None] * d
    s2 = np.asarray(s, dtype=np.float64)[..., None, None] ** 2
    H[..., :2, :2] += E[..., None, None] * (4 * d[..., :, None] * d[..., None, :] / s2 ** 2 - 2 / s2 * np.eye(2))
    e = x.copy()
    e[..., 0] -= gx
    e[..., 1] -= gy
    w = w_x + np.where(np.arange(N) == N - 1, 1.0, 0.0) * w_f   # [..., N]
    w = np.broadcast_to(w, lead)
    val += w * (e ** 2).sum(-1)
    g[..., :n] += 2 * w[..., None] * e
    H[..., np.arange(n), np.arange(n)] += 2 * w[..., None]
    return val.sum(-1), g, H
