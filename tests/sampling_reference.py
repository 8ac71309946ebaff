"""numpy restatement of one sampling round about a batch of nominals (csrc/sampling.hpp), written from the contract in
include/isls_hip.h -- what tests/test_sampling_*.py compare the library with.  Draws: mc_reference.normals; models: the scalar
restatements of tests/user_models.py evaluated on arrays; costs: the via-point sum, user_costs.coupled_numpy (the cost with the
obstacle bump) and table_costs.tracking_numpy."""
import numpy as np

import table_costs
import user_costs
import user_models
from mc_reference import normals


# ---- models: step(x [..., n], u [..., m], par [P] or [B, P] with B the leading axis of x) --------------------------------------
def _cols(a):
    return [a[..., j] for j in range(a.shape[-1])]


def _par_cols(par, x):
    par = np.asarray(par)
    if par.ndim == 1:
        return [par[k] for k in range(par.shape[0])]
    return [par[:, k].reshape((par.shape[0],) + (1,) * (x.ndim - 2)) for k in range(par.shape[1])]


def _di_f(x, u, par, M):
    a, b0, b1 = par
    d = len(u)
    return [(x[i] + a * x[d + i]) + b0 * u[i] for i in range(d)] + [x[d + i] + b1 * u[i] for i in range(d)]


def _sqrt_f(x, u, par, M):
    """SQRT_MODEL below: the square root of a state that the controls can push below zero"""
    return [x[0] + par[0] * u[0], M.sqrt(x[0]) + x[1]]


# (2, 1): x0 is driven by u and x1 integrates sqrt(x0): a sample whose x0 falls below zero goes NaN
SQRT_MODEL = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    xn[0] = x[0] + par[0] * u[0];
    xn[1] = sqrt(x[0]) + x[1];
}
'''


def _tassa_f(x, u, par, M):
    """ISLS_MODEL_TASSA (include/isls_hip.h): f = dt v, b = f cos w + d - sqrt(d^2 - (f sin w)^2)"""
    dt, d = par
    f = dt * x[3]
    sw = M.sin(u[0]) * f
    b = (f * M.cos(u[0]) + d) - M.sqrt(d * d - sw * sw)
    return [x[0] + b * M.cos(x[2]), x[1] + b * M.sin(x[2]), x[2] + M.arcsin(sw / d), x[3] + u[1] * dt]


MODELS = {"tassa": _tassa_f, "di": _di_f, "car": user_models.car_f, "arm": user_models.arm_f, "quad": user_models.quad_f, "sqrt": _sqrt_f}


def model(name):
    f = MODELS[name]

    def step(x, u, par):
        with np.errstate(invalid="ignore"):
            out = f(_cols(x), _cols(u), _par_cols(par, x), np)
        return np.stack([np.broadcast_to(o, x.shape[:-1]) for o in out], axis=-1).astype(x.dtype)
    return step


def rollout(step, x0, u, par):
    """x [..., N, n] of the open-loop rollout of u [..., N, m] from x0 [..., n]"""
    N = u.shape[-2]
    xs = [x0]
    for t in range(N - 1):
        xs.append(step(xs[-1], u[..., t, :], par))
    return np.stack(xs, axis=-2)


# ---- costs: cost(x [B, ..., N, n], u [B, ..., N, m]) -> [B, ...] ------------------------------------------------------------------
def via_cost(zs, Qs, seq, u_std):
    """sum_t (x_t - z_t)' Q_t (x_t - z_t) + u_std |u_t|^2 (no 1/2); zs [nvia, n] or [B, nvia, n], Qs likewise"""
    def cost(x, u):
        z, Q = np.asarray(zs, dtype=x.dtype), np.asarray(Qs, dtype=x.dtype)
        zt, Qt = z[..., seq, :], Q[..., seq, :, :]                 # [(B,) N, n], [(B,) N, n, n]
        if z.ndim == 3:
            zt = zt.reshape((zt.shape[0],) + (1,) * (x.ndim - 3) + zt.shape[1:])
        if Q.ndim == 4:
            Qt = Qt.reshape((Qt.shape[0],) + (1,) * (x.ndim - 3) + Qt.shape[1:])
        d = x - zt
        return np.einsum("...ti,...tij,...tj->...", d, np.broadcast_to(Qt, d.shape + (d.shape[-1],)), d) + \
            x.dtype.type(u_std) * np.sum(u * u, axis=(-1, -2))
    return cost


def phuber_cost(cu, cx, px, cf, pf):
    """ISLS_COST_PHUBER (include/isls_hip.h): sum_t [cu . u_t^2 + cx . ph(x_t, px)] + cf . ph(x_{N-1}, pf), ph(x, p) = sqrt(x^2 + p^2) - p"""
    def cost(x, u):
        cu_, cx_, px_, cf_, pf_ = (np.asarray(v, dtype=x.dtype) for v in (cu, cx, px, cf, pf))
        ph = lambda v, p: np.sqrt(v * v + p * p) - p             # noqa: E731
        return np.sum(cu_ * u * u, axis=(-1, -2)) + np.sum(cx_ * ph(x, px_), axis=(-1, -2)) + np.sum(cf_ * ph(x[..., -1, :], pf_), axis=-1)
    return cost


def coupled_cost(par):
    return lambda x, u: user_costs.coupled_numpy(x, u, par)[0]


def tracking_cost(table, u_std):
    return lambda x, u: table_costs.tracking_numpy(x, u, table, u_std)[0]


def sum_cost(stage):
    """a cost given as stage(x [..., n], u [..., m], t, N) -> [...]"""
    def cost(x, u):
        N = x.shape[-2]
        return sum(stage(x[..., t, :], u[..., t, :], t, N) for t in range(N))
    return cost


# ---- the round -------------------------------------------------------------------------------------------------------------------
def draws(seed, B, S, N, m, sigma, problem0=0, dtype=np.float64):
    """eps [B, S, N, m]: sample 0 zero, else sigma o normals(seed, problem, sample, step); the product in fp64, rounded once"""
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B, m))
    b, s, t = np.meshgrid(problem0 + np.arange(B), np.arange(S), np.arange(N), indexing="ij")
    eps = sigma[:, None, None, :] * normals(int(seed), b, s, t, m)
    eps[:, 0] = 0.0
    return eps.astype(dtype)


def sample_round(step, par, cost, xhat, uhat, sigma, seed, S, temperature=1.0, clip_u=None, dtype=np.float64):
    """Steps 1 to 5 for every problem; xhat [B, N, n], uhat [B, N, m].  Returns a dict: costs [B, S], u [B, S, N, m], xhat, uhat
    (the new nominal), cost_before, cost_after, cost_best, ess, took_best [B], and the two margins the device comparison needs:
    lead (the arg-min's lead over the runner-up) and decide (|c_new - Smin|), both relative to |Smin|."""
    B, N, m = uhat.shape
    xhat, uhat, par = np.asarray(xhat, dtype=dtype), np.asarray(uhat, dtype=dtype), np.asarray(par, dtype=dtype)
    eps = draws(seed, B, S, N, m, sigma, dtype=dtype)
    u = uhat[:, None] + eps
    if clip_u is not None:
        u = np.minimum(np.maximum(u, np.asarray(clip_u[0], dtype=dtype)), np.asarray(clip_u[1], dtype=dtype))
    e = u - uhat[:, None]
    x = rollout(step, np.broadcast_to(xhat[:, None, 0], (B, S, xhat.shape[-1])), u, par)
    with np.errstate(invalid="ignore", over="ignore"):
        costs = np.asarray(cost(x, u), dtype=dtype)
    costs = np.where(np.isnan(costs), np.inf, costs)
    smin = np.argmin(costs, axis=1)                            # the first index of the minimum
    Smin = costs[np.arange(B), smin]
    tiny = np.finfo(dtype).tiny
    with np.errstate(over="ignore"):
        w = np.exp(-(costs - Smin[:, None]) / (dtype(temperature) * np.maximum(Smin, tiny))[:, None])
    w = w / w.sum(axis=1, keepdims=True)
    u_new = uhat + np.einsum("bs,bstr->btr", w, e)
    x_new = rollout(step, xhat[:, 0], u_new, par)
    with np.errstate(invalid="ignore", over="ignore"):
        c_new = np.asarray(cost(x_new, u_new), dtype=dtype)
    took = ~(c_new < Smin)
    idx = np.arange(B)
    uh = np.where(took[:, None, None], u[idx, smin], u_new)
    xh = np.where(took[:, None, None], x[idx, smin], x_new)
    runner = np.sort(costs, axis=1)[:, 1] if S > 1 else np.full(B, np.inf)
    scale = np.maximum(np.abs(Smin), tiny)
    return dict(costs=costs, u=u, x=x, xhat=xh, uhat=uh, cost_before=costs[:, 0], cost_after=np.where(took, Smin, c_new), cost_best=Smin,
                ess=1.0 / np.sum(w * w, axis=1), took_best=took, lead=(runner - Smin) / scale, decide=np.abs(c_new - Smin) / scale)


def sample_nominal(step, par, cost, xhat, uhat, sigma, seed=0, samples=1024, temperature=1.0, rounds=1, clip_u=None, dtype=np.float64):
    """iSLS.sample_nominal: `rounds` rounds, round r with seed + r; the last round's dict with cost_before of the first and the
    per-round columns cost_best_sample, took_best, ess [B, rounds], lead, decide [B, rounds]"""
    cols = {k: [] for k in ("cost_best", "took_best", "ess", "lead", "decide")}
    first = None
    for r in range(rounds):
        out = sample_round(step, par, cost, xhat, uhat, sigma, seed + r, samples, temperature, clip_u, dtype)
        xhat, uhat = out["xhat"], out["uhat"]
        first = out["cost_before"] if first is None else first
        for k in cols:
            cols[k].append(out[k])
    out.update(cost_before=first, cost_best_sample=np.stack(cols["cost_best"], 1), took_best=np.stack(cols["took_best"], 1),
               ess=np.stack(cols["ess"], 1), lead=np.stack(cols["lead"], 1), decide=np.stack(cols["decide"], 1))
    return out
