"""numpy restatement of one CLOSED-LOOP sampling round about a batch of nominals (isls_sample_nominal_fb_*, csrc/sampling.hpp),
written from the contract in include/isls_hip.h -- what tests/test_sampling_feedback_*.py compare the library with.  Draws, models,
costs and the open-loop rollout are those of tests/sampling_reference.py."""
import numpy as np

from sampling_reference import draws, rollout  # noqa: F401  (rollout: re-exported for the tests)


def _clip(u, clip_u, dtype):
    if clip_u is None:
        return u
    return np.minimum(np.maximum(u, np.asarray(clip_u[0], dtype=dtype)), np.asarray(clip_u[1], dtype=dtype))


def closed_loop(step, par, xa, base, G, eps, clip_u, base_first, dtype):
    """x [B, S, N, n], u [B, S, N, m] of S closed loops per problem from xa[:, 0].  xa [B, N, n]: the anchors; G [B, N, m, n];
    base [B, N, m] or [B, S, N, m] and eps likewise (or None).  base_first: u_t = clip((base_t + G_t (x_t - xa_t)) + eps_t), the
    order of the samples; else u_t = clip(base_t + G_t (x_t - xa_t)) with no noise (the candidate: base = ua + d)."""
    B, N, n = xa.shape
    lead = base.shape[:-2]
    x = np.broadcast_to(xa[:, 0].reshape((B,) + (1,) * (len(lead) - 1) + (n,)), lead + (n,)).astype(dtype)
    ex = lambda a, t: a[:, t].reshape((B,) + (1,) * (len(lead) - 1) + a.shape[2:])     # noqa: E731
    xs, us = [], []
    for t in range(N):
        fb = np.einsum("...rj,...j->...r", ex(G, t), x - ex(xa, t))
        v = base[..., t, :] + fb
        if base_first and eps is not None:
            v = v + eps[..., t, :]
        u = _clip(v, clip_u, dtype)
        xs.append(x), us.append(u)
        if t < N - 1:
            x = step(x, u, par)
    return np.stack(xs, axis=-2), np.stack(us, axis=-2)


def sample_round(step, par, cost, xhat, uhat, G, sigma, seed, S, temperature=1.0, clip_u=None, dtype=np.float64):
    """Steps 1 to 5 of isls_sample_nominal_fb_* for every problem; xhat [B, N, n], uhat [B, N, m], G [N, m, n] or [B, N, m, n].
    Returns the dict of sampling_reference.sample_round: costs [B, S], u, x of the samples, xhat, uhat (the new nominal),
    cost_before, cost_after, cost_best, ess, took_best [B], and the margins lead and decide."""
    B, N, m = uhat.shape
    n = xhat.shape[-1]
    xhat, uhat, par = np.asarray(xhat, dtype=dtype), np.asarray(uhat, dtype=dtype), np.asarray(par, dtype=dtype)
    G = np.broadcast_to(np.asarray(G, dtype=dtype), (B, N, m, n))
    eps = draws(seed, B, S, N, m, sigma, dtype=dtype)
    x, u = closed_loop(step, par, xhat, np.broadcast_to(uhat[:, None], (B, S, N, m)), G, eps, clip_u, True, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        costs = np.asarray(cost(x, u), dtype=dtype)
    costs = np.where(np.isnan(costs), np.inf, costs)
    smin = np.argmin(costs, axis=1)                            # the first index of the minimum
    Smin = costs[np.arange(B), smin]
    tiny = np.finfo(dtype).tiny
    with np.errstate(over="ignore"):
        w = np.exp(-(costs - Smin[:, None]) / (dtype(temperature) * np.maximum(Smin, tiny))[:, None])
    w = w / w.sum(axis=1, keepdims=True)
    d = np.einsum("bs,bstr->btr", w, eps)                      # the DRAWN noise, not the realised deviation
    x_new, u_new = closed_loop(step, par, xhat, uhat + d, G, None, clip_u, False, dtype)
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


def sample_nominal(step, par, cost, xhat, uhat, G, sigma, seed=0, samples=1024, temperature=1.0, rounds=1, clip_u=None, dtype=np.float64):
    """iSLS.sample_nominal(feedback=G): `rounds` rounds with the same gains, round r with seed + r; the last round's dict with
    cost_before of the first and the per-round columns of sampling_reference.sample_nominal"""
    cols = {k: [] for k in ("cost_best", "took_best", "ess", "lead", "decide")}
    first = None
    for r in range(rounds):
        out = sample_round(step, par, cost, xhat, uhat, G, sigma, seed + r, samples, temperature, clip_u, dtype)
        xhat, uhat = out["xhat"], out["uhat"]
        first = out["cost_before"] if first is None else first
        for k in cols:
            cols[k].append(out[k])
    out.update(cost_before=first, cost_best_sample=np.stack(cols["cost_best"], 1), took_best=np.stack(cols["took_best"], 1),
               ess=np.stack(cols["ess"], 1), lead=np.stack(cols["lead"], 1), decide=np.stack(cols["decide"], 1))
    return out
