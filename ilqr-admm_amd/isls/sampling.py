"""Sampling warm start of a batch of nominals on the device (isls_sample_nominal_*, csrc/sampling.hpp).

iLQR and iLQR-ADMM refine the nominal they are handed and end in the nearest local minimum; with a non-convex cost (an obstacle
bump, a keep-out set) a straight-line guess on the wrong side of the obstacle stays there.  One round of model-predictive path
integral control about the nominal -- `samples` open-loop rollouts per problem with controls drawn about uhat, weighted by
exp(-cost) -- moves it, and never raises its cost: where the weighted mean does not beat the best sample, the best sample is
taken.  `iSLS.sample_nominal` is a thin front end of `run`.

Open-loop noise accumulates: on an unstable or strongly nonlinear plant (a quadrotor over 100 steps) most samples diverge and the
nominal itself stays the best of them.  With `feedback=` the samples run in closed loop about feedback gains, u = uhat_t +
K_t (x_t - xhat_t) + noise (isls_sample_nominal_fb_*): noise injected at step t is corrected at the steps behind it, the samples
stay where the model is valid, and their cost reflects the route taken.  The gains are the caller's or, with feedback=True, those
of a backward pass about the nominal before every round.

The random numbers are counter-based (Philox4x32-10, csrc/philox.hpp): a draw depends on (seed, problem, sample, step, coordinate)
only, and the update generates the draws again instead of storing them.  There is no host loop behind this module: a forward model
or a cost that is a Python callable is refused."""
import numpy as np
import torch

from . import _capi as capi


class SampleResult:
    """What iSLS.sample_nominal returns (numpy): cost_before [B] (the nominal controls rolled out from xhat_0), cost_after [B],
    and per round cost_best_sample, took_best (bool), ess [B, rounds]; costs [B, S] of the last round with return_costs=True."""
    costs = None

    def __init__(self, **arrays):
        self.__dict__.update(arrays)


def check_feedback(feedback, B, N, m, n):
    """`feedback=` of sample_nominal: None (open loop; also False), True (gains from the device before each round), or the gains
    themselves, [N, m, n] or [B, N, m, n], numpy or torch, every entry finite -- returned as given (a torch tensor stays where it is);
    IslsError otherwise."""
    if feedback is None or feedback is False:
        return None
    if feedback is True:
        return True
    G = feedback if isinstance(feedback, torch.Tensor) else np.asarray(feedback)
    if tuple(G.shape) not in ((N, m, n), (B, N, m, n)):
        raise capi.IslsError(f"sample_nominal: feedback is True or gains [{N}, {m}, {n}] or [{B}, {N}, {m}, {n}], got {tuple(G.shape)}")
    if isinstance(G, torch.Tensor):
        ok = G.is_floating_point() and bool(torch.isfinite(G).all())
    else:
        ok = G.dtype.kind in "fiu" and bool(np.all(np.isfinite(G)))
    if not ok:
        raise capi.IslsError("sample_nominal: the feedback gains must be real and finite")
    return G


def check_args(B, m, samples, sigma, temperature, rounds, clip_u, feedback=None, N=None, n=None):
    """The refusals of sample_nominal that need no library (IslsError); returns (sigma [m] or [B, m], lo [m] or None, hi).
    feedback (with N and n): checked by check_feedback."""
    check_feedback(feedback, B, N, m, n)
    if int(samples) != samples or samples < 1:
        raise capi.IslsError(f"sample_nominal: samples >= 1, got {samples}")
    if int(rounds) != rounds or rounds < 1:
        raise capi.IslsError(f"sample_nominal: rounds >= 1, got {rounds}")
    if not (np.isfinite(temperature) and temperature > 0):
        raise capi.IslsError(f"sample_nominal: temperature > 0, got {temperature}")
    sg = np.asarray(sigma, dtype=np.float64)
    if sg.ndim == 0:
        sg = np.full(m, float(sg))
    if sg.shape not in ((m,), (B, m)):
        raise capi.IslsError(f"sample_nominal: sigma is a number, [{m}] or [{B}, {m}], got {sg.shape}")
    if not np.all(np.isfinite(sg)) or np.any(sg < 0):
        raise capi.IslsError("sample_nominal: sigma must be finite and >= 0")
    lo = hi = None
    if clip_u is not None:
        try:
            lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (m,)).copy() for v in clip_u)
        except ValueError:
            raise capi.IslsError(f"sample_nominal: clip_u = (lo, hi), numbers or [{m}]") from None
        if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(lo > hi):
            raise capi.IslsError("sample_nominal: clip_u needs lo <= hi")
    return np.ascontiguousarray(sg), lo, hi


def run(e, samples=1024, sigma=0.5, temperature=1.0, rounds=1, seed=0, clip_u=None, return_costs=False, feedback=None,
        feedback_checked=False):
    """`rounds` sampling rounds on the engine's own nominal, in place (round r draws with seed + r), then
    Engine.nominal_rewritten().  Nothing is read back before the last round has been enqueued.
    feedback: None (open loop), the gains [N, m, n] / [B, N, m, n] of the closed-loop round (used as given in every round), or a
    callable that leaves the gains of the nominal as it stands on the device and returns them (called before every round; it may
    read the device).  A bare True is iSLS.sample_nominal's (it hands the callable over): IslsError here.  feedback_checked: the
    caller has passed these gains through check_feedback already (they are not read a second time)."""
    if feedback is True:
        raise capi.IslsError("sampling.run: feedback is None, gains [N, m, n] / [B, N, m, n] or a callable that returns them; "
                             "feedback=True is served by iSLS.sample_nominal")
    if e.model is None:
        raise capi.IslsError("sample_nominal runs on the device: set forward_model to an isls.models descriptor")
    if not e.fast_dims:
        raise capi.IslsError(f"sample_nominal needs one of the (x_dim, u_dim) pairs with the row-per-lane kernels "
                             f"{capi.supported_dims()}, got ({e.n}, {e.m})")
    gains = feedback if callable(feedback) else None
    sg, lo, hi = check_args(e.B, e.m, samples, sigma, temperature, rounds, clip_u, None if gains or feedback_checked else feedback,
                            e.N, e.n)
    K = None if gains or feedback is None or feedback is False else e._t(feedback)
    B, S, R = e.B, int(samples), int(rounds)
    z = lambda *s_, dt=e.dtype: torch.zeros(*s_, dtype=dt, device=e.device)   # noqa: E731
    sigma_t, lo_t, hi_t = e._t(sg), None if lo is None else e._t(lo), None if hi is None else e._t(hi)
    costs = z(B, S)
    before, after, best, ess, took = z(B, R), z(B, R), z(B, R), z(B, R), z(B, R, dt=torch.int32)
    for r in range(R):
        if gains:
            try:
                K = gains()
            except Exception:
                if r:                                              # the rounds so far have moved the nominal
                    e.nominal_rewritten()
                raise
        e.sample_round(sigma_t, costs, u_lo=lo_t, u_hi=hi_t, temperature=temperature, seed=int(seed) + r, K=K,
                       cost_before=before[:, r], cost_after=after[:, r], cost_best=best[:, r], ess=ess[:, r], took_best=took[:, r])
    e.nominal_rewritten()
    before_h = before.cpu().numpy()
    res = SampleResult(cost_before=before_h[:, 0].copy(), cost_after=after[:, -1].cpu().numpy(),
                       cost_best_sample=best.cpu().numpy(), took_best=took.cpu().numpy().astype(bool), ess=ess.cpu().numpy())
    if return_costs:
        res.costs = costs.cpu().numpy()
    if not np.all(np.isfinite(before_h)):                      # the other problems have moved: the engine's state is consistent
        bad = np.flatnonzero(~np.isfinite(before_h).all(axis=1))
        raise capi.IslsError(f"sample_nominal: the nominal controls of problems {bad[:8].tolist()} roll out to a cost that is not "
                             f"finite; those problems were left as they are")
    return res
