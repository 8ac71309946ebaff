"""Monte-Carlo validation of a batch of controllers on the device (isls_mc_closed_loop_*, csrc/monte_carlo.hpp).

One launch rolls `samples` closed loops of every problem through its forward model and its own controller, draws the spread of
the initial states and the process noise on the device (or takes them as arrays), and returns per-problem violation counts and
extrema -- the trajectories only on request.  `SLS.monte_carlo` and `iSLS.monte_carlo` are thin front ends of `run`.

The random numbers are counter-based (Philox4x32-10, csrc/philox.hpp): a draw depends on (seed, problem, sample, step,
coordinate) only, so the chunks this module cuts large batches into are invisible in the results.  There is no host loop
behind this module: a forward model that is a Python callable is refused.

Chunks: the scratch of a launch (dense controllers: N n words per sample) is held under WORK_BYTES by cutting the problems, and
the samples of one problem if need be, into chunks.  K, k, x0s and w given as numpy arrays go to the device chunk by chunk, so a
batch of dense controllers ([P, N m, N n] grows as N^2) need not fit on the device at once; torch tensors are used where they
are.  The statistics ([P,N,.]) and, when asked for, the trajectories are allocated whole."""
import numpy as np
import torch

from . import _capi as capi

WORK_BYTES = 1 << 30            # scratch of one launch at most (dense controllers): larger batches are cut into chunks


class MonteCarloResult:
    """Statistics over the samples of every problem (numpy; the leading problem axis is kept):
    viol_u [P,N,m], viol_x [P,N,n]  samples outside the bound at that step and coordinate;  viol_any [P]  samples with any
    violation;  u_min, u_max [P,N,m], x_min, x_max [P,N,n];  samples.  With return_trajectories: x [P,M,N,n], u [P,M,N,m],
    w [P,M,N,n] (None without noise), x0 [P,M,n]."""
    x = u = w = x0 = None

    def __init__(self, samples, **arrays):
        self.samples = samples
        self.__dict__.update(arrays)

    @property
    def rate(self):
        """empirical probability of any violation, per problem"""
        return self.viol_any / float(self.samples)


def _form(K, N, n, m):
    """(K_form, per_problem) from the shape of K"""
    s = tuple(K.shape)
    if s == (N, m, n):
        return 0, False
    if len(s) == 4 and s[1:] == (N, m, n):
        return 0, True
    if s == (N * m, N * n):
        return 1, False
    if len(s) == 3 and s[1:] == (N * m, N * n):
        return 1, True
    raise ValueError(f"K: expected [N,m,n], [P,N,m,n], [N m, N n] or [P, N m, N n] with N={N}, m={m}, n={n}; got {s}")


def _bound(e, b, P, N, d, name):
    """one side of a bound -> (tensor kept alive, View): scalar, [d], [N,d], [P,1,d] or [P,N,d]; None = free"""
    if b is None:
        return None, capi.View(None, 0, 0)
    t = e._t(np.asarray(b, dtype=np.float64) if not isinstance(b, torch.Tensor) else b)
    if t.numel() == 1 and t.ndim <= 1:                         # one number for every coordinate
        t = t.reshape(()).expand(d).contiguous()
    return t, capi.make_view(t, P, N, (d,), name)


def run(e, model, par, K, k, N, n, m, *, samples=None, x0=None, x0_std=None, x0s=None, noise_scale=0.0, w=None, seed=0,
        u_bounds=None, x_bounds=None, xhat=None, uhat=None, problems=None, return_trajectories=False, chunk_problems=None,
        chunk_samples=None):
    """The launch(es) behind SLS.monte_carlo / iSLS.monte_carlo.  `e`: the engine (dtype, device, kernels); `model`, `par`: model
    id and its parameter rows ([q] shared or [P,q]); xhat / uhat: the nominal ([N,.] shared, [P,N,.] or None: absolute form)."""
    # operands with a problem axis stay where the caller has them (numpy on the host, torch on the device) until their chunk runs
    keep_ = lambda t: t if t is None or isinstance(t, torch.Tensor) else np.asarray(t)                # noqa: E731
    K, k = keep_(K), keep_(k)
    form, per_problem = _form(K, N, n, m)
    kcore = (N, m) if form == 0 else (N * m,)
    if tuple(k.shape) != ((K.shape[0],) if per_problem else ()) + kcore:
        raise ValueError(f"k: shape {tuple(k.shape)} does not go with K {tuple(K.shape)}")
    if (x0s is None) == (x0 is None):
        raise ValueError("give the mean x0 (with x0_std) or the explicit samples x0s, not both")
    if w is not None and np.any(np.asarray(noise_scale) != 0):
        raise ValueError("give noise_scale or the explicit noise w, not both")
    x0s, w = keep_(x0s), keep_(w)
    x0 = None if x0 is None else e._t(x0)
    xhat = None if xhat is None else e._t(xhat)
    uhat = None if uhat is None else e._t(uhat)
    # the number of problems: whatever carries a problem axis says it
    cands = [K.shape[0]] if per_problem else []
    cands += [t.shape[0] for t, nd in ((x0s, 3), (w, 4), (x0, 2), (xhat, 3), (uhat, 3)) if t is not None and t.ndim == nd]
    cands += [par.shape[0]] if par.ndim == 2 else []
    P = int(problems) if problems is not None else (max(cands) if cands else 1)
    if any(c not in (1, P) for c in cands):
        raise ValueError(f"operands disagree on the number of problems: {sorted(set(cands))}")
    if x0s is not None:
        x0s = x0s if x0s.ndim == 3 else x0s[None]
        M = x0s.shape[1]
        if x0s.shape[0] != P or x0s.shape[2] != n:
            raise ValueError(f"x0s: expected [P,M,n] = [{P},M,{n}], got {tuple(x0s.shape)}")
        if samples is not None and samples != M:
            raise ValueError("samples disagrees with x0s")
    elif w is not None and samples is None:
        M = w.shape[-3]
    else:
        if samples is None:
            raise ValueError("samples: how many closed loops per problem")
        M = int(samples)
    if w is not None:
        w = w if w.ndim == 4 else w[None]
        if tuple(w.shape) != (P, M, N, n):
            raise ValueError(f"w: expected [P,M,N,n] = {(P, M, N, n)}, got {tuple(w.shape)}")
    if x0 is not None and x0.shape[-1] != n:
        raise ValueError("x0: last dimension is not the state dimension")
    z = lambda v: None if v is None or not np.any(np.asarray(v) != 0) else e._t(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))   # noqa: E731
    x0_std_t = None if x0s is not None else z(x0_std)
    noise_t = z(noise_scale)
    dev, dt = e.device, e.dtype
    sfx = "f32" if dt == torch.float32 else "f64"

    u_lo_t, u_lo = _bound(e, None if u_bounds is None else u_bounds[0], P, N, m, "u_lo")
    u_hi_t, u_hi = _bound(e, None if u_bounds is None else u_bounds[1], P, N, m, "u_hi")
    x_lo_t, x_lo = _bound(e, None if x_bounds is None else x_bounds[0], P, N, n, "x_lo")
    x_hi_t, x_hi = _bound(e, None if x_bounds is None else x_bounds[1], P, N, n, "x_hi")

    zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)                     # noqa: E731
    full = lambda v, *s: torch.full(s, v, dtype=dt, device=dev)                       # noqa: E731
    viol_u, viol_x, viol_any = zi(P, N, m), zi(P, N, n), zi(P)
    u_min, u_max = full(float("inf"), P, N, m), full(-float("inf"), P, N, m)
    x_min, x_max = full(float("inf"), P, N, n), full(-float("inf"), P, N, n)
    noisy = w is not None or noise_t is not None
    traj = {}
    if return_trajectories:
        zt = lambda *s: torch.zeros(*s, dtype=dt, device=dev)                           # noqa: E731
        traj = dict(x=zt(P, M, N, n), u=zt(P, M, N, m), w=zt(P, M, N, n) if noisy else None, x0=zt(P, M, n))

    # chunks: over the problems so that the scratch of a launch stays under WORK_BYTES, over the samples when one problem's does not
    item = 4 if dt == torch.float32 else 8
    per_sample = N * n * item if form == 1 else 0
    Mc = M if chunk_samples is None else max(1, min(M, int(chunk_samples)))
    if chunk_samples is None and per_sample and per_sample * (-(-M // 128) * 128) > WORK_BYTES:
        Mc = max(128, WORK_BYTES // per_sample // 128 * 128)
    Pc = P if chunk_problems is None else max(1, min(P, int(chunk_problems)))
    if chunk_problems is None and per_sample:
        Pc = max(1, min(P, WORK_BYTES // (per_sample * (-(-Mc // 128) * 128))))
    work = torch.empty(capi.mc_work_elems(Pc, Mc, N, n, m, form), dtype=dt, device=dev) if form == 1 else None

    def rows(t, nd, p0, p1):
        """rows p0:p1 of an operand with a problem axis, (tensor, problem stride)"""
        if t is None:
            return None, 0
        if t.ndim < nd or t.shape[0] == 1:
            return t, 0
        c = t[p0:p1]
        return c, int(np.prod(c.shape[1:]))

    def view_rows(v, p0):
        return capi.View((v.p + p0 * v.sb * item) if v.p else None, v.sb, v.st)

    stream = torch.cuda.current_stream().cuda_stream
    for p0 in range(0, P, Pc):
        p1 = min(P, p0 + Pc)
        for s0 in range(0, M, Mc):
            s1 = min(M, s0 + Mc)
            whole = s0 == 0 and s1 == M
            a = capi.McLoopArgs(P=p1 - p0, M=s1 - s0, N=N, n=n, m=m, model=int(model), K_form=form)
            pr, a.par_sb = rows(par, 2, p0, p1)
            Kc, a.K_sb = rows(K, 4 if form == 0 else 3, p0, p1)
            kc, a.k_sb = rows(k, 3 if form == 0 else 2, p0, p1)
            xh, a.xhat_sb = rows(xhat, 3, p0, p1)
            uh, a.uhat_sb = rows(uhat, 3, p0, p1)
            xm, a.x0_sb = rows(x0, 2, p0, p1)
            Kc, kc = e._t(Kc), e._t(kc)
            a.model_par, a.K, a.k, a.xhat, a.uhat, a.x0 = (capi._ptr(t) for t in (pr, Kc, kc, xh, uh, xm))
            xs = None if x0s is None else e._t(x0s[p0:p1, s0:s1])
            wc = None if w is None else e._t(w[p0:p1, s0:s1])
            a.x0s, a.w = capi._ptr(xs), capi._ptr(wc)
            a.x0_std, a.noise_std, a.seed = capi._ptr(x0_std_t), capi._ptr(noise_t), int(seed) & 0xFFFFFFFFFFFFFFFF
            a.problem0, a.sample0 = p0, s0
            a.u_lo, a.u_hi, a.x_lo, a.x_hi = (view_rows(v, p0) for v in (u_lo, u_hi, x_lo, x_hi))
            a.viol_u, a.viol_x, a.viol_any = (capi._ptr(t[p0:p1]) for t in (viol_u, viol_x, viol_any))
            a.u_min, a.u_max, a.x_min, a.x_max = (capi._ptr(t[p0:p1]) for t in (u_min, u_max, x_min, x_max))
            outs = {}
            if return_trajectories:
                for name, t in traj.items():
                    if t is not None:
                        outs[name] = t[p0:p1] if whole else torch.empty_like(t[p0:p1, s0:s1])
                a.x_log, a.u_log, a.x0_out = capi._ptr(outs["x"]), capi._ptr(outs["u"]), capi._ptr(outs["x0"])
                a.w_out = capi._ptr(outs.get("w"))
            a.work, a.work_elems = capi._ptr(work), (work.numel() if work is not None else 0)
            e.kern.mc_closed_loop(a, sfx, stream=stream)
            if not whole:
                for name, t in outs.items():
                    traj[name][p0:p1, s0:s1].copy_(t)
            # the chunk's tensors go back to torch's allocator here: the launch is on torch's current stream, which orders their reuse
    torch.cuda.current_stream().synchronize()
    del u_lo_t, u_hi_t, x_lo_t, x_hi_t
    host = lambda t: None if t is None else t.cpu().numpy()                              # noqa: E731
    return MonteCarloResult(M, viol_u=host(viol_u), viol_x=host(viol_x), viol_any=host(viol_any), u_min=host(u_min),
                            u_max=host(u_max), x_min=host(x_min), x_max=host(x_max), **{kk: host(v) for kk, v in traj.items()})
