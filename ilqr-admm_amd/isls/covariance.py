"""Closed-loop mean and covariance of a batch of stage-local controllers on the device (isls_cov_closed_loop_*,
csrc/covariance.hip): the analytic counterpart of `montecarlo`.

One launch propagates, for every problem, the mean and the covariance of the LINEARISED closed loop under its own gains K_t, k_t,
    Sig_{t+1} = (A_t + B_t K_t) Sig_t (A_t + B_t K_t)' + W_t ,   Su_t = K_t Sig_t K_t' ,
from an initial covariance and under process noise w_t ~ (0, W_t) added behind step t (the convention of the Monte-Carlo kernel:
x_{t+1} = f(x_t, u_t) + w_t), and returns per step and coordinate the mean, the variance and the Gaussian probability of leaving
a bound -- no sample is drawn.  `SLS.covariance` and `iSLS.covariance` are thin front ends of `run`.  The reference has no
covariance code.

Stage-local gains only ([N,m,n] / [P,N,m,n]): for a dense causal controller of an SLS design the spread of u is phi_u S0 phi_u'
by construction, and this module refuses it."""
import numpy as np
import torch

from . import _capi as capi


def _is_t(x):
    return isinstance(x, torch.Tensor)


class CovarianceResult:
    """Per problem, step and coordinate (numpy; torch tensors on the device where the caller passed K as a torch tensor; the
    leading problem axis is kept):  x_mean, x_var, p_x [P,N,n];  u_mean, u_var, p_u [P,N,m]  (p: the probability of lying outside
    the bound given, None without bounds on that block);  with full=True also x_cov [P,N,n,n], u_cov [P,N,m,m]."""
    x_cov = u_cov = p_x = p_u = None

    def __init__(self, **arrays):
        self.__dict__.update(arrays)

    @property
    def u_std(self):
        return torch.sqrt(self.u_var) if _is_t(self.u_var) else np.sqrt(self.u_var)

    @property
    def x_std(self):
        return torch.sqrt(self.x_var) if _is_t(self.x_var) else np.sqrt(self.x_var)

    def tightened(self, lo, hi, psi_inv):
        """The box [lo, hi] on u (anything that broadcasts to [P,N,m]) tightened into a chance constraint by psi_inv standard
        deviations: (lo + psi_inv sigma_u, hi - psi_inv sigma_u), arrays [P,N,m].  ValueError where the two cross."""
        sd = self.u_std
        if _is_t(sd):
            as_ = lambda v: torch.as_tensor(v, dtype=sd.dtype, device=sd.device)            # noqa: E731
            lo_t, hi_t = (as_(lo) + float(psi_inv) * sd).expand(sd.shape), (as_(hi) - float(psi_inv) * sd).expand(sd.shape)
            crossed = bool((lo_t > hi_t).any())
        else:
            lo_t = np.broadcast_to(np.asarray(lo, dtype=sd.dtype) + float(psi_inv) * sd, sd.shape)
            hi_t = np.broadcast_to(np.asarray(hi, dtype=sd.dtype) - float(psi_inv) * sd, sd.shape)
            crossed = bool(np.any(lo_t > hi_t))
        if crossed:
            raise ValueError(f"tightened: the bounds cross (lo + psi_inv sigma_u > hi - psi_inv sigma_u) at psi_inv = {psi_inv}: "
                             "the spread of u does not fit into the box at this confidence")
        return lo_t, hi_t


def stage_local(K, N, n, m):
    """True when K is per problem ([P,N,m,n]), False when shared ([N,m,n]); ValueError for a dense causal K or another shape"""
    s = tuple(K.shape)
    if s == (N, m, n):
        return False
    if len(s) == 4 and s[1:] == (N, m, n):
        return True
    if s == (N * m, N * n) or (len(s) == 3 and s[1:] == (N * m, N * n)):
        raise ValueError("covariance serves stage-local gains K [N,m,n] / [P,N,m,n]; for the dense causal controller of an SLS "
                         "design the spread of u is phi_u S0 phi_u' by construction (chance_constraint_rows)")
    raise ValueError(f"K: expected stage-local gains [N,m,n] or [P,N,m,n] with N={N}, m={m}, n={n}; got {s}")


def second_moment(std, cov, n, name, N=None):
    """A covariance from one of its two forms: per-coordinate standard deviations `std` (a scalar, [n] or [P,n]) or the full
    matrices `cov` ([n,n], [P,n,n] or, with N given, [P,N,n,n]).  Returns None (nothing given, or all zero standard deviations)
    or a numpy / torch array [n,n], [P,n,n] or [P,N,n,n]; ValueError for both forms at once or a wrong shape."""
    std_given = std is not None and (_is_t(std) or np.any(np.asarray(std) != 0))
    if cov is not None:
        if std_given:
            raise ValueError(f"give {name} as standard deviations or as a covariance, not both")
        s = tuple(cov.shape) if _is_t(cov) else np.shape(cov)
        ok = s == (n, n) or (len(s) == 3 and s[1:] == (n, n)) or (N is not None and len(s) == 4 and s[1:] == (N, n, n))
        if not ok:
            raise ValueError(f"{name}: expected [n,n], [P,n,n]" + (" or [P,N,n,n]" if N is not None else "") +
                             f" with n={n}" + (f", N={N}" if N is not None else "") + f"; got {s}")
        return cov if _is_t(cov) else np.asarray(cov, dtype=np.float64)
    if not std_given:
        return None
    sd = std.detach().cpu().numpy() if _is_t(std) else np.asarray(std, dtype=np.float64)
    if sd.ndim > 2 or (sd.ndim >= 1 and sd.shape[-1] not in (1, n)):
        raise ValueError(f"{name}: standard deviations are a scalar, [n] or [P,n] with n={n}; got {sd.shape}")
    sd = np.broadcast_to(sd, sd.shape[:-1] + (n,)) if sd.ndim else np.full(n, float(sd))
    return sd[..., :, None] * np.eye(n) * sd[..., None, :]


def _bound(e, b, P, N, d, name):
    """one side of a bound -> (tensor kept alive, View): scalar, [d], [N,d], [P,1,d] or [P,N,d]; None = free"""
    if b is None:
        return None, capi.View(None, 0, 0)
    t = e._t(np.asarray(b, dtype=np.float64) if not _is_t(b) else b)
    if t.numel() == 1 and t.ndim <= 1:
        t = t.reshape(()).expand(d).contiguous()
    return t, capi.make_view(t, P, N, (d,), name)


def _rows(t, core_ndim):
    """batch stride in elements of an operand that may carry a problem axis"""
    return int(np.prod(t.shape[1:])) if t.ndim > core_ndim and t.shape[0] != 1 else 0


def run(e, A, Bm, K, k, N, n, m, *, problems=None, xhat=None, uhat=None, dx0=None, x0_std=None, x0_cov=None, noise_scale=0.0,
        noise_cov=None, u_bounds=None, x_bounds=None, full=False, active=None, as_torch=None):
    """The launch behind SLS.covariance / iSLS.covariance.  `e`: the engine (dtype, device, kernels); A, Bm: anything make_view
    takes ([n,n], [N,n,n], [P,N,n,n], [1,1,n,n] ...); K [N,m,n] / [P,N,m,n], k to match or None (zero); xhat / uhat: the nominal
    ([N,.] shared, [P,N,.] or None: absolute form); dx0 [n] / [P,n]: the mean initial deviation (None: zero); active: int32 [P]
    or None; as_torch: the result as torch tensors on the device (default: where K is a torch tensor), else numpy."""
    n, m, N = int(n), int(m), int(N)
    out_torch = _is_t(K) if as_torch is None else bool(as_torch)
    arr = lambda t: t if t is None or _is_t(t) else np.asarray(t)                         # noqa: E731
    A, Bm, K, xhat, uhat, dx0 = (arr(t) for t in (A, Bm, K, xhat, uhat, dx0))
    per_problem = stage_local(K, N, n, m)
    if k is not None:
        k = k if _is_t(k) else np.asarray(k)
        if tuple(k.shape) != ((K.shape[0],) if per_problem else ()) + (N, m):
            raise ValueError(f"k: shape {tuple(k.shape)} does not go with K {tuple(K.shape)}")
    S0 = second_moment(x0_std, x0_cov, n, "the initial spread (x0_std / x0_cov)")
    W = second_moment(noise_scale, noise_cov, n, "the process noise (noise_scale / noise_cov)", N=N)
    if not capi.dims_supported(n, m):
        raise capi.IslsError(f"covariance: no kernel for (x_dim, u_dim) = ({n}, {m}); csrc/families.def lists the pairs served: "
                             f"{capi.supported_dims()}")
    cands = [K.shape[0]] if per_problem else []
    cands += [t.shape[0] for t, nd in ((A, 4), (Bm, 4), (xhat, 3), (uhat, 3), (dx0, 2), (S0, 3), (W, 3), (W, 4))
              if t is not None and len(t.shape) == nd]
    P = int(problems) if problems is not None else (max(cands) if cands else 1)
    if any(c not in (1, P) for c in cands):
        raise ValueError(f"operands disagree on the number of problems: {sorted(set(cands + [P]))}")

    dev, dt = e.device, e.dtype
    sfx = "f32" if dt == torch.float32 else "f64"
    a = capi.CovArgs(P=P, N=N, n=n, m=m)
    A_t, B_t = e._t(A), e._t(Bm)
    a.A, a.Bm = capi.make_view(A_t, P, N, (n, n), "A"), capi.make_view(B_t, P, N, (n, m), "B")
    K_t = e._t(K)
    a.K, a.K_sb = capi._ptr(K_t), _rows(K_t, 3)
    k_t = None if k is None else e._t(k)
    if k_t is not None:
        a.k, a.k_sb = capi._ptr(k_t), _rows(k_t, 2)
    keep = [A_t, B_t, K_t, k_t]
    for name, t, core in (("xhat", xhat, (N, n)), ("uhat", uhat, (N, m)), ("dx0", dx0, (n,))):
        if t is None:
            continue
        t = e._t(t)
        if tuple(t.shape[-len(core):]) != core or t.ndim > len(core) + 1:
            raise ValueError(f"{name}: expected {list(core)} or [P] + {list(core)}, got {tuple(t.shape)}")
        setattr(a, name, capi._ptr(t))
        setattr(a, name + "_sb", _rows(t, len(core)))
        keep.append(t)
    S0_t = torch.zeros(n, n, dtype=dt, device=dev) if S0 is None else e._t(S0)
    a.S0, a.S0_sb = capi._ptr(S0_t), _rows(S0_t, 2)
    if W is not None:
        W_t = e._t(W)
        W_t = W_t.reshape(W_t.shape[0], 1, n, n) if W_t.ndim == 3 else W_t                # [P,n,n]: per problem, every step
        a.W = capi.make_view(W_t, P, N, (n, n), "noise_cov")
        keep.append(W_t)
    u_lo_t, a.u_lo = _bound(e, None if u_bounds is None else u_bounds[0], P, N, m, "u_lo")
    u_hi_t, a.u_hi = _bound(e, None if u_bounds is None else u_bounds[1], P, N, m, "u_hi")
    x_lo_t, a.x_lo = _bound(e, None if x_bounds is None else x_bounds[0], P, N, n, "x_lo")
    x_hi_t, a.x_hi = _bound(e, None if x_bounds is None else x_bounds[1], P, N, n, "x_hi")
    act = None
    if active is not None:
        act = torch.as_tensor(np.asarray(active) if not _is_t(active) else active, dtype=torch.int32, device=dev).contiguous()
        if tuple(act.shape) != (P,):
            raise ValueError(f"active: expected [{P}], got {tuple(act.shape)}")
        a.active = capi._ptr(act)

    # problems that are not active keep what the outputs are created with: NaN
    new = lambda *s: torch.full(s, float("nan"), dtype=dt, device=dev)                    # noqa: E731
    out = dict(x_mean=new(P, N, n), u_mean=new(P, N, m), x_var=new(P, N, n), u_var=new(P, N, m))
    if full:
        out.update(x_cov=new(P, N, n, n), u_cov=new(P, N, m, m))
    if u_lo_t is not None or u_hi_t is not None:
        out["p_u"] = new(P, N, m)
    if x_lo_t is not None or x_hi_t is not None:
        out["p_x"] = new(P, N, n)
    for name, t in out.items():
        setattr(a, name, capi._ptr(t))
    e.kern.cov_closed_loop(a, sfx, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    del keep, S0_t, u_lo_t, u_hi_t, x_lo_t, x_hi_t, act
    if not out_torch:
        out = {name: t.cpu().numpy() for name, t in out.items()}
    return CovarianceResult(**out)
