"""Built-in non-quadratic cost models with a device implementation (line search + expansion).

The reference takes arbitrary `cost_function(x, u)` / `get_Cs(x, u)` callbacks (isls/isls.py:102,360); a HIP kernel
cannot call back into Python, so a cost that the line search evaluates for every candidate has to be one the kernels
know.  `Custom` is a cost of the user's own, written once as a short HIP C++ function and compiled at run time for gfx950 into the
line search of whichever model it is used with, plus an expansion on second-order forward-mode numbers (no get_Cs to write).
`PseudoHuber` is the car-parking cost of notebooks/Tutorial.ipynb cell 14 (Tassa et al.): assigning an instance to
`iSLS.cost_function` selects ISLS_COST_PHUBER on the device; the object itself is the numpy version of the same cost
(and of its derivatives, which the notebook gets from autograd) for use on the host and in tests.
"""
import numpy as np

from . import _capi as capi
from .models import UserSource


class PseudoHuber:
    """sum_t [ sum_i cu_i u_ti^2 + sum_i cx_i ph(x_ti, px_i) ] + sum_i cf_i ph(x_{N-1,i}, pf_i),  ph(x,p) = sqrt(x^2+p^2) - p.
    cu [m]; cx, px, cf, pf [n] (entries of cx / cf may be zero; the matching px / pf must not be)."""
    cost_model = capi.COST_PHUBER

    def __init__(self, cu, cx, px, cf, pf):
        self.cu, self.cx, self.px, self.cf, self.pf = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (cu, cx, px, cf, pf))

    def params(self):
        return np.concatenate([self.cu, self.cx, self.px, self.cf, self.pf])

    @staticmethod
    def _ph(x, p):
        return np.sqrt(x ** 2 + p ** 2) - p

    def __call__(self, x, u):
        """x [..., N, n], u [..., N, m] -> cost [...] (Tutorial.ipynb cell 14, `cost`; NaN -> 1e6 for stacked candidates)."""
        x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
        c = np.sum(self.cu * u ** 2, axis=(-1, -2)) + np.sum(self.cx * self._ph(x, self.px), axis=(-1, -2))
        c = c + np.sum(self.cf * self._ph(x[..., -1, :], self.pf), axis=-1)
        if x.ndim == 3:
            c = np.where(np.isnan(c), 1e6, c)
        return c

    def get_Cs(self, x, u):
        """(cs [N, n+m], Cs [N, n+m, n+m]): gradient and Hessian per time step (Tutorial.ipynb cell 16 without autograd)."""
        x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
        N, n = x.shape
        m = u.shape[1]
        s1 = np.sqrt(x ** 2 + self.px ** 2)
        g, h = self.cx * x / s1, self.cx * self.px ** 2 / s1 ** 3
        s2 = np.sqrt(x[-1] ** 2 + self.pf ** 2)
        g[-1] += self.cf * x[-1] / s2
        h[-1] += self.cf * self.pf ** 2 / s2 ** 3
        cs = np.concatenate([g, 2 * self.cu * u], axis=1)
        Cs = np.zeros((N, n + m, n + m))
        idx = np.arange(n + m)
        Cs[:, idx, idx] = np.concatenate([h, np.broadcast_to(2 * self.cu, (N, m))], axis=1)
        return cs, Cs


class Custom(UserSource):
    """A cost of the user's own: `source` defines

        template <typename S, typename P>
        __device__ S stage(const S *x, const S *u, const P *par, int t, int N);

    the cost of step t in plain arithmetic on S (the contract of csrc/user_model_ad.hpp); the total cost is the sum over
    t = 0 .. N-1 (a terminal term: `if (t == N - 1)`; u_{N-1} is costed, as the reference does).  Assigned to
    `iSLS.cost_function` it puts the line search, the nominal cost and the expansion on the device, with any built-in model or a
    `models.Custom`: the library compiles it at run time for gfx950 (hiprtc) into the rollout kernel of that model and into an
    expansion on hyper-dual numbers -- gradient and full Hessian, x-u cross terms included, come from `stage` itself, so
    `get_Cs=None` is all `solve` / `ilqr_admm` need.  `params` is [P] (shared) or [B, P] (one row per trajectory), P <= 16.
    Only the (x_dim, u_dim) pairs with the row-per-lane kernels are served (`isls._capi.supported_dims()`).

    Per-step data (a reference to track, weights that change along the horizon, a moving obstacle): `table` is [N, W] (shared by
    the batch) or [B, N, W] (one per trajectory), 1 <= W <= 16, and `source` then defines the six-argument form

        template <typename S, typename P>
        __device__ S stage(const S *x, const S *u, const P *par, const P *row, int t, int N);

    `row` the W words of step t: plain P, never differentiated.  `set_table` replaces the values (same shape) between two calls
    of a solver -- a receding-horizon window: no compile, and the engines holding the cost copy the new values into the device
    table they already have.

    Nonlinear path constraints g(x, u) <= 0 (a keep-out region of any shape, a friction cone, a limit on a nonlinear function of
    the state, an inequality that couples x and u): `constraints=K` (K >= 1), and `source` also defines

        template <typename S, typename P>
        __device__ void constraint(const S *x, const S *u, const P *par, int t, int N, S *g);

    (with a table both functions take `const P *row` behind `par`); feasible is g[i] <= 0.  The solver treats them by augmented
    Lagrangian: what it costs a step with is stage + sum_i PHR(lambda_i, mu, g_i) (csrc/user_cost.hpp), the multipliers lambda
    [B, N, K] and the penalty mu [B] ride on the device in the cost's per-step table, [user row (W) | lambda | mu], W + K + 1 <= 16,
    one table per trajectory from the moment the cost is assigned to an iSLS (a shared table is replicated then).  `iSLS.solve_al`
    runs the outer loop; every other solver runs on the multipliers that stand.  `multipliers`, `penalty`: the host copies;
    `reset_multipliers(mu)`: lambda = 0, mu = mu; `constraint(x, u)`: g on the device; __call__ and get_Cs evaluate the augmented
    cost with the current multipliers (exactly `stage` while lambda = 0 and mu = 0, which is how the object starts).  Such a cost
    belongs to one iSLS at a time (a second assignment is an IslsError until the first iSLS takes another cost); assigned to an
    iSLS of another batch or horizon afterwards, its multipliers start again at lambda = 0, mu = the last reset's.

    A map (a signed-distance map from an occupancy grid, a terrain height map, a risk map -- 10^4 .. 10^6 words, shared by the
    batch and indexed by the state): `field` is [nx, ny] or [C, nx, ny] (C <= 4 channels, nx, ny >= 4), sample [c, i, j] at
    (field_origin[0] + i field_spacing[0], field_origin[1] + j field_spacing[1]), and `stage` and `constraint` read it as

        isls::field(c, px, py)        c: a plain int channel; px, py: each an S or a plain number; the result an S

    with exact first and second derivatives: the tensor-product Catmull-Rom cubic (csrc/user_field.hpp), C1, exact on the samples
    and on polynomials up to degree 2 per variable; outside the grid the field continues as a constant (zero derivative along a
    clamped axis).  It composes with `table=` and `constraints=`: `g[0] = par[0] - isls::field(0, x[0], x[1])` keeps a car at a
    clearance par[0] from a region known only by its distance map.  `field`: the host copy; `set_field(values)` replaces the
    values (same shape) between two calls of a solver -- no compile, and the copy goes INTO the device buffers the cost owns.
    Each such object is a registration of its own, and it owns device memory: an fp64 and an fp32 copy of the samples (12 bytes per
    sample) on every device it has been used on, which garbage collection of the object does NOT free -- they live until
    `release_field()` or the end of the process.  A program that builds many field costs (one per map) calls `release_field()` on
    the ones it is done with; one that only changes the map keeps one object and calls `set_field`.  After `release_field()` the
    object still works: its next use puts the host copy on the device again.  A field per trajectory is not served.  One read per step keeps the
    fp64 line search free of scratch memory; a stage with several reads per step may spill registers there."""

    def __init__(self, x_dim, u_dim, params, source, table=None, constraints=0, field=None, field_origin=(0.0, 0.0),
                 field_spacing=(1.0, 1.0)):
        self._lam = self._mu = None                           # host copies of the multipliers [B, N, K] and penalties [B]
        self._mu_init, self._mult_version = 0.0, 0
        self._owner = None                                    # weakref to the iSLS whose device table holds the multipliers
        shape = None
        if field is not None:
            self._field = self._field_values(field, None)
            self._field_origin, self._field_spacing = (tuple(float(v) for v in np.ravel(a)) for a in (field_origin, field_spacing))
            if len(self._field_origin) != 2 or len(self._field_spacing) != 2 or not all(np.isfinite(self._field_origin)):
                raise ValueError("field_origin, field_spacing: (x0, y0), (dx, dy)")
            if not all(np.isfinite(d) and d > 0 for d in self._field_spacing):
                raise ValueError(f"field_spacing: dx, dy > 0, got {self._field_spacing}")
            shape = self._field.shape if self._field.ndim == 3 else (1,) + self._field.shape
            self._field_on = {}                               # device index -> the version of the values in the device buffers there
        self.cost_model = self._register("cost", capi.user_cost_create, x_dim, u_dim, params, source, table=table,
                                         constraints=constraints, field=shape)

    # ---- the field ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _field_values(field, like):
        """`field` as the fp64 host copy, checked against the limits of the registration (like=None) or the shape that stands"""
        field = np.array(field, dtype=np.float64, order="C")
        if like is not None:
            if field.shape != like.shape:
                raise ValueError(f"set_field: the field is {like.shape}, got {field.shape} (a new shape is a new costs.Custom)")
            return field
        if field.ndim == 4:
            raise ValueError(f"field: [nx, ny] or [C, nx, ny], one field shared by the batch; got {field.shape} -- a field per "
                             "trajectory is not served (put the maps into the channels, or build one cost per map)")
        if field.ndim not in (2, 3):
            raise ValueError(f"field: [nx, ny] or [C, nx, ny], got {field.shape}")
        C, nx, ny = ((1,) + field.shape)[-3:]
        if not 1 <= C <= capi.USER_MAX_FIELD:
            raise ValueError(f"field: 1 <= C <= {capi.USER_MAX_FIELD} channels, got {C}")
        if nx < 4 or ny < 4:
            raise ValueError(f"field: nx, ny >= 4 (the interpolant has four taps per axis), got {nx} x {ny}")
        if C * nx * ny > capi.USER_MAX_FIELD_WORDS:
            raise ValueError(f"field: at most {capi.USER_MAX_FIELD_WORDS} samples over all channels, got {C * nx * ny}")
        return field

    @property
    def field(self):
        """The host copy of the field ([nx, ny] or [C, nx, ny] as it was given; None: a cost without one)."""
        return self._field

    @property
    def field_origin(self):
        return self._field_origin if self._field is not None else None

    @property
    def field_spacing(self):
        return self._field_spacing if self._field is not None else None

    def set_field(self, values):
        """New values for the field, of the shape it has: the next call of a solver on any iSLS holding this object, and the next
        evaluation of the object itself, use them -- no compile, one copy into the device buffers the cost owns."""
        if self._field is None:
            raise ValueError("set_field: this cost was built without a field")
        self._field, self._field_version = self._field_values(values, self._field), self._field_version + 1

    def release_field(self):
        """Free the device copies of the field on every device (the host copy stays; the next use of the cost uploads it again).
        The cost's registration and its compiled programs are kept."""
        if self._field is None:
            raise ValueError("release_field: this cost was built without a field")
        capi.user_cost_release_field(self.cost_model)
        self._field_on = {}

    def _push_field(self, device=None):
        """The values that stand into the cost's buffers on `device` (the current one), unless they are there already"""
        if self._field is None:
            return
        import torch
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        index = torch.cuda.current_device() if dev.index is None else dev.index
        if self._field_on.get(index) == self._field_version:
            return
        with torch.cuda.device(index):
            values = torch.as_tensor(self._field, device=torch.device("cuda", index)).reshape(capi.user_cost_field_dims(self.cost_model))
            capi.user_cost_set_field(self.cost_model, values, self._field_origin, self._field_spacing,
                                     stream=torch.cuda.current_stream().cuda_stream)
        self._field_on[index] = self._field_version

    # ---- constraints: the multipliers and the library's table ----------------------------------------------------------------
    @property
    def multipliers(self):
        """lambda [B, N, K] (None until the cost has met a batch: assigned to an iSLS)"""
        return self._lam

    @property
    def penalty(self):
        """mu [B] (None until the cost has met a batch)"""
        return self._mu

    def reset_multipliers(self, mu=1.0):
        """lambda = 0 and mu = mu for every trajectory; the iSLS holding the cost copy them into their device table at their next call"""
        if not self.n_con:
            raise ValueError("reset_multipliers: this cost was built without constraints")
        self._mu_init = float(mu)
        if self._lam is not None:
            self._lam, self._mu = np.zeros_like(self._lam), np.full_like(self._mu, float(mu))
        self._mult_version += 1

    def _al_table(self, B, N, bind=True):
        """The library's table [B, N, W + K + 1] = [user row | lambda | mu] for B trajectories of N steps, from the host copies.
        bind: multipliers of another shape (or none yet) start again at lambda = 0, mu = the last reset's; else they must fit."""
        W, K = self.n_tab, self.n_con
        if self._table is not None and (self._table.shape[-2] != N or (self._table.ndim == 3 and self._table.shape[0] != B)):
            raise ValueError(f"the cost's table is {self._table.shape}, needed [{N}, {W}] or [{B}, {N}, {W}]")
        lam, mu = self._lam, self._mu
        if lam is None or lam.shape != (B, N, K):
            if lam is not None and not bind:
                raise ValueError(f"the cost's multipliers are {lam.shape}: x, u of [{lam.shape[0]}, {lam.shape[1]}, .]")
            lam, mu = np.zeros((B, N, K)), np.full(B, self._mu_init)
            if bind:
                self._lam, self._mu = lam, mu
        tab = np.empty((B, N, W + K + 1))
        if W:
            tab[..., :W] = self._table
        tab[..., W:W + K], tab[..., W + K] = lam, mu[:, None]
        return tab

    def _pull(self, tab):
        """The multipliers and penalties out of a library table [B, N, W + K + 1] (numpy) into the host copies"""
        W, K = self.n_tab, self.n_con
        self._lam, self._mu = np.array(tab[..., W:W + K], dtype=np.float64), np.array(tab[:, 0, W + K], dtype=np.float64)

    def constraint(self, x, u):
        """x [..., N, n], u [..., N, m] -> g [..., N, K] (numpy, fp64), evaluated on the device by the kernel that updates the multipliers."""
        if not self.n_con:
            raise ValueError("constraint: this cost was built without constraints")
        torch, kern, lead, R, N, xs, us, par, dev = self._batch(x, u, multipliers=False)
        g = torch.empty(R, N, self.n_con, dtype=torch.float64, device=dev)
        viol = torch.zeros(2, R, dtype=torch.float64, device=dev)
        kern.user_constraint_update(self.cost_model, par, self._tab_dev, xs, us, viol[0], viol[1], update=False, g_out=g,
                                    stream=torch.cuda.current_stream().cuda_stream)
        return g.cpu().numpy().reshape(lead + (N, self.n_con))

    def code(self, model=None, dtype=np.float64):
        """The gfx950 code object of the cost for dtype: with `model` (an isls.models object or a model id) every kernel of the
        pair -- line search, expansion, value --, without one the expansion and the value."""
        mid = -1 if model is None else int(getattr(model, "model_id", model))
        return capi.user_cost_code(self.cost_model, mid, dtype)

    def _load(self, dtype):
        self._push_field()
        capi.user_cost_load(self.cost_model, -1, dtype)

    def _batch(self, x, u, multipliers=True):
        x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
        lead = np.broadcast_shapes(x.shape[:-2], u.shape[:-2])
        N = x.shape[-2]
        R = int(np.prod(lead)) if lead else 1
        if self._table is not None and self._table.shape[-2] != N:
            raise ValueError(f"the cost's table has {self._table.shape[-2]} steps, x has {N}")
        torch, kern, dev, (par, xs, us) = self._on_device(R, "{0} trajectories x, u, got {1}",
                                                           np.broadcast_to(x, lead + (N, self.x_dim)).reshape(R, N, self.x_dim),
                                                           np.broadcast_to(u, lead + (N, self.u_dim)).reshape(R, N, self.u_dim))
        if self.n_con:                                        # the library's table, one per trajectory (multipliers=False: zeros)
            keep = self._lam, self._mu
            if not multipliers:
                self._lam = None
            try:
                self._tab_dev = torch.as_tensor(self._al_table(R, N, bind=False), device=dev)
            finally:
                self._lam, self._mu = keep
        else:
            self._tab_dev = None if self._table is None else torch.as_tensor(self._table, device=dev)
        return torch, kern, lead, R, N, xs, us, par, dev

    def __call__(self, x, u):
        """x [..., N, n], u [..., N, m] -> cost [...] (numpy, fp64), evaluated on the device."""
        torch, kern, lead, R, N, xs, us, par, dev = self._batch(x, u)
        cost = torch.empty(R, dtype=torch.float64, device=dev)
        kern.user_cost_value(self.cost_model, par, xs, us, cost, stream=torch.cuda.current_stream().cuda_stream, tab=self._tab_dev)
        c = cost.cpu().numpy().reshape(lead)
        return float(c) if lead == () else c

    def get_Cs(self, x, u):
        """(cs [N, n+m], Cs [N, n+m, n+m]) along x [N,n], u [N,m] in the reference's convention (or with a leading batch axis), on
        the device by the same hyper-dual kernel the solver expands with."""
        single = np.ndim(x) == 2
        torch, kern, lead, R, N, xs, us, par, dev = self._batch(x, u)
        n, m = self.x_dim, self.u_dim
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=dev)   # noqa: E731
        Cxx, Cuu, Cux, c0x, c0u = z(R, N, n, n), z(R, N, m, m), z(R, N, m, n), z(R, N, n), z(R, N, m)
        zero = z(1, n, n)
        exp = capi.Kernels.expand_args(zero, zero[0, :1], torch.zeros(N, dtype=torch.int32, device=dev), 0.0, c0x, c0u, xhat=xs, uhat=us,
                                       Cxx=Cxx, Cuu=Cuu, cost_model=self.cost_model, cost_par=par, cost_tab=self._tab_dev)
        kern.user_cost_expand(exp, Cux, "f64", stream=torch.cuda.current_stream().cuda_stream)
        cs = torch.cat([c0x, c0u], dim=-1).cpu().numpy()
        Cs = torch.cat([torch.cat([Cxx, Cux.transpose(-1, -2)], dim=-1), torch.cat([Cux, Cuu], dim=-1)], dim=-2).cpu().numpy()
        if single:
            return cs[0], Cs[0]
        return cs.reshape(lead + cs.shape[1:]), Cs.reshape(lead + Cs.shape[1:])
