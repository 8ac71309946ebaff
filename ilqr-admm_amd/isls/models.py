"""Built-in forward models with device implementations (HIP kernels `rollout_ls` / `linearize`).

The reference takes arbitrary Python callbacks `forward_model(x,u)` and `get_AB(x,u)` (isls/isls.py:61-66,
isls/isls_base.py:105-111); the systems its notebooks define are provided here as descriptors that select
the device implementation.  A descriptor is also callable with the reference's calling
convention (`f(x[L,n], u[L,m]) -> [L,n]` on numpy), which is what the reference's notebooks plot with.
`Custom` is a model of the user's own, written once as a short HIP C++ function and compiled at run time for gfx950 into the
kernels the built-in models use (line search, linearisation, closed loops).
"""
import re

import numpy as np

from . import _capi as capi


class Model:
    model_id = None
    x_dim = u_dim = None

    def params(self):
        raise NotImplementedError

    def get_AB(self, x, u):
        """Numpy linearisation in the reference's convention: x[N,n], u[N,m] -> A[N,n,n], B[N,n,m]."""
        raise NotImplementedError


class LTI(Model):
    """x+ = A x + B u (isls/sls_base.py:49-53); A,B [n,n],[n,m] shared or [B,n,n],[B,n,m] per trajectory."""

    def __init__(self, A, B):
        self.A, self.B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        self.x_dim, self.u_dim = self.A.shape[-1], self.B.shape[-1]

    def _double_integrator(self):
        """(a, b0, b1) if A = [[I, aI],[0, I]] and B = [[b0 I],[b1 I]] exactly (get_double_integrator_AB(d, 2, dt)), else None."""
        n, m = self.x_dim, self.u_dim
        if self.A.ndim != 2 or n != 2 * m:
            return None
        a, b0, b1 = self.A[0, m], self.B[0, 0], self.B[m, 0]
        eye, zero = np.eye(m), np.zeros((m, m))
        if np.array_equal(self.A, np.block([[eye, a * eye], [zero, eye]])) and np.array_equal(self.B, np.vstack([b0 * eye, b1 * eye])):
            return np.array([a, b0, b1])
        return None

    @property
    def model_id(self):
        # a double integrator is evaluated through its Kronecker structure (ISLS_MODEL_DI): same numbers, 1/6 of the work
        return capi.MODEL_DI if self._double_integrator() is not None else capi.MODEL_LTI

    def params(self):
        di = self._double_integrator()
        if di is not None:
            return di
        if self.A.ndim == 2:
            return np.concatenate([self.A.ravel(), self.B.ravel()])
        nb = self.A.shape[0]
        return np.concatenate([self.A.reshape(nb, -1), self.B.reshape(nb, -1)], axis=1)

    def __call__(self, x, u):
        return x @ self.A.T + u @ self.B.T

    def get_AB(self, x, u):
        N = x.shape[0]
        return np.broadcast_to(self.A, (N,) + self.A.shape[-2:]).copy(), np.broadcast_to(self.B, (N,) + self.B.shape[-2:]).copy()


class Planar3R(Model):
    """Planar 3R arm of notebooks/3DoF robot (state [q, qd, ee], u = qdd), unit links, closed-form FK/J."""
    model_id = capi.MODEL_ARM3R
    x_dim, u_dim = 9, 3

    def __init__(self, dt):
        self.dt = float(dt)

    def params(self):
        return np.array([self.dt])

    @staticmethod
    def fk(q):
        c = np.cumsum(q, axis=-1)
        return np.stack([np.cos(c).sum(-1), np.sin(c).sum(-1), np.zeros(q.shape[:-1])], axis=-1)

    @staticmethod
    def jacobian(q):
        c = np.cumsum(q, axis=-1)
        J = np.zeros(q.shape[:-1] + (3, 3))
        for j in range(3):
            J[..., 0, j] = -np.sin(c[..., j:]).sum(-1)
            J[..., 1, j] = np.cos(c[..., j:]).sum(-1)
        return J

    def __call__(self, x, u):
        dt = self.dt
        q = x[..., :3] + x[..., 3:6] * dt + 0.5 * u * dt ** 2
        return np.concatenate([q, x[..., 3:6] + u * dt, self.fk(q)], axis=-1)

    def get_AB(self, x, u):
        dt, N = self.dt, x.shape[0]
        A, B = np.zeros((N, 9, 9)), np.zeros((N, 9, 3))
        for j in range(3):
            A[:, j, j] = A[:, 3 + j, 3 + j] = 1.0
            A[:, j, 3 + j] = dt
            B[:, j, j], B[:, 3 + j, j] = 0.5 * dt ** 2, dt
        J = self.jacobian(x[..., :3] + x[..., 3:6] * dt + 0.5 * u * dt ** 2)
        A[:, 6:, :3], A[:, 6:, 3:6], B[:, 6:] = J, J * dt, 0.5 * J * dt ** 2
        return A, B


class CarSimple(Model):
    """Car of notebooks/Car/Iterative LQR with state constraints.ipynb cell 6: [x, y, theta, v], [omega, a]."""
    model_id = capi.MODEL_CAR
    x_dim, u_dim = 4, 2

    def __init__(self, dt):
        self.dt = float(dt)

    def params(self):
        return np.array([self.dt])

    def __call__(self, x, u):
        dt = self.dt
        return np.stack([x[..., 0] + dt * x[..., 3] * np.cos(x[..., 2]), x[..., 1] + dt * x[..., 3] * np.sin(x[..., 2]),
                         (x[..., 2] + dt * x[..., 3] * u[..., 0]) % (2 * np.pi), x[..., 3] + dt * u[..., 1]], axis=-1)

    def get_AB(self, x, u):
        dt, N = self.dt, x.shape[0]
        A, B = np.tile(np.eye(4), (N, 1, 1)), np.zeros((N, 4, 2))
        th, v = x[..., 2], x[..., 3]
        A[:, 0, 2], A[:, 1, 2] = -dt * v * np.sin(th), dt * v * np.cos(th)
        A[:, 0, 3], A[:, 1, 3], A[:, 2, 3] = dt * np.cos(th), dt * np.sin(th), dt * u[..., 0]
        B[:, 2, 0], B[:, 3, 1] = dt * v, dt
        return A, B


class TassaCar(Model):
    """Car-parking model of notebooks/Tutorial.ipynb cell 8 (Tassa et al.): [x, y, theta, v], [front wheel angle w,
    acceleration a], axle distance `dist`; the Jacobians the notebook takes from autograd are written out here."""
    model_id = capi.MODEL_TASSA
    x_dim, u_dim = 4, 2

    def __init__(self, dt, dist=2.0):
        self.dt, self.dist = float(dt), float(dist)

    def params(self):
        return np.array([self.dt, self.dist])

    def __call__(self, x, u):
        dt, d = self.dt, self.dist
        f = dt * x[..., 3]
        sw = np.sin(u[..., 0]) * f
        b = (f * np.cos(u[..., 0]) + d) - np.sqrt(d * d - sw * sw)
        return np.stack([x[..., 0] + b * np.cos(x[..., 2]), x[..., 1] + b * np.sin(x[..., 2]), x[..., 2] + np.arcsin(sw / d),
                         x[..., 3] + u[..., 1] * dt], axis=-1)

    def get_AB(self, x, u):
        dt, d, N = self.dt, self.dist, x.shape[0]
        f, sw, cw = dt * x[..., 3], np.sin(u[..., 0]), np.cos(u[..., 0])
        r = np.sqrt(d * d - (sw * f) ** 2)
        b, dbdf, dbdw = (f * cw + d) - r, cw + (sw * sw * f) / r, -f * sw + (sw * cw * f * f) / r
        st, ct = np.sin(x[..., 2]), np.cos(x[..., 2])
        A, B = np.tile(np.eye(4), (N, 1, 1)), np.zeros((N, 4, 2))
        A[:, 0, 2], A[:, 1, 2] = -b * st, b * ct
        A[:, 0, 3], A[:, 1, 3], A[:, 2, 3] = (dbdf * dt) * ct, (dbdf * dt) * st, (sw / r) * dt
        B[:, 0, 0], B[:, 1, 0], B[:, 2, 0], B[:, 3, 1] = dbdw * ct, dbdw * st, (cw * f) / r, dt
        return A, B


class UserSource:
    """What models.Custom and costs.Custom share: the validation and registration of a run-time compiled source (`noun`: model |
    cost), its per-step table and the way their host-side evaluations put numpy arrays on the device."""

    _table = None                                            # the per-step table (Custom(table=)): [N, W] or [B, N, W]
    _table_version = 0

    n_con = 0                                                # path constraints of a cost (costs.Custom(constraints=)), 0: none

    _field = None                                            # the 2-D field of a cost (costs.Custom(field=)): [C, nx, ny]
    _field_version = 0

    def _register(self, noun, create, x_dim, u_dim, params, source, table=None, constraints=0, field=None):
        self._noun, self.x_dim, self.u_dim = noun, int(x_dim), int(u_dim)
        K = int(constraints)
        if K < 0:
            raise ValueError("constraints: K >= 0")
        if K:                                                # the library's row: [user row (W) | K multipliers | mu], checked ahead of any compile
            W = 0 if table is None else int(np.shape(table)[-1])
            if W + K + 1 > capi.USER_MAX_TAB:
                raise ValueError(f"a table of W = {W} words and K = {K} constraints make a row of W + K + 1 = {W + K + 1} words "
                                 f"(user row, multipliers, penalty): at most {capi.USER_MAX_TAB}")
        self.n_con = K
        if table is not None:
            table = np.array(table, dtype=np.float64, order="C")
            if table.ndim not in (2, 3) or table.shape[-1] < 1:
                raise ValueError("table: [N, W] or [B, N, W] with W >= 1")
            if table.shape[-1] > capi.USER_MAX_TAB:
                raise capi.IslsError(f"a user {noun}'s table holds at most {capi.USER_MAX_TAB} words per step, got {table.shape[-1]}")
            self._table, self._table_version = table, 0
        self._params = np.atleast_1d(np.asarray(params, dtype=np.float64))
        if self._params.ndim > 2:
            raise ValueError("params: [P] or [B, P]")
        P = self._params.shape[-1]
        if P > capi.USER_MAX_PAR:
            raise capi.IslsError(f"a user {noun} takes at most {capi.USER_MAX_PAR} parameters, got {P}")
        if not capi.dims_supported(self.x_dim, self.u_dim):
            raise capi.IslsError(f"user {noun}s need one of the (x_dim, u_dim) pairs with the row-per-lane kernels "
                                 f"{capi.supported_dims()}, got ({self.x_dim}, {self.u_dim})")
        if re.search(r"\b(asm|__asm|__asm__)\b", source) or "__builtin_amdgcn" in source:
            raise capi.IslsError(f"a user {noun} is plain arithmetic: `asm` and `__builtin_amdgcn_*` are not accepted")
        self.source = source
        if field is not None:                                # (C, nx, ny): a cost of its own registration, which owns the field's buffers
            return create(source, self.x_dim, self.u_dim, P, self.n_tab + (K + 1 if K else 0), K, field=field)
        if K:
            return create(source, self.x_dim, self.u_dim, P, self.n_tab + K + 1, K)
        if table is not None:
            return create(source, self.x_dim, self.u_dim, P, table.shape[-1])
        return create(source, self.x_dim, self.u_dim, P)

    def params(self):
        return self._params

    @property
    def table(self):
        """The host copy of the per-step table ([N, W] or [B, N, W]; None: a source without one)."""
        return self._table

    def set_table(self, table):
        """New values for the table, of the shape it has: the next call of a solver on any iSLS holding this object uses them --
        no compile, and the engine copies them into the device buffer it already has."""
        if self._table is None:
            raise ValueError(f"set_table: this {self._noun} was built without a table")
        table = np.array(table, dtype=np.float64, order="C")
        if table.shape != self._table.shape:
            cls = "costs.Custom" if self._noun == "cost" else "Custom"
            raise ValueError(f"set_table: the table is {self._table.shape}, got {table.shape} (a new shape is a new {cls})")
        self._table, self._table_version = table, self._table_version + 1

    @property
    def n_tab(self):
        """Words per step of the table (0: none)."""
        return 0 if self._table is None else int(self._table.shape[-1])

    def _on_device(self, rows, need, *arrays, par=None):
        """(torch, kernels, device, [parameters, *arrays] as fp64 device tensors) for an evaluation of `rows` trajectories on the
        current device, the module put there by _load(); per-trajectory parameters need one row each (`need`: the error's words).
        `par`: the buffer that goes in the parameters' place (a table model's device_params, which has made these checks)."""
        import torch
        from .engine import kernels
        if par is None:
            par, tab = self._params, self._table
            if par.ndim == 2 and par.shape[0] != rows:
                raise ValueError(f"per-trajectory params [{par.shape[0]}, P] need " + need.format(par.shape[0], rows))
            if tab is not None and tab.ndim == 3 and tab.shape[0] != rows:
                raise ValueError(f"a per-trajectory table [{tab.shape[0]}, N, W] needs " + need.format(tab.shape[0], rows))
        dev = torch.device("cuda", torch.cuda.current_device())
        self._load(np.float64)
        return torch, kernels(), dev, [torch.as_tensor(np.array(a, dtype=np.float64, order="C"), device=dev) for a in (par,) + arrays]


class Custom(UserSource, Model):
    """A forward model of the user's own: `source` defines

        template <typename S, typename P>
        __device__ void step(const S *x, const S *u, const P *par, S *xn);

    in plain arithmetic on S (`+ - * /`, comparisons, sin cos sqrt exp log tanh asin atan2 fabs, isls::sin_cos, isls::py_mod:
    the contract of csrc/user_model_ad.hpp).  The library compiles it at run time for gfx950 (hiprtc) into the rollout kernel of
    the built-in models, the dense closed loop, a row-wise step and a linearisation on forward-mode dual numbers -- A, B come
    from `step` itself, there is no get_AB to write.  `params` is [P] (shared) or [B, P] (one row per trajectory), P <= 16.
    Only the (x_dim, u_dim) pairs with the row-per-lane kernels are served (`isls._capi.supported_dims()`).

    Per-step data (a payload dropped at step 40, a wind forecast, a variable time step, a mode schedule, x+ = A_t x + B_t u):
    `table` is [N, W] (shared by the batch) or [B, N, W] (one per trajectory), 1 <= W <= 16, and `source` then defines the
    five-argument form

        template <typename S, typename P>
        __device__ void step(const S *x, const S *u, const P *par, const P *row, S *xn);

    `row` the W words of step t: plain P, never differentiated.  `set_table` replaces the values (same shape) between two calls of
    a solver -- a receding-horizon window, a new forecast: no compile, one copy into the buffer the engine holds.  On the device
    the table rides behind the parameters, [par | row 0 | ... | row N-1] (`device_params`; include/isls_hip.h).  Such a model is
    linearised at every iteration.  Served: solve / iterate_once_dp / solve_ilqr / ilqr_admm, mpc (model_table_future=,
    plant_table=) and sample_nominal; monte_carlo, isls_admm and the dense closed loop refuse it."""

    def __init__(self, x_dim, u_dim, params, source, table=None, field=None):
        if field is not None:
            raise ValueError("field=: a 2-D field belongs to a cost (costs.Custom(field=)); a forward model cannot read one")
        par, tab = np.atleast_1d(np.asarray(params)), None if table is None else np.asarray(table)
        if tab is not None and par.ndim == 2 and tab.ndim == 3 and tab.shape[0] != par.shape[0]:
            raise ValueError(f"per-trajectory params [{par.shape[0]}, P] and a per-trajectory table [{tab.shape[0]}, N, W]: "
                             "one row and one table per trajectory")
        self.model_id = self._register("model", capi.user_model_create, x_dim, u_dim, params, source, table=table)

    def device_params(self, batch=None, N=None, table=None):
        """The buffer a launch names as the model's parameters: params() for a model without a table, else [P + N W] (shared
        parameters and a shared table) or [batch, P + N W] -- [par | row 0 | ... | row N-1], a shared part replicated where the
        other is per trajectory.  `table`: another table of the same form in the object's place (a plant's)."""
        tab = self._table if table is None else np.asarray(table, dtype=np.float64)
        if tab is None:
            return self._params
        par = self._params
        if N is not None and tab.shape[-2] != N:
            raise ValueError(f"the model's table has {tab.shape[-2]} steps, the horizon {N}")
        rows = par.shape[0] if par.ndim == 2 else (tab.shape[0] if tab.ndim == 3 else None)
        if rows is None:
            return np.concatenate([par, tab.reshape(-1)])
        if batch is not None and rows != batch:
            raise ValueError(f"per-trajectory params / table of {rows} trajectories, the batch has {batch}")
        if tab.ndim == 3 and tab.shape[0] != rows:
            raise ValueError(f"a per-trajectory table [{tab.shape[0]}, N, W] needs {tab.shape[0]} trajectories, got {rows}")
        return np.concatenate([np.broadcast_to(par, (rows, par.shape[-1])), np.broadcast_to(tab, (rows,) + tab.shape[-2:]).reshape(rows, -1)], axis=1)

    def code(self, dtype=np.float64):
        """The gfx950 code object of the model (all its kernels) for dtype."""
        return capi.user_model_code(self.model_id, dtype)

    def _load(self, dtype):
        capi.user_model_load(self.model_id, dtype)

    def _call_table(self, x, u, t):
        """__call__ of a table model: trajectories [N, n] / [B, N, n] step with row t at step t; anything else needs t=."""
        tab, n, m = self._table, self.x_dim, self.u_dim
        N, per = tab.shape[-2], self._params.ndim == 2 or tab.ndim == 3
        lead = np.broadcast_shapes(x.shape[:-1], u.shape[:-1])
        R = int(np.prod(lead)) if lead else 1
        xs, us = np.broadcast_to(x, lead + (n,)).reshape(R, n), np.broadcast_to(u, lead + (m,)).reshape(R, m)
        if t is None:
            if len(lead) not in (1, 2) or lead[-1] != N:
                raise ValueError(f"a table model steps trajectories [{N}, n] / [B, {N}, n] with row t at step t; single rows need t=")
            run, groups, tix = N, R // N, None
        else:
            tix = np.ascontiguousarray(np.broadcast_to(np.asarray(t), lead).reshape(R), dtype=np.int32)
            if tix.size and (tix.min() < 0 or tix.max() >= N):
                raise ValueError(f"t: steps in [0, {N}), got [{tix.min()}, {tix.max()}]")
            run, groups = 1, R
        torch, kern, dev, (par, xs, us) = self._on_device(R, None, xs, us, par=self.device_params(groups if per else None, N))
        xn = torch.empty(R, n, dtype=torch.float64, device=dev)
        kern.user_model_step_tab(self.model_id, par, xs, us, xn, run, N, t=None if tix is None else torch.as_tensor(tix, device=dev),
                                 stream=torch.cuda.current_stream().cuda_stream)
        return xn.cpu().numpy().reshape(lead + (n,))

    def __call__(self, x, u, t=None):
        """x [..., n], u [..., m] -> f(x, u) [..., n] (numpy, fp64), evaluated on the device.  A table model: trajectories
        [N, n] / [B, N, n] use row t at step t; single rows take t= (an int or an int array broadcastable to the rows)."""
        x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
        if self._table is not None:
            return self._call_table(x, u, t)
        lead = np.broadcast_shapes(x.shape[:-1], u.shape[:-1])
        R = int(np.prod(lead)) if lead else 1
        torch, kern, dev, (par, xs, us) = self._on_device(R, "{0} rows of x, u, got {1}",
                                                           np.broadcast_to(x, lead + (self.x_dim,)).reshape(R, self.x_dim),
                                                           np.broadcast_to(u, lead + (self.u_dim,)).reshape(R, self.u_dim))
        xn = torch.empty(R, self.x_dim, dtype=torch.float64, device=dev)
        kern.user_model_step(self.model_id, par, xs, us, xn, stream=torch.cuda.current_stream().cuda_stream)
        return xn.cpu().numpy().reshape(lead + (self.x_dim,))

    def get_AB(self, x, u, t=None):
        """A [N,n,n], B [N,n,m] along x [N,n], u [N,m] in the reference's convention (or [Bt,N,...] for a batch), on the device
        by the same dual-number kernel the solver linearises with.  A table model: row t at step t; single rows x [n] / [R, n]
        take t= and give A [n,n] / [R,n,n]."""
        x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
        if self._table is not None:
            return self._get_AB_table(x, u, t)
        single = x.ndim == 2
        xb, ub = (x[None], u[None]) if single else (x, u)
        Bt, N = xb.shape[:2]
        torch, kern, dev, (par, xs, us) = self._on_device(Bt, "x, u of [{0}, N, .]", xb, ub)
        A = torch.zeros(Bt, N, self.x_dim, self.x_dim, dtype=torch.float64, device=dev)
        Bm = torch.zeros(Bt, N, self.x_dim, self.u_dim, dtype=torch.float64, device=dev)
        kern.linearize(self.model_id, par, xs, us, A, Bm, stream=torch.cuda.current_stream().cuda_stream)
        A, Bm = A.cpu().numpy(), Bm.cpu().numpy()
        return (A[0], Bm[0]) if single else (A, Bm)

    def _get_AB_table(self, x, u, t):
        tab, n, m = self._table, self.x_dim, self.u_dim
        N = tab.shape[-2]
        if t is not None:
            # single rows: each is a one-step trajectory whose table is row t of the model's, at step 0
            lead = np.broadcast_shapes(x.shape[:-1], u.shape[:-1])
            R = int(np.prod(lead)) if lead else 1
            tix = np.broadcast_to(np.asarray(t), lead).reshape(R).astype(np.int64)
            if tix.size and (tix.min() < 0 or tix.max() >= N):
                raise ValueError(f"t: steps in [0, {N}), got [{tix.min()}, {tix.max()}]")
            if tab.ndim == 3 and tab.shape[0] != R:
                raise ValueError(f"a per-trajectory table [{tab.shape[0]}, N, W] needs {tab.shape[0]} rows, got {R}")
            rows = tab[tix] if tab.ndim == 2 else tab[np.arange(R), tix]
            xb, ub = np.broadcast_to(x, lead + (n,)).reshape(R, 1, n), np.broadcast_to(u, lead + (m,)).reshape(R, 1, m)
            par = self.device_params(R, 1, table=rows[:, None, :])
            out = lambda a: a[:, 0].reshape(lead + a.shape[2:])   # noqa: E731
        else:
            if x.ndim not in (2, 3) or x.shape[-2] != N:
                raise ValueError(f"a table model linearises trajectories [{N}, n] / [B, {N}, n] with row t at step t; single rows need t=")
            single = x.ndim == 2
            xb, ub = (x[None], u[None]) if single else (x, u)
            par = self.device_params(xb.shape[0] if (self._params.ndim == 2 or tab.ndim == 3) else None, N)
            out = lambda a: a[0] if single else a                 # noqa: E731
        Bt, Nt = xb.shape[:2]
        torch, kern, dev, (par, xs, us) = self._on_device(Bt, None, xb, ub, par=par)
        A = torch.zeros(Bt, Nt, n, n, dtype=torch.float64, device=dev)
        Bm = torch.zeros(Bt, Nt, n, m, dtype=torch.float64, device=dev)
        kern.linearize(self.model_id, par, xs, us, A, Bm, stream=torch.cuda.current_stream().cuda_stream)
        return out(A.cpu().numpy()), out(Bm.cpu().numpy())
