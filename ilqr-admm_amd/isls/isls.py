"""Batched iLQR / DP-form iLQR-ADMM front end with the reference's `iSLS` class surface.

Reference: `iSLS` (isls/isls.py) + `iSLSBase` (isls/isls_base.py).  The public names, arguments and loop
semantics follow the reference (HEAD names plus the notebook-era aliases listed in SURVEY 8b); every
numerical step runs in the HIP kernels behind `engine.Engine`:

    backward_pass_DP  -> riccati_gain + riccati_ff           (isls/isls.py:229-308)
    rollout_DP        -> rollout_ls                          (isls/isls.py:310-334)
    iterate_once_dp   -> gain, ff, rollout_ls(NaN rule, acceptance test)   (isls/isls.py:336-374)
    ilqr_admm         -> DP form: ilqr_admm_outer + accept_step            (isls/isls.py:379-501, "TODO: add dp solution")
    isls_admm         -> DP form: gain + C x ff + columns_rollout + rollout_ls + columns_admm (isls/isls.py:503-712)
    backward_pass_batch / iterate_once_batch -> gain + ff + columns_rollout (column 0) + open-loop rollout_ls (isls.py:156-228)

Differences from the reference, all deliberate and documented in DESIGN.md: `ilqr_admm` uses the DP (Riccati)
solve instead of the dense batch-form least squares (identical iterates except the never-applied last control,
SURVEY 8a quirk i); forward models and costs are the built-in device implementations (`isls.models`, via-point
quadratic cost); status is per trajectory; nothing falls back to the CPU.
"""
import weakref

import numpy as np
import torch

from . import _capi as capi
from . import hostpath
from .admm import ADMM
from .base import ALPHAS, Base
from .engine import STATIC
from .models import Model
from .projections import Box, ConvexSets
from .robust import isls_admm as _isls_admm


class MpcResult:
    """What iSLS.mpc returns: x [B, T+1, n] measured states, u [B, T, m] applied controls, and per control step the cost,
    status bits and executed ADMM iterations [B, T] of the plan the control was taken from (numpy)."""

    def __init__(self, x, u, cost, status, admm_iters):
        self.x, self.u, self.cost, self.status, self.admm_iters = x, u, cost, status, admm_iters


class AlResult:
    """What iSLS.solve_al returns (numpy): viol [B, rounds] the violation max_t max_i max(0, g_i) of every trajectory after each
    round's solve (a trajectory that was already within tol_con keeps its last value), mu [B] the final penalties, rounds [B] the
    rounds each trajectory took part in, converged [B] (its last violation <= tol_con), cost [B] the final (augmented) cost."""

    def __init__(self, viol, mu, rounds, converged, cost):
        self.viol, self.mu, self.rounds, self.converged, self.cost = viol, mu, rounds, converged, cost


class iSLS(Base):
    def __init__(self, x_dim, u_dim, N, batch=1, dtype=np.float64, device="cuda"):
        super().__init__(x_dim, u_dim, N, batch=batch, dtype=dtype, device=device)
        self.alphas = ALPHAS.copy()                             # 10**linspace(0,-5,50), isls/isls_base.py:10-11
        self._forward_model = None
        self._cost_function = None
        self.cost_log = []
        self._K = self._k = None
        self._user_AB = False
        self._host_model = self._host_cost = False              # plain Python callables: the line search runs on the host

    @property
    def _dx_columns(self):
        """[d_x, phi_x] rows [B, N n, 1 + dim] of the last `isls_admm` x-step, copied from the device on first use"""
        if getattr(self, "_dx_columns_host", None) is None and getattr(self, "_dx_columns_dev", None) is not None:
            from .robust import ColumnSolver
            self._dx_columns_host = ColumnSolver.rows_to_host(self._dx_columns_dev)
        return getattr(self, "_dx_columns_host", None)

    # ---- setters / getters (isls/isls_base.py:74-158) ------------------------------------------------------
    @property
    def forward_model(self):
        return self._forward_model

    @forward_model.setter
    def forward_model(self, model):
        """An `isls.models` descriptor selects the device implementation of the rollout.  A plain callable
        `f(x[R,n], u[R,m]) -> [R,n]` (the reference's convention, isls/isls.py:153,332) is accepted too: the Riccati passes
        and the ADMM update stay on the GPU, the line-search rollouts go through the callable on the host (hostpath.py)."""
        if isinstance(model, Model):
            if model.x_dim != self.x_dim or model.u_dim != self.u_dim:
                raise ValueError("model dimensions do not match x_dim/u_dim")
            self._forward_model, self._host_model = model, False
            if getattr(model, "table", None) is not None:      # models.Custom(table=): [par | rows] is what the device reads
                self.engine.set_model(model.model_id, model.device_params(self.batch, self.N))
                self._model_table_version = model._table_version
            else:
                self.engine.set_model(model.model_id, model.params())
            return
        if not callable(model):
            raise TypeError("forward_model must be an isls.models descriptor or a callable f(x, u)")
        self._forward_model, self._host_model = model, True

    @property
    def cost_function(self):
        return self._cost_function if self._cost_function is not None else self.compute_cost

    @cost_function.setter
    def cost_function(self, function):
        """None -> the via-point quadratic cost of set_cost_variables; an `isls.costs` object (PseudoHuber, or a Custom cost of
        the user's own) -> that cost on the device, for the line search and for the expansion (the reference's cost_function / get_Cs pair)."""
        if function is None:
            self._release_constraint_cost()
            self._cost_function, self._host_cost = None, False
            return
        if hasattr(function, "cost_model") and hasattr(function, "x_dim") and (function.x_dim, function.u_dim) != (self.x_dim, self.u_dim):
            raise ValueError("cost dimensions do not match x_dim/u_dim")
        if getattr(function, "n_con", 0):
            # the multipliers are state of ONE device table: a second iSLS would see neither what solve_al leaves on the first
            # nor keep the object's host copies in step with its own
            owner = function._owner() if function._owner is not None else None
            if owner is not None and owner is not self:
                raise capi.IslsError("a cost with constraints (costs.Custom(constraints=)) belongs to one iSLS at a time: its "
                                     "multipliers live in that object's device table; build a second costs.Custom for a second iSLS, "
                                     "or assign the first one another cost_function first")
        self._release_constraint_cost()
        self._cost_function = function
        if hasattr(function, "cost_model"):
            self._host_cost = False
            if getattr(function, "field", None) is not None:   # costs.Custom(field=): its samples onto this device ahead of any launch
                function._push_field(self.engine.device)
                self._cost_field_version = function._field_version
            table = getattr(function, "table", None)           # costs.Custom(table=): per-step data of the user's stage
            if getattr(function, "n_con", 0):
                # costs.Custom(constraints=): the library's table [B, N, W + K + 1] = [user row | multipliers | penalty], one per
                # trajectory -- a shared table and shared parameters are replicated now that the batch is known
                par = function.params()
                if par.ndim == 1 and par.shape[0] > 0:
                    par = np.broadcast_to(par, (self.batch, par.shape[0]))
                self.engine.set_cost_model(function.cost_model, par, table=function._al_table(self.batch, self.N))
                function._owner = weakref.ref(self)
                self._cost_table_version, self._cost_mult_version = function._table_version, function._mult_version
            elif table is None:
                self.engine.set_cost_model(function.cost_model, function.params())
            else:
                self.engine.set_cost_model(function.cost_model, function.params(), table=table)
                self._cost_table_version = function._table_version
        elif callable(function):
            # the reference's `cost_function(x[L,N,n], u[L,N,m]) -> [L]` (isls.py:360): evaluated on the host for every
            # candidate of the line search; its expansion comes from the caller's get_Cs
            self._host_cost = True
        else:
            raise TypeError("cost_function must be None, an isls.costs object or a callable cost(x, u)")

    def _release_constraint_cost(self):
        """The cost with constraints this object holds, if any, is free for another iSLS"""
        f = self._cost_function
        if getattr(f, "n_con", 0) and f._owner is not None and f._owner() is self:
            f._owner = None

    def _sync_tables(self):
        """set_table on the model or on the cost since this object last looked: the new values go INTO the buffer the engine holds
        (one copy_, no compile, no allocation; cached argument blocks stay valid).  The model's rows first (update_model_table
        marks the linearisation stale), so that the cost of the nominal is then evaluated again with both in place."""
        if not self._host_model:
            self._sync_table(self._forward_model, "_model_table_version", self.engine.update_model_table)
        if not self._host_cost and getattr(self._cost_function, "n_con", 0):
            if self._sync_al_table():
                self.engine.evaluate_cost()
        elif not self._host_cost and self._sync_table(self._cost_function, "_cost_table_version", self.engine.update_cost_table):
            self.engine.evaluate_cost()
        # set_field on the cost: the new samples go INTO the buffers its registration owns on this device (no compile either)
        if not self._host_cost and getattr(self._cost_function, "field", None) is not None:
            f = self._cost_function
            f._push_field(self.engine.device)
            if f._field_version != self._cost_field_version:
                self._cost_field_version = f._field_version
                self.engine.evaluate_cost()

    def _sync_al_table(self):
        """The same for a cost with constraints, whose device table is [user row (W) | multipliers (K) | penalty]: set_table
        writes the user's columns only, reset_multipliers the others -- strided copy_ INTO the table the engine holds."""
        f, tab = self._cost_function, self.engine.cost_tab
        W, K, changed = f.n_tab, f.n_con, False
        if W and f._table_version != self._cost_table_version:
            tab[..., :W].copy_(self.engine._t(f.table))
            self._cost_table_version, changed = f._table_version, True
        if f._mult_version != self._cost_mult_version:
            if f._lam is None or f._lam.shape != (self.batch, self.N, K):
                f._al_table(self.batch, self.N)
            tab[..., W:W + K].copy_(self.engine._t(f._lam))
            tab[..., W + K].copy_(self.engine._t(f._mu)[:, None])
            self._cost_mult_version, changed = f._mult_version, True
        return changed

    def _refuse_constraints(self, what):
        """The entry points a costs.Custom(constraints=) is not served by"""
        if not self._host_cost and getattr(self._cost_function, "n_con", 0):
            raise capi.IslsError(f"{what} does not serve a cost with constraints (costs.Custom(constraints=)): its augmented Lagrangian "
                                 "runs in the device routes of solve / solve_al, ilqr_admm, mpc, sample_nominal and covariance")

    def _sync_table(self, obj, seen, update):
        """update(obj.table) if obj has a table whose version is not the one this object last saw (the attribute `seen`)"""
        if getattr(obj, "table", None) is None or obj._table_version == getattr(self, seen):
            return False
        update(obj.table)
        setattr(self, seen, obj._table_version)
        return True

    def _refuse_table_model(self, what):
        """The entry points a models.Custom(table=) is not served by: their kernels step the model with no notion of time."""
        if not self._host_model and getattr(self._forward_model, "table", None) is not None:
            raise capi.IslsError(f"{what} does not serve a model with a per-step table (models.Custom(table=)): fold the schedule into "
                                 "the state (a clock state that the step reads), or run the loop yourself with the model's "
                                 "__call__(x, u, t=)")

    @property
    def AB(self):
        return [self.A, self.B]

    @AB.setter
    def AB(self, value):
        """A [N,n,n] / [n,n] (or with a leading batch axis), B likewise: linearisation used by the next backward pass."""
        A, B = np.asarray(value[0], dtype=np.float64), np.asarray(value[1], dtype=np.float64)
        self.A, self.B = A, B
        e = self.engine
        # a linearisation of the same shape as the one in use is copied INTO the buffers the engine already holds: argument blocks
        # and captured HIP graphs (isls_admm) keep raw device pointers, and a get_AB callback delivers a fresh array per outer
        # iteration -- replacing the tensors would leave those pointers on freed memory (the engine drops its own cached blocks)
        for name, new in (("A", e._t(A)), ("Bm", e._t(B))):
            old = getattr(e, name)
            if old is not None and old.shape == new.shape and old.is_contiguous():
                old.copy_(new)
            else:
                setattr(e, name, new)
        e.ab_from_caller()                                      # written in place or not, a caller's A, B
        self._user_AB = True

    @property
    def nominal_values(self):
        return self.x_nom, self.u_nom

    @nominal_values.setter
    def nominal_values(self, value):
        e = self.engine
        self._sync_tables()
        if e.Qtab is None:                                      # no via-point cost (a callable cost only): a zero table
            e.set_quadratic_cost(np.zeros((1, self.x_dim)), np.zeros((1, self.x_dim, self.x_dim)), np.zeros(self.N, dtype=np.int32), 0.0)
        e.set_nominal(self._batched(value[0], 2), self._batched(value[1], 2))
        if self._host_cost:                                     # the nominal's cost through the caller's function
            self._refresh_host_cost(reset_history=True)
        self.cost_log.append(self.cost)

    def _refresh_host_cost(self, reset_history=False):
        e = self.engine
        e.cost.copy_(e._t(hostpath.nominal_cost(self)))
        if reset_history:
            e.cost_hist[:, 0] = e.cost

    @property
    def _host_ls(self):
        return self._host_model or self._host_cost

    def _line_search(self, L, flags=0, active=None):
        """Line search over alphas[:L]: the rollout kernel, or the host route when the model / cost is a Python callable."""
        if self._host_ls:
            self._refuse_constraints("the host route (a forward model given as a Python callable)")
            hostpath.line_search(self, L, flags, active)
        else:
            self.engine.rollout(L, flags=flags, active=active)

    @property
    def x_nom(self):
        return self._out(self.engine.xhat)

    @property
    def u_nom(self):
        return self._out(self.engine.uhat)

    @property
    def cost(self):
        self._sync_tables()
        c = self.engine.cost.detach().cpu().numpy()
        return float(c[0]) if self.batch == 1 else c

    @property
    def K(self):
        return self._out(self.engine.K)

    @property
    def k(self):
        return self._out(self.engine.k)

    @property
    def status(self):
        """Per-trajectory status bits (ISLS_ST_*): non-PD Quu, NaN cost, line search rejected."""
        return self.engine.status.cpu().numpy()

    @property
    def reg_mu(self):
        """Per-trajectory mu [B] of the regularisation in use (the `regularization=` of the last solver call; zeros without one)."""
        return self.engine.reg_mu.cpu().numpy()

    def _set_regularization(self, regularization):
        from .regularization import Regularization
        if regularization is not None and not isinstance(regularization, Regularization):
            raise TypeError("regularization must be an isls.Regularization or None")
        if regularization is not None or self.engine.reg is not None:
            self.engine.set_regularization(regularization)

    def reset(self):
        self.cost_log = []
        self.engine.status.zero_()
        self.engine.outer_active.fill_(1)

    def compute_cost(self, x, u=None):
        """(x-xd)'Q(x-xd) + u'Ru, no 1/2 (SLSBase.compute_cost, isls/sls_base.py:25-44) for arrays [.., N, n]."""
        x = np.asarray(x, dtype=np.float64)
        lead = x.shape[:-2]
        seq = self.seq
        zs = self.zs if self.zs.ndim == 2 else None
        if zs is None:
            raise NotImplementedError("compute_cost on host needs shared via-points; use .cost for per-trajectory targets")
        dx = x - zs[seq]
        c = np.einsum("...ti,tij,...tj->...", dx, self.Qs[seq], dx)
        if u is not None:
            u = np.asarray(u, dtype=np.float64)
            c = c + self.u_std * np.sum(u * u, axis=(-1, -2))
        return float(c) if lead == () else c

    # ---- DP iLQR kernels -----------------------------------------------------------------------------------
    def _linearize(self, get_AB):
        e = self.engine
        model = self._forward_model
        if get_AB is None or (getattr(get_AB, "__self__", None) is model and not self._host_model):
            if model is None or self._host_model:
                raise ValueError("set forward_model to an isls.models descriptor or pass get_AB (a callable forward model has no "
                                 "built-in linearisation)")
            if self._user_AB:                                   # restore the engine's own dense buffers
                z = lambda *s: torch.zeros(*s, dtype=e.dtype, device=e.device)   # noqa: E731
                e.A, e.Bm = z(e.B, e.N, e.n, e.n), z(e.B, e.N, e.n, e.m)
                self._user_AB = False
            e.linearize()
            return
        # user callback in the reference's convention (numpy, one trajectory): host round trip by design
        xs, us = e.xhat.cpu().numpy(), e.uhat.cpu().numpy()
        AB = [get_AB(xs[b], us[b]) for b in range(self.batch)]
        self.AB = np.stack([np.array(a[0]) for a in AB]), np.stack([np.array(a[1]) for a in AB])

    def _expand(self, Cts=None, cts=None):
        e = self.engine
        self._sync_tables()
        if Cts is None:
            if not e.user_cost:                                 # (a user cost's expansion writes Cux)
                e.Cux = None
            e.expand()
            return
        n = self.x_dim
        e.allow_shared_hessian = False                          # the caller's Hessians differ per trajectory
        Cts, cts = self._batched(Cts, 3), self._batched(cts, 2)
        e.Cxx.copy_(e._t(Cts[..., :n, :n])), e.Cuu.copy_(e._t(Cts[..., n:, n:]))
        e.Cux = e._t(Cts[..., n:, :n])
        e.c0x.copy_(e._t(cts[..., :n])), e.c0u.copy_(e._t(cts[..., n:]))

    def backward_pass_DP(self, Cts=None, cts=None):
        """Riccati recursion about the nominal (isls/isls.py:229-308).  Returns (K [N,m,n], k [N,m])."""
        if not self._user_AB:
            self._linearize(None)                               # built-in model: A_t, B_t along the current nominal
        self._expand(Cts, cts)
        self.engine.gain()
        self.engine.feedforward()
        return self.K, self.k

    def rollout_DP(self, K, k):
        """Closed-loop rollout of the candidates k[l] (isls/isls.py:310-334): returns (x_log [L,N,n], u_log [L,N,m])."""
        e = self.engine
        k = np.asarray(k, dtype=np.float64)                     # [L,N,m] (batch == 1) or [B,L,N,m]
        if self._host_model:
            if self.batch != 1:
                raise NotImplementedError("rollout_DP through a callable forward model: batch == 1")
            K = np.asarray(K, dtype=np.float64)
            xn, un, f = self.x_nom, self.u_nom, self._forward_model
            x = np.tile(xn[0], (k.shape[0], 1))
            x_log, u_log = np.zeros((k.shape[0], self.N, self.x_dim)), np.zeros((k.shape[0], self.N, self.u_dim))
            for i in range(self.N):
                u = (x - xn[i]) @ K[i].T + k[:, i] + un[i]
                u_log[:, i], x_log[:, i] = u, x
                x = np.asarray(f(x, u), dtype=np.float64)
            return x_log, u_log
        if k.ndim == 3 and self.batch > 1:
            k = np.broadcast_to(k[None], (self.batch,) + k.shape)
        Kt = e._t(self._batched(K, 3))
        xs, us = [], []
        one = torch.ones(1, dtype=e.dtype, device=e.device)
        for l in range(k.shape[-3]):
            kl = e._t(self._batched(k[l] if k.ndim == 3 else k[:, l], 2))
            e.kern.rollout_ls(e.model, e.model_par, Kt, kl, e.xhat, e.uhat, one, e.Qtab, e.ztab, e.seq, e.u_std, e.xx, e.xu,
                              q_nonzero=e.q_nonzero, stream=torch.cuda.current_stream().cuda_stream)
            xs.append(e.xx.cpu().numpy()), us.append(e.xu.cpu().numpy())
        x, u = np.stack(xs, axis=1), np.stack(us, axis=1)
        return (x[0], u[0]) if self.batch == 1 else (x, u)

    _KEEP = object()                                            # regularization=: leave the engine's setting (and its mu) as it is

    def iterate_once_dp(self, max_line_search=15, verbose=False, Cts=None, cts=None, _linearized=False, regularization=_KEEP):
        """Backward pass + line search over alphas[:max_line_search] with the NaN rule and the acceptance test
        (isls/isls.py:336-374).  Returns (fp_success, K, k); fp_success is a bool, or a bool array when batched.
        regularization: an `isls.Regularization` (mu restarts at mu_init) or None for the plain pass; not given: the setting of the
        last call stays, with its mu.  With one, a Quu that is not positive definite makes the gain pass run again with a raised
        mu instead of raising LinAlgError, and mu follows the verdict of the line search."""
        e = self.engine
        if regularization is not iSLS._KEEP:
            self._set_regularization(regularization)
        if not _linearized and not self._user_AB:
            self._linearize(None)
        self._expand(Cts, cts)
        if e.reg is not None:
            return self._iterate_once_dp_regularised(max_line_search, verbose)
        e.status.zero_()
        e.gain(active=e.outer_active)
        e.feedforward(active=e.outer_active)
        self._line_search(max_line_search, flags=capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST, active=e.outer_active)
        st = e.status.cpu().numpy()
        ok = (st & capi.ST_LS_REJECT) == 0
        if (st & capi.ST_NOT_PD).any():
            raise np.linalg.LinAlgError(f"Quu not positive definite for trajectories {np.nonzero(st & capi.ST_NOT_PD)[0].tolist()}")
        e.accept_x_step()                                       # rejected trajectories received their nominal back
        if self.batch == 1:
            if ok[0]:
                self.cost_log.append(self.cost)
            elif verbose:
                print("Forward pass failed with a cost of", float(e.cost_new[0]))
            return bool(ok[0]), self.K, self.k
        self.cost_log.append(self.cost)
        return ok, self.K, self.k

    def _iterate_once_dp_regularised(self, max_line_search, verbose):
        """iterate_once_dp with a regularisation: gain pass with retries; a trajectory at the end of the ladder stops (outer_active
        <- 0, ISLS_ST_NOT_PD | ISLS_ST_REG_MAX stay in its status), the others run the line search; then the schedule on its verdict."""
        e = self.engine
        e.status.mul_((e.outer_active == 0).to(torch.int32))    # the status of the trajectories still iterating restarts
        e.backward_pass_regularised(active=e.outer_active)
        e.outer_active.mul_(((e.status & capi.ST_NOT_PD) == 0).to(torch.int32))
        self._line_search(max_line_search, flags=capi.RO_NAN_TO_1E5 | capi.RO_ACCEPT_TEST, active=e.outer_active)
        e.reg_after_line_search(active=e.outer_active)
        st = e.status.cpu().numpy()
        ok = (st & (capi.ST_LS_REJECT | capi.ST_NOT_PD)) == 0
        e.accept_x_step()                                       # rejected trajectories received their nominal back
        if self.batch == 1:
            if ok[0]:
                self.cost_log.append(self.cost)
            elif verbose:
                print("Forward pass failed with a cost of", float(e.cost_new[0]))
            return bool(ok[0]), self.K, self.k
        self.cost_log.append(self.cost)
        return ok, self.K, self.k

    def solve(self, get_AB=None, get_Cs=None, is_dynamics_linear=False, is_cost_quadratic=False, method='dp',
              max_iter=100, max_line_search_iter=25, tol_fun=1e-5, tol_grad=1e-4, verbose=False, regularization=None):
        """iLQR outer loop with the reference's stop rules (isls/isls.py:54-132), per trajectory when batched.
        regularization: an `isls.Regularization`.  A Quu that is not positive definite then raises that trajectory's mu and
        repeats the gain pass instead of raising LinAlgError; a rejected line search raises mu and the trajectory goes on from its
        unchanged nominal instead of stopping; an accepted step lowers mu.  A trajectory stops when its step was accepted and
        small, or when its ladder ended (ISLS_ST_REG_MAX in `status`).  `reg_mu` holds the final mu."""
        if method not in ('dp', 'batch'):
            raise NotImplementedError("method must be 'dp' or 'batch' (the reference raises for 'sls' too, isls.py:121-122)")
        if regularization is not None and method == 'batch':
            raise capi.IslsError("solve(method='batch') does not serve a regularisation (its column passes have no such term); use method='dp'")
        self._set_regularization(regularization)
        self._sync_tables()
        e = self.engine
        e.outer_active.fill_(1)
        prev = np.atleast_1d(np.array(self.cost, dtype=np.float64)).copy()
        Cts = cts = None
        for i in range(max_iter):
            if verbose:
                print("Iteration", i)
            if not (is_dynamics_linear and i > 0):
                self._linearize(get_AB)
            Cts, cts = self._user_expansion(get_Cs) if not (is_cost_quadratic and i > 0) else (Cts, cts)
            if method == 'dp':
                ok, _, _ = self.iterate_once_dp(max_line_search=max_line_search_iter, verbose=verbose, Cts=Cts, cts=cts,
                                                _linearized=True)
            else:
                self._user_AB, keep = True, self._user_AB         # linearised above: backward_pass_batch must not redo it
                ok = self.iterate_once_batch(max_line_search=max_line_search_iter, Cts=Cts, cts=cts, verbose=verbose)
                self._user_AB = keep
            cur = np.atleast_1d(np.array(self.cost, dtype=np.float64))
            okv = np.atleast_1d(ok)
            act = e.outer_active.cpu().numpy().astype(bool)
            # reference: |diff(cost_log[-2:])| < tol_fun (a rejected step leaves cost_log untouched, so the test
            # is on the last two ACCEPTED costs), then `not fp_success`
            small = np.abs(cur - prev) < tol_fun
            if e.reg is not None:                               # a rejected trajectory goes on with a raised mu
                stop = act & ((okv & small) | ((e.status.cpu().numpy() & capi.ST_REG_MAX) != 0))
            else:
                stop = act & ((okv & small) | ~okv)
            prev = np.where(act & okv, cur, prev)
            act &= ~stop
            e.outer_active.copy_(torch.as_tensor(act.astype(np.int32), device=e.device))
            if not act.any():
                if verbose:
                    print("Converged / stopped at iteration", i + 1)
                break
        return None

    def _device_expansion(self, get_Cs):
        """True when the device expands the cost itself: no get_Cs, or the get_Cs of the isls.costs object on the device."""
        return get_Cs is None or (self._cost_function is not None and not self._host_cost and
                                  getattr(get_Cs, "__self__", None) is self._cost_function)

    def _user_expansion(self, get_Cs):
        """(Cts, cts) from the caller's derivative callback `cts, Cts = get_Cs(x_nom, u_nom)` (isls/isls.py:102), evaluated
        on the host per trajectory -- or (None, None) when the device expands the cost itself."""
        if self._device_expansion(get_Cs):
            if self._host_cost and get_Cs is None:
                raise ValueError("a callable cost_function needs get_Cs (its gradient / Hessian along the nominal)")
            return None, None
        return hostpath.expansion(self, get_Cs)

    def _check_get_Cs(self, get_Cs):
        if self._host_cost and get_Cs is None:
            raise ValueError("a callable cost_function needs get_Cs (its gradient / Hessian along the nominal)")

    def solve_ilqr(self, get_AB=None, max_ilqr_iter=100, max_line_search_iter=25, dp=True, verbose=False, **kw):
        """Notebook-era name (Car notebooks :254): iLQR with the quadratic cost set by set_cost_variables.  Further keywords
        (`regularization=` among them) go to `solve`."""
        return self.solve(get_AB, method='dp' if dp else 'batch', max_iter=max_ilqr_iter, max_line_search_iter=max_line_search_iter,
                          verbose=verbose, **kw)

    # ---- nonlinear path constraints by augmented Lagrangian ---------------------------------------------------
    def solve_al(self, max_outer=10, max_iter=20, tol_con=1e-4, mu0=1.0, phi=10.0, mu_max=1e8, eta=0.25, regularization=None,
                 **solve_keywords):
        """iLQR under the constraints g(x, u) <= 0 of a costs.Custom(constraints=) cost, by augmented Lagrangian.  mu0: lambda = 0
        and mu = mu0 to start with (None: go on from the multipliers that stand).  Per round: solve(max_iter=, regularization=,
        **solve_keywords) on the augmented cost; then one launch (isls_user_constraint_update_*) on the new nominal, for the
        trajectories whose last violation was above tol_con: viol = max_t max_i max(0, g_i), lambda <- max(0, lambda + mu g), and
        mu <- min(phi mu, mu_max) where viol > eta * (the violation one round before; +inf at the first); then one read of viol.
        Stops when every trajectory is within tol_con, or after max_outer rounds.  A trajectory within tol_con keeps its
        multipliers but is still re-solved with the batch.  At the end one evaluate-only launch on the returned nominal gives
        `converged` (so it is true of that nominal, whatever the later solves did to a trajectory that had been within tol_con;
        `viol` is the log of the rounds).  Afterwards the cost object's multipliers / penalty are the device's.  Returns an AlResult."""
        f, e = self._cost_function, self.engine
        if self._host_cost or f is None or not getattr(f, "n_con", 0):
            raise capi.IslsError("solve_al needs a costs.Custom(constraints=K) cost_function" +
                                 (": a cost given as a Python callable has no constraint the device could evaluate" if self._host_cost else ""))
        if self._host_model or e.model is None:
            raise capi.IslsError("solve_al runs on the device: set forward_model to an isls.models descriptor (models.Custom for a "
                                 "model of your own), not a Python callable")
        if solve_keywords.get("method", "dp") != "dp":
            self._refuse_constraints("the batch form (iterate_once_batch, solve(method='batch'))")
        if mu0 is not None:
            f.reset_multipliers(mu0)
        self._sync_tables()
        B = self.batch
        viol = torch.zeros(B, dtype=e.dtype, device=e.device)
        prev = torch.full((B,), float("inf"), dtype=e.dtype, device=e.device)
        act = torch.ones(B, dtype=torch.int32, device=e.device)
        log, rounds, on = np.zeros((B, 0)), np.zeros(B, dtype=np.int64), np.ones(B, dtype=bool)
        stream = torch.cuda.current_stream().cuda_stream
        for r in range(int(max_outer)):
            self.solve(max_iter=max_iter, regularization=regularization, **solve_keywords)
            e.kern.user_constraint_update(e.cost_model, e.cost_par, e.cost_tab, e.xhat, e.uhat, viol, prev, update=True, eta=eta,
                                          phi=phi, mu_max=mu_max, active=act, stream=stream)
            last = viol.cpu().numpy().astype(np.float64)        # the round's read (a trajectory left out keeps its last value)
            rounds += on
            log = np.concatenate([log, last[:, None]], axis=1)
            e.nominal_rewritten()                               # the nominal's cost under the new multipliers, as after the nominal_values setter
            if (last <= tol_con).all():
                break
            act.mul_((viol > tol_con).to(torch.int32))          # on the device: nothing is sent up
            on = on & (last > tol_con)
        # a trajectory that was within tol_con is still re-solved with the batch, and a solve that had stopped at max_iter can move
        # it afterwards: `converged` speaks of the nominal that is returned -- one evaluate-only launch (update = 0) on it
        final = torch.zeros(B, dtype=e.dtype, device=e.device)
        e.kern.user_constraint_update(e.cost_model, e.cost_par, e.cost_tab, e.xhat, e.uhat, final, prev.clone(), update=False,
                                      stream=stream)
        f._pull(e.cost_tab.cpu().numpy().astype(np.float64))
        return AlResult(log, f.penalty.copy(), rounds, final.cpu().numpy().astype(np.float64) <= tol_con,
                        np.atleast_1d(np.array(self.cost, dtype=np.float64)).copy())

    # ---- gradients of the nominal's cost ------------------------------------------------------------------------
    def gradient(self, wrt=("u", "x0"), as_tensors=False):
        """Gradients of J = `cost` of the current nominal by an adjoint sweep on the device (isls/gradient.py).  J is the sum of
        the stage costs along the nominal with x_0 given and x_{t+1} = f(x_t, u_t): for a costs.Custom(constraints=) it includes
        the augmented-Lagrangian terms at the multipliers that stand; ADMM's proximal terms are not part of it.
        wrt: any of "u", "x0", "cost_params", "model_params", "cost_table", "model_table".  Returns a Gradient with cost [B],
        costate [B, N, n] (lambda_t = dJ/dx_t along the dynamics) and, where asked for (else None), u [B, N, m], x0 [B, n] (=
        costate[:, 0]), cost_params [B, Pc], model_params [B, Pm], cost_table [B, N, Wc], model_table [B, N, Wm] (row N-1: 0, the
        last control steps nothing) -- numpy arrays, or torch tensors on the device with as_tensors=True.  Shared params [P] /
        tables [N, W] still give one gradient per trajectory: sum over the batch for the shared quantity's.
        What it is: the TOTAL derivative of J at FIXED controls, at whatever nominal stands.  At a converged unconstrained
        `solve` the envelope theorem makes it the derivative of the optimal cost as well; after `solve_al` it is the derivative
        of the Lagrangian at the multipliers that stand; under an active projection of `ilqr_admm` it is only the fixed-controls
        derivative.  Nothing more is promised: no derivative of the optimal trajectory, none with respect to the multipliers.
        "u", "x0" and the costate serve every device model and cost (built-in, Custom, the generic (x_dim, u_dim) pairs, a
        caller's A, B from the AB setter); the parameter / table entries need the models.Custom / costs.Custom they belong to, whose
        source must keep to the S contract of csrc/user_model_ad.hpp in what it does with `par` and `row` too (the gradient program
        is compiled on the first request; IslsError with the compile log otherwise).  IslsError for an unknown entry, a missing
        Custom object or table, or a model / cost given as a Python callable -- before anything is launched.
        The call linearises and expands about the nominal (A, B, c0x, c0u are rewritten, as every solver rewrites them first) and
        touches nothing else: gains, records, regularisation state, multipliers and the nominal stay as they are."""
        from .gradient import gradient
        return gradient(self, wrt, as_tensors)

    # ---- iLQR-ADMM (DP form) --------------------------------------------------------------------------------
    def ilqr_admm(self, get_AB=None, get_Cs=None, project_x=False, project_u=False, max_iter=20,
                  max_line_search_iter=20, max_admm_iter=20, rho_x=None, rho_u=None, alpha=1, tol=1e-3,
                  verbose=False, log=False, k_max=None, max_line_search=None, threshold=None, regularization=None):
        """Outer loop of isls/isls.py:420-499 with the Riccati (DP) inner solve.  Per outer iteration:
        linearise, expand, then max_admm_iter x [ff pass, line search over alphas[:max_line_search_iter] without
        acceptance test, z/lambda update] with lambda reset and z warm-started, nominal <- last x-step, and the
        stop rules |dcost| < 1e-3 / oscillation < 1e-3.  Returns the residual log of the last outer iteration."""
        if self._host_cost and get_Cs is None:
            raise ValueError("a callable cost_function needs get_Cs (its gradient / Hessian along the nominal)")
        self._sync_tables()
        max_iter = k_max if k_max is not None else max_iter
        L = max_line_search if max_line_search is not None else max_line_search_iter
        tol = threshold if threshold is not None else tol
        e = self.engine
        px, pu, host_proj = self._setup_admm(project_x, project_u, rho_x, rho_u, alpha)
        if host_proj:
            self._refuse_constraints("ilqr_admm through the host (a projection or a model given as a Python callable)")
        if regularization is not None and host_proj:
            raise capi.IslsError("ilqr_admm through the host (a projection or a model / cost given as a Python callable) does not serve "
                                 "a regularisation; use Box / ConvexSets projections and device models")
        # regularization: the gain pass of every outer iteration runs with its retry loop ahead of the driver (Engine.run_outer);
        # no schedule on the line search, which has no acceptance test here
        self._set_regularization(regularization)
        J = int(max_admm_iter)
        logbuf = torch.zeros(J, self.batch, 2, dtype=e.dtype, device=e.device)
        e.outer_active.fill_(1)
        logs = []
        for j in range(max_iter):
            self._linearize(get_AB)
            self._expand_regularised(get_Cs)
            if host_proj:
                logs = self._admm_host(px, pu, L, J, tol, alpha, verbose)
            else:
                e.build_outer(L, J, tol_abs=tol, tol_rel=tol, log=logbuf)
                e.run_outer()
                lb = logbuf.cpu().numpy()
                logs = [lb[i, 0] if self.batch == 1 else lb[i] for i in range(J)]
            e.accept_x_step(tol_cost=1e-3, tol_osc=1e-3)
            self.cost_log.append(self.cost)
            st = e.status.cpu().numpy()
            if e.reg is None and (st & capi.ST_NOT_PD).any():
                raise np.linalg.LinAlgError("Quu not positive definite")
            if verbose:
                print("Iteration number ", j, "iLQR cost: ", self.cost)
            if not bool(e.outer_active.any().item()):
                break
        # the reference's `logs` holds one [prim, dual] entry per EXECUTED ADMM iteration of the last outer
        # iteration; batched: all J rows (rows after a trajectory's own stop repeat its last residuals) and
        # `self.admm_iters` tells how many are real per trajectory
        self.admm_iters = e.admm_iters.cpu().numpy()
        return logs[:int(self.admm_iters[0])] if self.batch == 1 and not host_proj else logs

    # ---- receding-horizon control of the whole batch ----------------------------------------------------------------------
    def mpc(self, steps, iters=1, project_x=False, project_u=False, rho_x=None, rho_u=None, alpha=1, max_admm_iter=5,
            max_line_search_iter=20, tol=1e-3, plant_params=None, noise_scale=0.0, w=None, seed=0, feedback=True,
            warm_start_z=False, clip_u=None, table_future=None, regularization=None, model_table_future=None, plant_table=None):
        """Model-predictive control of every trajectory of the batch for `steps` control steps, with no host round trip per step.
        Per control step s: `iters` outer iterations of ilqr_admm's device route about the current plan (same stop rules per
        trajectory, tol_cost = tol_osc = 1e-3, same gain / feed-forward / line-search settings), then one launch
        (Engine.mpc_step, isls_mpc_step_*) applies the first control to the plant, moves the plan -- nominal, gains, the user
        cost's table -- up by one step with its last row held and rolls it out again from the measured state.  The next step's
        ADMM starts as a fresh ilqr_admm call would: z = 0, lambda = 0; warm_start_z=True keeps the moved z.
        The plant is the forward model with `plant_params` ([P] or [batch, P]; None: the model's own parameters) plus a
        disturbance: none, explicit w [batch, steps, n], or noise_scale (a number or [n]) o z drawn on the device with `seed`
        (the normals of monte_carlo at (seed, trajectory, sample 0, step)).  feedback=True: the moved gains K correct the plan for
        the measured state, False: the moved controls are rolled out open loop.  clip_u=(lo, hi) (numbers or [m]) clips the
        APPLIED control only.  table_future [steps, W] or [batch, steps, W] (a costs.Custom(table=) cost): row s enters the
        window as its last row after step s; without it the last row is held.  The via-point cost of set_cost_variables is
        horizon-relative: it is reused unchanged in every window (a via point at step t stays t steps ahead of the plant).
        A models.Custom(table=) model: its table is the window of a world-time table that the engine keeps on the device;
        model_table_future [steps, W] or [batch, steps, W] are the rows behind the window -- row s enters it as its last row after
        control step s, without it the last row is held -- and per control step the window inside the model's device buffer is
        refreshed with one device-to-device copy ahead of the re-roll.  The plant of step s steps with the window's row 0
        (world row s) and `plant_params`; plant_table [steps, W] or [batch, steps, W] supplies its own row s instead: a forecast
        against the truth.  Afterwards the model object's table is the last window.
        A ConvexSets with per-row tables (par_rows / b_rows: moving obstacles) follows the loop by the rows it has left from its
        row0: exactly N -- horizon-relative, it stays put as well; N + steps or more -- world time, its window moves up one row
        per control step (pointers in the descriptors, no device work) and the object's row0 is steps further on afterwards, so
        that a second call continues; anything between is an IslsError that asks for a padded table.  The object's row0 is
        written once, after the last step: if the call raises on the way (an IslsError of a launch; the LinAlgError on a status row
        comes after the last step and after row0 is written), the object still says where the call began, while the engine's descriptors stand where the loop stopped -- the next call builds its
        descriptors from the object's row0 again, so it repeats those rows and does not skip any.
        Returns an MpcResult: x [batch, steps+1, n] (the measured states, x[:, 0] the first), u [batch, steps, m] (the applied
        controls), cost, status, admm_iters [batch, steps] (of the plan each step was taken from).  They are read once, after
        the last step; then, with no regularisation, LinAlgError("Quu not positive definite") if any status row has
        ISLS_ST_NOT_PD.  x_nom, u_nom, K, k hold the last plan afterwards: covariance() and monte_carlo() work on it."""
        e = self.engine
        if self._host_ls or e.model is None:
            raise capi.IslsError("mpc runs on the device: set forward_model to an isls.models descriptor (models.Custom for a model of "
                                 "your own) and cost_function to an isls.costs object (costs.Custom for a cost of your own), not "
                                 "Python callables; a host-driven loop can use ilqr_admm and the nominal_values setter")
        if regularization is not None:
            raise capi.IslsError("mpc does not serve regularization=: its retry loop reads a counter on the host at every gain pass; "
                                 "use ilqr_admm(regularization=) in a loop of your own")
        T_, iters, B, N, n, m = int(steps), int(iters), self.batch, self.N, self.x_dim, self.u_dim
        if T_ < 1 or iters < 1:
            raise ValueError("mpc: steps >= 1 and iters >= 1")
        # per-row constraint sets (ConvexSets par_rows / b_rows): a table of exactly N rows from row0 is horizon-relative and
        # stays put, like the via-point cost; one of N + steps rows or more is in world time and its window moves up one row
        # per control step (Engine.advance_sets: pointers in the descriptors, no device work)
        moving = {}
        for blk, pr in (("x", project_x), ("u", project_u)):   # (checked ahead of any device work)
            if isinstance(pr, ConvexSets) and pr.per_row:
                left = pr.total_rows - pr.row0
                if left != N and left < N + T_:
                    raise capi.IslsError(f"project_{blk}: {left} rows of its per-row tables are left from row0 = {pr.row0}; {N} (the "
                                         f"horizon: sets that stay put in every window) or at least {N + T_} (the horizon + steps: "
                                         "sets in world time) are needed -- pad the table by repeating its last row")
                moving[blk] = left != N
        self._sync_tables()
        mtab = e.model_table                                   # a models.Custom(table=): the window [N, W] / [B, N, W] in model_par
        if mtab is None and (model_table_future is not None or plant_table is not None):
            raise capi.IslsError("model_table_future / plant_table belong to a models.Custom(table=) forward model")
        if table_future is not None and e.cost_tab is None:
            raise capi.IslsError("table_future is the future of a costs.Custom(table=) cost's table: set such a cost_function, or move "
                                 "the via points of set_cost_variables yourself")
        if w is not None and noise_scale is not None and np.any(np.asarray(noise_scale) != 0):
            raise ValueError("mpc: explicit w or noise_scale, not both")
        plant = None
        if plant_params is not None:
            pp = np.ascontiguousarray(plant_params, dtype=np.float64)
            P_ = e.model_par.shape[-1] - N * e.model_tab_w
            if pp.ndim not in (1, 2) or pp.shape[-1] != P_ or (pp.ndim == 2 and pp.shape[0] != B):
                raise capi.IslsError(f"plant_params: [{P_}] for every trajectory or [{B}, {P_}] (one row per trajectory), got "
                                     f"{pp.shape}")
            plant = e._t(pp)
        px, pu, host_proj = self._setup_admm(project_x, project_u, rho_x, rho_u, alpha)
        if host_proj:
            raise capi.IslsError("mpc runs on the device: project_x / project_u must be Box or ConvexSets, not Python callables; a "
                                 "host-driven loop can use ilqr_admm and the nominal_values setter")
        self._set_regularization(None)
        if e.Qtab is None:                                      # no via-point cost: a zero table (the nominal_values setter's rule)
            e.set_quadratic_cost(np.zeros((1, n)), np.zeros((1, n, n)), np.zeros(N, dtype=np.int32), 0.0)

        def vec(v, d):
            return None if v is None else e._t(np.broadcast_to(np.asarray(v, dtype=np.float64), (d,)).copy())
        u_lo, u_hi = (None, None) if clip_u is None else (vec(clip_u[0], m), vec(clip_u[1], m))
        noise_std = vec(noise_scale, n) if (w is None and noise_scale is not None and np.any(np.asarray(noise_scale) != 0)) else None
        if w is not None:                                       # [steps, batch, n]: a step's rows are one dense block
            w = e._t(w)
            if tuple(w.shape) != (B, T_, n):
                raise ValueError(f"w: [{B}, {T_}, {n}], got {tuple(w.shape)}")
            w = w.permute(1, 0, 2).contiguous()
        n_con = 0 if self._host_cost else getattr(self._cost_function, "n_con", 0)
        if n_con and table_future is not None and self._cost_function.n_tab == 0:
            raise capi.IslsError("table_future supplies the user's columns of the cost's table: this cost has none (its table "
                                 "holds the multipliers only, which move up with the window)")
        if table_future is not None:
            # (a cost with constraints: the user's columns only -- the multipliers and mu of the held last row ride behind them)
            W, per_traj = int(e.cost_tab.shape[-1]) - (n_con + 1 if n_con else 0), e.cost_tab.ndim == 3
            if n_con and np.ndim(table_future) == 3 and self._cost_function.table.ndim == 2:
                # (the device table of such a cost is per trajectory for its multipliers' sake, but the object's table is one for
                # the batch: per-trajectory futures would leave windows that the object cannot hold afterwards)
                raise ValueError(f"table_future: [{T_}, {W}] (the cost's table is shared by the batch)")
            tf = e._t(table_future)
            if tuple(tf.shape) not in ((T_, W), (B, T_, W)) or (tf.ndim == 3 and not per_traj):
                raise ValueError(f"table_future: [{T_}, {W}]" + (f" or [{B}, {T_}, {W}]" if per_traj else " (the table is shared)") +
                                 f", got {tuple(tf.shape)}")
            if per_traj:
                tf = (tf if tf.ndim == 3 else tf.unsqueeze(0).expand(B, T_, W)).permute(1, 0, 2).contiguous()
            table_future = tf
        world = plants = None
        if mtab is not None:
            # the world-time table [.., N + steps, W] on the device, and every step's plant buffer [par | its row]: built once
            W, MP = e.model_tab_w, e.model_par.shape[-1] - N * e.model_tab_w

            def rows(v, name):
                if v is None:
                    return None
                v = e._t(v)
                if tuple(v.shape) not in ((T_, W), (B, T_, W)):
                    raise ValueError(f"{name}: [{T_}, {W}] or [{B}, {T_}, {W}], got {tuple(v.shape)}")
                return v
            fut, ptab = rows(model_table_future, "model_table_future"), rows(plant_table, "plant_table")
            if fut is not None and fut.ndim == 3 and self._forward_model.table.ndim == 2:
                # (with per-trajectory parameters the engine's window is [B, N, W], but the object's table is one for the batch:
                # per-trajectory futures would leave windows that the object cannot hold afterwards)
                raise ValueError(f"model_table_future: [{T_}, {W}] (the model's table is shared by the batch)")
            if fut is None:
                fut = mtab[..., -1:, :].expand(*mtab.shape[:-2], T_, W)
            elif fut.ndim < mtab.ndim:
                fut = fut.unsqueeze(0).expand(B, T_, W)
            world = torch.cat([mtab, fut], dim=-2).contiguous()
            prow = world[..., :T_, :] if ptab is None else ptab                  # the plant's row of step s
            ppar = e.model_par[..., :MP] if plant is None else plant
            per = prow.ndim == 3 or ppar.ndim == 2
            if per:
                prow = (prow if prow.ndim == 3 else prow.unsqueeze(0).expand(B, T_, W)).permute(1, 0, 2)
                plants = torch.cat([(ppar if ppar.ndim == 2 else ppar.unsqueeze(0).expand(B, MP)).unsqueeze(0).expand(T_, B, MP), prow], dim=-1)
            else:
                plants = torch.cat([ppar.unsqueeze(0).expand(T_, MP), prow], dim=-1)
            plants = plants.contiguous()
        L, J = int(max_line_search_iter), int(max_admm_iter)
        z = lambda *s_, dt=e.dtype: torch.zeros(*s_, dtype=dt, device=e.device)   # noqa: E731
        x_log, u_log, cost_log = z(B, T_ + 1, n), z(B, T_, m), z(B, T_)
        st_log, it_log = z(B, T_, dt=torch.int32), z(B, T_, dt=torch.int32)
        logbuf = z(J, B, 2)
        e.outer_active.fill_(1)
        e._outer_args, fused = None, False
        for s in range(T_):                                    # nothing below reads the device
            for it in range(iters):
                if it == 0 or not fused:
                    if e._ab_src != STATIC or self._user_AB:    # a state-independent model keeps its one linearisation
                        self._linearize(None)
                    self._expand_regularised(None)
                if e._outer_args is None:
                    e.build_outer(L, J, tol_abs=tol, tol_rel=tol, log=logbuf)
                    # between two outer iterations of a step, Engine.advance where it serves the cost's Hessians
                    fused = e.user_cost or e._shared_hessian()
                e.run_outer()
                if it == iters - 1:
                    it_log[:, s].copy_(e.admm_iters)
                    e.accept_x_step(tol_cost=1e-3, tol_osc=1e-3)
                elif fused:
                    e.advance(tol_cost=1e-3, tol_osc=1e-3)
                else:
                    e.accept_x_step(tol_cost=1e-3, tol_osc=1e-3)
            cost_log[:, s].copy_(e.cost)
            st_log[:, s].copy_(e.status)
            if world is not None:                              # the window moves up: one device-to-device copy INTO model_par
                mtab.copy_(world[..., s + 1:s + 1 + N, :])
            e.mpc_step(plant_par=plant if plants is None else plants[s], u_lo=u_lo, u_hi=u_hi, w=None if w is None else w[s], noise_std=noise_std, seed=seed, step=s,
                       feedback=feedback, shift_z=warm_start_z,
                       tab_next=None if table_future is None else table_future[s] if not n_con else
                       torch.cat([table_future[s], e.cost_tab[:, -1, -(n_con + 1):]], dim=-1),
                       x_meas_out=x_log[:, s], u_out=u_log[:, s], x_next_out=x_log[:, s + 1])
            if any(moving.values()):
                e.advance_sets(1, x=moving.get("x", False), u=moving.get("u", False))
            if not warm_start_z:
                for zz in (e.zx, e.zu):
                    if zz is not None:
                        zz.zero_()
        f = self._cost_function
        if n_con:                                               # the cost object follows the window the engine holds now
            full = e.cost_tab.cpu().numpy().astype(np.float64)
            f._pull(full)
            if f.n_tab:
                f._table = np.ascontiguousarray(full[..., :f.n_tab] if f._table.ndim == 3 else full[0, :, :f.n_tab])
        elif getattr(f, "table", None) is not None:
            f._table = e.cost_tab.cpu().numpy().astype(np.float64)
        if mtab is not None:                                    # ... and so does the model object
            mdl = self._forward_model
            last = mtab.cpu().numpy().astype(np.float64)
            mdl._table = np.ascontiguousarray(last if last.ndim == mdl._table.ndim else last[0])
        for blk, pr in (("x", px), ("u", pu)):                  # ... and the sets' objects the rows consumed
            if moving.get(blk):
                pr.advance(T_)
        r = MpcResult(x_log.cpu().numpy(), u_log.cpu().numpy(), cost_log.cpu().numpy(), st_log.cpu().numpy(), it_log.cpu().numpy())
        self.admm_iters = r.admm_iters[:, -1].copy()
        self.cost_log.append(self.cost)
        if (r.status & capi.ST_NOT_PD).any():
            raise np.linalg.LinAlgError("Quu not positive definite")
        return r

    def _setup_admm(self, project_x, project_u, rho_x, rho_u, alpha):
        """project_x / project_u of an ilqr_admm call -> the engine's ADMM state (weights, boxes or device sets, z / lambda
        buffers); returns (px, pu, host_proj): the projections as objects and whether the z-step runs through the host."""
        e = self.engine
        px, pu = self._projection(project_x, self.x_dim), self._projection(project_u, self.u_dim)
        on_device = (Box, ConvexSets)
        host_proj = (px is not None and not isinstance(px, on_device)) or (pu is not None and not isinstance(pu, on_device))
        host_proj = host_proj or self._host_ls                  # a host line search: the whole ADMM loop is host driven
        xs = px if isinstance(px, ConvexSets) and not host_proj else None
        us = pu if isinstance(pu, ConvexSets) and not host_proj else None
        xb = px.bounds(self.N, self.x_dim) if isinstance(px, Box) else ((-np.inf, np.inf) if px is not None and xs is None else None)
        ub = pu.bounds(self.N, self.u_dim) if isinstance(pu, Box) else ((-np.inf, np.inf) if pu is not None and us is None else None)
        e.set_admm(rho_x=rho_x if px is not None else None, rho_u=rho_u if pu is not None else None,
                   x_box=xb, u_box=ub, relax=alpha, x_sets=xs, u_sets=us)
        return px, pu, host_proj

    def _expand_regularised(self, get_Cs):
        """Quadratic expansion about the nominal plus the ADMM regulariser's Hessians: on the device for the built-in costs,
        from the caller's get_Cs otherwise (gradients of the regulariser are added by the feed-forward pass either way)."""
        e = self.engine
        if self._device_expansion(get_Cs):
            if not e.user_cost:                                 # (a user cost's expansion writes Cux)
                e.Cux = None
            e.expand()
            return
        Cts, cts = hostpath.expansion(self, get_Cs)
        self._expand(Cts, cts)
        if e.Qr is not None:
            e.Cxx.add_(2.0 * (e.Qr if e.Qr.ndim == 4 else e.Qr.unsqueeze(0)))
        if e.Rr is not None:
            e.Cuu.add_(2.0 * (e.Rr if e.Rr.ndim == 4 else e.Rr.unsqueeze(0)))

    def _admm_host(self, px, pu, L, J, tol, alpha, verbose):
        """Generic route for projections without a device kernel: x-step on the GPU, z-step through the caller's
        numpy functions, one trajectory at a time (isls/admm.py semantics via `isls.admm.ADMM`)."""
        e = self.engine
        B, N, n, m = self.batch, self.N, self.x_dim, self.u_dim
        e.gain()
        res = []
        # the B trajectories advance in lock-step: every ADMM iteration launches the batched x-step once;
        # lambda restarts at zero and z is warm-started from the previous outer iteration (isls.py:414-417,489-490)
        z_x = e.zx.cpu().numpy().reshape(B, -1).copy() if e.zx is not None else None
        z_u = e.zu.cpu().numpy().reshape(B, -1).copy() if e.zu is not None else None
        l_x = np.zeros_like(z_x) if z_x is not None else None
        l_u = np.zeros_like(z_u) if z_u is not None else None
        prev = np.full((B, 2), 1e6)
        active = np.ones(B, dtype=bool)
        for it in range(J):
            if z_x is not None:
                e.zx.copy_(e._t(z_x.reshape(B, N, n))), e.lx.copy_(e._t(l_x.reshape(B, N, n)))
            if z_u is not None:
                e.zu.copy_(e._t(z_u.reshape(B, N, m))), e.lu.copy_(e._t(l_u.reshape(B, N, m)))
            act_t = torch.as_tensor(active.astype(np.int32), device=e.device)
            e.feedforward(active=act_t)
            self._line_search(L, active=act_t)
            xx, xu = e.xx.cpu().numpy().reshape(B, -1), e.xu.cpu().numpy().reshape(B, -1)
            cur = np.zeros((B, 2))
            for b in range(B):
                if not active[b]:
                    cur[b] = prev[b]
                    continue
                prim = dual = 0.0
                for z, l, x, proj in ((z_x, l_x, xx, px), (z_u, l_u, xu, pu)):
                    if z is None:
                        continue
                    fn = proj if not isinstance(proj, Box) else proj.__call__
                    z_new = np.asarray(fn(alpha * x[b] + (1 - alpha) * z[b] + l[b]), dtype=np.float64).reshape(-1)
                    r = x[b] - z_new
                    l[b] += r
                    prim += np.linalg.norm(r)
                    dual += np.linalg.norm(z_new - z[b])
                    z[b] = z_new
                cur[b] = prim, dual
                stop = (prim < tol and dual < tol) or (abs(prev[b, 0] - prim) / (prev[b, 0] + 1e-30) < tol and
                                                       abs(prev[b, 1] - dual) / (prev[b, 1] + 1e-30) < tol)
                prev[b] = prim, dual
                if stop:
                    active[b] = False
            res.append(cur[0].copy() if B == 1 else cur.copy())
            if not active.any():
                break
        if z_x is not None:
            e.zx.copy_(e._t(z_x.reshape(B, N, n))), e.lx.copy_(e._t(l_x.reshape(B, N, n)))
        if z_u is not None:
            e.zu.copy_(e._t(z_u.reshape(B, N, m))), e.lu.copy_(e._t(l_u.reshape(B, N, m)))
        return res

    def isls_admm(self, *args, **kwargs):                       # isls/isls.py:503-712, DP form (robust.py)
        self._refuse_constraints("isls_admm")
        return _isls_admm(self, *args, **kwargs)

    isls_admm.__doc__ = _isls_admm.__doc__

    def controller(self, PHI_U, du):
        """K = Phi_u Phi_x^-1, k = (I - K Su) du with the dynamics of the last linearisation, engine.A / engine.Bm (notebook-era
        `iSLS.controller`, isls/sls.py:235-242 on `Base.AB`'s Sw / Su): all problems in one device synthesis
        (isls_sls_controller: block recursions through A_t, B_t instead of the dense transfer matrices and inverse), in fp64
        whatever the solver's dtype.  PHI_U [N m, N n] and du [N m] (problem 0's dynamics) or with a leading batch axis, numpy
        or torch tensors on the engine's device; numpy in gives numpy out, torch in gives device tensors.  Problems whose PHI_U
        is not causal (flagged in self.controller_flags) take the dense host route, sls_dense.controller."""
        from . import sls_dense as dense
        from .sls_controller import synthesize
        e = self.engine
        A, Bm = e.A.to(torch.float64), e.Bm.to(torch.float64)    # [B or 1, N or 1, n, n], [B or 1, N or 1, n, m]
        if (PHI_U.ndim if isinstance(PHI_U, torch.Tensor) else np.ndim(PHI_U)) == 2:
            A, Bm = A[:1], Bm[:1]

        def dense_one(b, P_, d_):
            Ab, Bb = A[min(b, A.shape[0] - 1)].cpu().numpy(), Bm[min(b, Bm.shape[0] - 1)].cpu().numpy()
            Sw, Su = dense.transfer_matrices_ltv(np.broadcast_to(Ab, (self.N,) + Ab.shape[-2:]),
                                                 np.broadcast_to(Bb, (self.N,) + Bb.shape[-2:]))
            return dense.controller(Sw, Su, P_, d_)
        K, k, self.controller_flags = synthesize(e, A, Bm, PHI_U, du, dense_one)
        if self.batch == 1 and K.ndim == 3:                     # one problem: unbatched results, as the host route returned them
            K, k = K[0], k[0]
        return K, k

    def get_trajectory_sls(self, x0, K, k, noise_scale=0, problem=0):
        """Monte-Carlo closed loop of the dense controller about the nominal of problem `problem` through the forward model
        (isls/isls_base.py:28-42): x0 [M, n] -> (x_log [M,N,n], u_log [M,N,m]); one device thread per initial state."""
        e = self.engine
        self._refuse_table_model("get_trajectory_sls (the dense closed loop)")
        if noise_scale or self._host_model:
            # process noise comes from numpy's global generator, one draw per step in the reference's order: host loop
            # through the (numpy-callable) forward model, isls/isls_base.py:28-42
            K, k = hostpath.as_numpy(K), hostpath.as_numpy(k)
            xn, un = e.xhat[problem].cpu().numpy().astype(np.float64), e.uhat[problem].cpu().numpy().astype(np.float64)
            n, m = self.x_dim, self.u_dim

            def control(i, x_log):
                xv = np.zeros((x_log.shape[0], self.N * n))
                xv[:, :(i + 1) * n] = (x_log[:, :i + 1] - xn[None, :i + 1]).reshape(x_log.shape[0], -1)
                return (xv @ K.T + k)[:, i * m:(i + 1) * m] + un[i]
            return hostpath.noisy_closed_loop(self._forward_model, x0, self.N, m, control, noise_scale)
        x0 = np.asarray(x0, dtype=np.float64)
        single = x0.ndim == 1
        x0 = np.atleast_2d(x0)
        M = x0.shape[0]
        dev = lambda a: e._t(np.ascontiguousarray(a))                           # noqa: E731
        par = e.model_par if e.model_par.ndim == 1 else e.model_par[problem].contiguous()
        x_log = torch.zeros(M, self.N, self.x_dim, dtype=e.dtype, device=e.device)
        u_log = torch.zeros(M, self.N, self.u_dim, dtype=e.dtype, device=e.device)
        e.kern.dense_closed_loop(e.model, par, e._t(K), e._t(k), dev(x0), x_log, u_log,
                                 xhat=e.xhat[problem].contiguous(), uhat=e.uhat[problem].contiguous(),
                                 stream=torch.cuda.current_stream().cuda_stream)
        x, u = x_log.cpu().numpy().astype(np.float64), u_log.cpu().numpy().astype(np.float64)
        return (x[0], u[0]) if single else (x, u)

    def monte_carlo(self, K, k, samples=None, x0=None, x0_std=None, noise_scale=0.0, seed=0, u_bounds=None, x_bounds=None,
                    return_trajectories=False, x0s=None, w=None, absolute=False, **chunks):
        """Monte-Carlo validation of every problem's controller in one launch (isls/montecarlo.py, isls_mc_closed_loop_*):
        `samples` closed loops of each of the `batch` problems about ITS OWN nominal through the forward model (a built-in
        descriptor or models.Custom), u_i = K dx + k + uhat_i with dx = x - xhat (absolute=True: u_i = K x + k, the form of
        get_trajectory_dp).  Initial states x0 + x0_std o z (x0 default: every problem's xhat_0) or explicit x0s [B,M,n];
        process noise noise_scale o z drawn on the device with `seed`, or explicit w [B,M,N,n].  K, k, the bounds and the
        result as in SLS.monte_carlo.  A forward model that is a Python callable is refused: no host loop stands behind this."""
        from . import montecarlo
        e = self.engine
        if self._host_model or e.model is None:
            raise capi.IslsError("monte_carlo runs on the device: set forward_model to an isls.models descriptor (models.Custom for a "
                                 "model of your own), not a Python callable")
        self._refuse_table_model("monte_carlo")
        xhat, uhat = (None, None) if absolute else (e.xhat, e.uhat)
        if x0 is None and x0s is None:
            x0 = e.xhat[:, 0].contiguous()
        return montecarlo.run(e, e.model, e.model_par, K, k, self.N, self.x_dim, self.u_dim, samples=samples, x0=x0, x0_std=x0_std,
                              x0s=x0s, noise_scale=noise_scale, w=w, seed=seed, u_bounds=u_bounds, x_bounds=x_bounds, xhat=xhat,
                              uhat=uhat, problems=self.batch, return_trajectories=return_trajectories, **chunks)

    def _sampling_gains(self):
        """The gains of sample_nominal(feedback=True): the backward pass about the nominal as it stands on the device -- linearise,
        expand, gain pass on the form that writes the K array (what backward_pass_DP runs) -- for every trajectory, with the
        engine's regularisation if it has one.  A Quu that stays not positive definite raises as iterate_once_dp does."""
        e = self.engine
        e.outer_active.fill_(1)
        e.status.zero_()
        if not self._user_AB:
            self._linearize(None)
        self._expand()
        e.gain()
        st = e.status.cpu().numpy()
        if (st & capi.ST_NOT_PD).any():
            raise np.linalg.LinAlgError(f"Quu not positive definite for trajectories {np.nonzero(st & capi.ST_NOT_PD)[0].tolist()}")
        return e.K

    def sample_nominal(self, samples=1024, sigma=0.5, temperature=1.0, rounds=1, seed=0, clip_u=None, return_costs=False,
                       feedback=None, regularization=_KEEP):
        """Sampling warm start of every problem's nominal on the device (isls/sampling.py, isls_sample_nominal_*): per round,
        `samples` open-loop rollouts from xhat_0 with controls uhat + sigma o z (sample 0: uhat itself; z drawn on the device
        with seed + round, the normals of monte_carlo at (seed, problem, sample, step); clip_u=(lo, hi), numbers or [m], clips
        them), each costed with the problem's own cost -- what `cost` means: the via-point cost, costs.PseudoHuber, or a
        costs.Custom with its table; a NaN counts as +inf.  The nominal moves to uhat + sum_s w_s (u_s - uhat) with
        w_s ~ exp(-(S_s - S_min) / (temperature max(S_min, tiny))), or to the best sample where that mean does not cost less:
        the nominal's cost never rises.  sigma: a number, [m] or [batch, m].  x_nom, u_nom are rewritten in place (x_nom[:, 0]
        stays), then cost, cost_log, status and the masks as the nominal_values setter leaves them.  Returns a SampleResult:
        cost_before, cost_after [batch], cost_best_sample, took_best, ess [batch, rounds] (+ costs [batch, samples] of the last
        round with return_costs=True), read once at the end.  IslsError: a forward model or cost that is a Python callable, an
        (x_dim, u_dim) outside the fast pairs, samples < 1, rounds < 1, temperature <= 0, a negative or non-finite sigma, lo > hi --
        all before anything is launched -- and, after the rounds (the other problems have moved, cost_log has its entry), a nominal
        whose own rollout has no finite cost: that problem is left as it is.

        feedback: the samples run in CLOSED LOOP about feedback gains (isls_sample_nominal_fb_*), u_s,t = clip((uhat_t +
        K_t (x_s,t - xhat_t)) + eps_s,t) with the same draws eps as the open-loop round of that seed: noise injected at step t is
        corrected at the steps behind it, which is what an unstable or strongly nonlinear plant needs.  The nominal moves to the
        closed-loop rollout of uhat + sum_s w_s eps_s (the weighted DRAWN noise) or to the best sample, and what is stored are the
        realised states and the realised, clipped controls: x_nom, u_nom are dynamically consistent and inside clip_u.
        feedback=None or False: the open-loop rounds above.  feedback=an array [N, m, n] or [batch, N, m, n] (numpy or torch; a
        torch tensor on the device is used in place): these gains in every round -- `q.sample_nominal(feedback=q.K)` after a solve;
        a wrong shape or a non-finite entry raises IslsError before anything is launched.  feedback=True: before EVERY round the
        backward pass about the current nominal (linearise, expand, gain pass: what backward_pass_DP runs) gives the gains, for
        every trajectory; the engine's K is overwritten, k is stale afterwards, and the status is read once per round.
        regularization (an `isls.Regularization` or None, as in `solve`; not given: the engine's setting stays) is the gain pass's:
        it is read with feedback=True only, every other form runs no gain pass and leaves the engine's setting and mu alone;
        without one, a Quu that is not positive definite raises np.linalg.LinAlgError as iterate_once_dp does -- in the first round
        before anything is sampled."""
        from . import sampling
        e = self.engine
        if self._host_ls or e.model is None:
            raise capi.IslsError("sample_nominal runs on the device: set forward_model to an isls.models descriptor (models.Custom for a "
                                 "model of your own) and cost_function to an isls.costs object (costs.Custom for a cost of your "
                                 "own), not Python callables")
        sampling.check_args(self.batch, self.u_dim, samples, sigma, temperature, rounds, clip_u, feedback, self.N, self.x_dim)
        if feedback is True:                                    # the only form that runs a gain pass: regularization= is its
            if regularization is not iSLS._KEEP:
                self._set_regularization(regularization)
            feedback = self._sampling_gains
        self._sync_tables()
        if e.Qtab is None:                                      # no via-point cost: a zero table (the nominal_values setter's rule)
            e.set_quadratic_cost(np.zeros((1, self.x_dim)), np.zeros((1, self.x_dim, self.x_dim)), np.zeros(self.N, dtype=np.int32), 0.0)
        try:
            return sampling.run(e, samples=samples, sigma=sigma, temperature=temperature, rounds=rounds, seed=seed, clip_u=clip_u,
                                return_costs=return_costs, feedback=feedback, feedback_checked=True)
        finally:                                                # also when a nominal without a finite cost raises: the others moved
            self.cost_log.append(self.cost)

    def covariance(self, K=None, k=None, x0=None, x0_std=None, x0_cov=None, noise_scale=0.0, noise_cov=None, u_bounds=None,
                   x_bounds=None, full=False):
        """Mean and covariance of every problem's closed loop, predicted without a sample (isls/covariance.py,
        isls_cov_closed_loop_*): the analytic counterpart of monte_carlo.  The loop is the LINEARISED one about the current
        nominal, Sig_{t+1} = (A_t + B_t K_t) Sig_t (A_t + B_t K_t)' + W_t, Su_t = K_t Sig_t K_t', with the engine's A, Bm: the
        caller's (get_AB / AB) where they are, else the forward model (an isls.models descriptor; models.Custom through its
        dual-number linearisation) is linearised first.  A forward model that is a Python callable is therefore served only with
        the caller's get_AB / AB; no roll-out is needed.  The nominal is ASSUMED dynamically consistent (xhat_{t+1} = f(xhat_t,
        uhat_t), as after solve / ilqr_admm): the mean is xhat + d with d_{t+1} = (A + B K) d_t + B k_t from d_0 = x0 - xhat_0.
        K [N,m,n] / [B,N,m,n], k (stage-local gains; default: the engine's own; a dense causal K is a ValueError); x0 [n] / [B,n]
        (default: xhat_0); x0_std / noise_scale: per-coordinate standard deviations as monte_carlo takes them, or x0_cov /
        noise_cov: full matrices [n,n], [B,n,n] (the noise also [B,N,n,n]) -- both forms of one quantity: ValueError; the noise
        acts behind step t as in monte_carlo.  u_bounds / x_bounds = (lo, hi) as in monte_carlo.  Returns a CovarianceResult:
        x_mean, u_mean, x_var, u_var, p_x, p_u (+ x_cov, u_cov with full=True); its tightened(lo, hi, psi_inv) is the box of
        ilqr_admm shrunk into a chance constraint."""
        from . import covariance
        e = self.engine
        if not self._user_AB:
            self._linearize(None)
        as_torch = isinstance(K, torch.Tensor)                   # the engine's own gains are no torch operand of the caller's
        K = e.K if K is None else K
        k = e.k if k is None else k
        dx0 = None
        if x0 is not None:
            dx0 = e._t(x0) - e.xhat[:, 0]
        return covariance.run(e, e.A, e.Bm, K, k, self.N, self.x_dim, self.u_dim, problems=self.batch, xhat=e.xhat, uhat=e.uhat,
                              dx0=dx0, x0_std=x0_std, x0_cov=x0_cov, noise_scale=noise_scale, noise_cov=noise_cov,
                              u_bounds=u_bounds, x_bounds=x_bounds, full=full, as_torch=as_torch)

    # ---- batch-form iLQR (isls/isls.py:135-228) through the Riccati kernels ---------------------------------------------
    def rollout_batch(self, x_nom, u_nom):
        """Open-loop rollouts from x_nom[0] (isls/isls.py:135-154): u_nom [L,N,m] (or [B,L,N,m]) -> (x_log, u_nom)."""
        e = self.engine
        u = np.asarray(u_nom, dtype=np.float64)
        ub = u if (self.batch > 1 and u.ndim == 4) else np.broadcast_to(u[None], (self.batch,) + u.shape)
        x0 = e._t(self._batched(np.asarray(x_nom, dtype=np.float64), 2)[:, 0].copy())
        zero_K = torch.zeros(self.batch, self.N, self.u_dim, self.x_dim, dtype=e.dtype, device=e.device)
        zero_u = torch.zeros(self.batch, self.N, self.u_dim, dtype=e.dtype, device=e.device)
        one = torch.ones(1, dtype=e.dtype, device=e.device)
        xs = []
        for l in range(ub.shape[1]):
            e.kern.rollout_ls(e.model, e.model_par, zero_K, e._t(np.ascontiguousarray(ub[:, l])), e.xhat, zero_u, one, e.Qtab, e.ztab,
                              e.seq, e.u_std, e.xx, e.xu, x0=x0, q_nonzero=e.q_nonzero, cost_model=e.cost_model, cost_par=e.cost_par,
                              cost_tab=e.cost_tab, stream=torch.cuda.current_stream().cuda_stream)
            xs.append(e.xx.cpu().numpy())
        x = np.stack(xs, axis=1)
        return (x[0] if self.batch == 1 else x), u

    def backward_pass_batch(self, Cts=None, cts=None):
        """delta_u_opt [N,m] of the batch-form least squares (isls/isls.py:156-189): the minimiser of the LQ sub-problem
        about the nominal, i.e. the Riccati solution rolled through the linearised dynamics, plus the dense form's last
        control (column 0 of isls_columns_rollout; SURVEY 8a quirk i)."""
        e = self.engine
        if e.reg is not None:
            raise capi.IslsError("the batch-form iLQR (backward_pass_batch, iterate_once_batch, solve(method='batch')) does not serve a "
                                 "regularisation; use method='dp'")
        if e.user_cost:
            # the column roll-out (isls_columns_rollout) takes Cuu alone: a user cost's x-u cross terms would be dropped
            raise capi.IslsError("the batch-form iLQR (backward_pass_batch, iterate_once_batch, solve(method='batch')) does not serve a "
                                 "user cost (costs.Custom): its column roll-out has no Cux term; use method='dp'")
        if not self._user_AB:
            self._linearize(None)
        self._expand(Cts, cts)
        e.gain()
        z = lambda *s_: torch.zeros(*s_, dtype=e.dtype, device=e.device)        # noqa: E731
        B, N, n, m = self.batch, self.N, self.x_dim, self.u_dim
        kcol, dx, du = z(2, B, N, m), z(2, B, N, n), z(2, B, N, m)
        e.kern.riccati_ff(e.A, e.Bm, e.c0x, e.c0u, e.K, e.Quu, e.fac, e.Qux, kcol[0], solve_mode=e.solve_mode,
                          stream=torch.cuda.current_stream().cuda_stream)
        e.kern.columns_rollout(e.A, e.Bm, e.hessians()[1], e.c0u, e.K, kcol, dx, du, stream=torch.cuda.current_stream().cuda_stream)
        self._du_batch = du[0]
        return self._out(du[0])

    def iterate_once_batch(self, verbose=False, max_line_search=15, **kwargs):
        """Batch-form backward pass + open-loop line search with the acceptance test costs[ind] < cost
        (isls/isls.py:191-225).  Returns fp_success (bool, or a bool array when batched)."""
        e = self.engine
        self._refuse_table_model("the batch form (iterate_once_batch, solve(method='batch'))")
        self._refuse_constraints("the batch form (iterate_once_batch, solve(method='batch'))")
        self.backward_pass_batch(**kwargs)
        zero_K = torch.zeros(self.batch, self.N, self.u_dim, self.x_dim, dtype=e.dtype, device=e.device)
        e.status.zero_()
        e.kern.rollout_ls(e.model, e.model_par, zero_K, self._du_batch, e.xhat, e.uhat, e.alphas[:max_line_search], e.Qtab, e.ztab,
                          e.seq, e.u_std, e.xx, e.xu, best=e.best, cost_new=e.cost_new, cost_cur=e.cost, flags=capi.RO_ACCEPT_TEST,
                          status=e.status, active=e.outer_active, q_nonzero=e.q_nonzero, cost_model=e.cost_model,
                          cost_par=e.cost_par, stream=torch.cuda.current_stream().cuda_stream)
        ok = (e.status.cpu().numpy() & capi.ST_LS_REJECT) == 0
        e.accept_x_step()
        if self.batch == 1:
            if ok[0]:
                self.cost_log.append(self.cost)
            return bool(ok[0])
        self.cost_log.append(self.cost)
        return ok

    # ---- closed-loop evaluation (isls/isls_base.py:28-71) -----------------------------------------------------
    def get_trajectory_batch(self, x0, us, noise_scale=0):
        """Open loop: the control sequence us [N,m] (or [B,N,m]) applied from x0 (isls/isls_base.py:44-57) -- the notebooks'
        way to turn initial controls into a nominal trajectory."""
        us = np.asarray(us, dtype=np.float64)
        return self.get_trajectory_dp(x0, np.zeros(us.shape[:-1] + (self.u_dim, self.x_dim)), us, noise_scale)

    def _transfer_ltv(self, problem=0):
        from . import sls_dense as dense
        A, Bm = self.engine.A.cpu().numpy().astype(np.float64), self.engine.Bm.cpu().numpy().astype(np.float64)
        b = min(problem, A.shape[0] - 1)
        return dense.transfer_matrices_ltv(np.broadcast_to(A[b], (self.N,) + A.shape[-2:]), np.broadcast_to(Bm[b], (self.N,) + Bm.shape[-2:]))

    # dense transfer matrices of the last linearisation (Base.AB's Sw / Su, isls/base.py:98-119; notebook-era names C / D):
    # host numpy, built on demand for problem 0 of the batch -- the solvers themselves never form them
    Sw = property(lambda self: self._transfer_ltv()[0])
    Su = property(lambda self: self._transfer_ltv()[1])
    C, D = Sw, Su

    def get_trajectory_dp(self, x0, K, k, noise_scale=0):
        """u_t = K_t x_t + k_t, x_{t+1} = f(x_t, u_t) from x0 (absolute form), noise-free only.  x0 [n] (or [B,n]): one
        trajectory per problem of the batch; x0 [M,n] with batch == 1: M initial states against the same controller."""
        e = self.engine
        if noise_scale or self._host_model:                          # isls/isls_base.py:59-71 on the host (see get_trajectory_sls)
            K, k = np.asarray(K, dtype=np.float64), np.asarray(k, dtype=np.float64)
            if K.ndim == 4 or k.ndim == 3:
                raise NotImplementedError("noisy / callable-model closed loops take one controller (K [N,m,n], k [N,m])")
            return hostpath.noisy_closed_loop(self._forward_model, x0, self.N, self.u_dim,
                                              lambda i, x_log: x_log[:, i] @ K[i].T + k[i], noise_scale)
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.ndim == 2 and self.batch == 1 and x0.shape[0] != 1:      # Monte Carlo over initial states: a batch of M rollouts
            mc = iSLS(self.x_dim, self.u_dim, self.N, batch=x0.shape[0], dtype=self.np_dtype, device=e.device)
            mc.forward_model = self._forward_model
            mc.engine.Qtab, mc.engine.ztab, mc.engine.seq, mc.engine.q_nonzero = e.Qtab, e.ztab, e.seq, e.q_nonzero
            mc.engine.u_std, mc.engine.cost_model, mc.engine.cost_par = e.u_std, e.cost_model, e.cost_par
            return mc.get_trajectory_dp(x0, K, k)
        x0 = self._batched(x0, 1)
        if e.Qtab is None:                                       # no cost yet (the notebooks roll the initial controls out first)
            e.set_quadratic_cost(np.zeros((1, self.x_dim)), np.zeros((1, self.x_dim, self.x_dim)), np.zeros(self.N, dtype=np.int32), 0.0)
        one = torch.ones(1, dtype=e.dtype, device=e.device)
        e.kern.rollout_ls(e.model, e.model_par, e._t(self._batched(K, 3)), e._t(self._batched(k, 2)), e.xhat, e.uhat, one,
                          e.Qtab, e.ztab, e.seq, e.u_std, e.xx, e.xu, x0=e._t(x0), flags=capi.RO_ABSOLUTE,
                          q_nonzero=e.q_nonzero, stream=torch.cuda.current_stream().cuda_stream)
        return self._out(e.xx), self._out(e.xu)
