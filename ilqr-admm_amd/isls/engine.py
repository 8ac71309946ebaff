"""Device-side state and kernel sequencing of the batched DP-form iLQR-ADMM solver.

`Engine` owns the HBM-resident arrays of B independent trajectories (torch tensors on one MI355X) and
drives the HIP kernels of csrc/ through the C ABI (include/isls_hip.h).  It is the batched counterpart
of the state the reference keeps on an `iSLS`/`SLS` object (x_nom, u_nom, A, B, K, k, cost, z, lambda:
isls/isls_base.py:4-27, isls/base.py:11-24) and of the bodies of `iSLS.ilqr_admm` (isls/isls.py:420-499)
and `ADMM` (isls/admm.py:6-106).  torch is used for memory and streams only.

HBM layout: every array is [B, N, ...] row-major (trajectory-major), so one trajectory's horizon is a
contiguous stream (A: N*n*n, K: N*m*n, x: N*n ... elements) that a wavefront slot walks backwards
(Riccati) or forwards (rollout) with one-step-ahead prefetch; shared tables (LTI A/B, via-point Q, box
bounds, rho weights) are passed with zero batch/time strides and stay cache-resident.
"""
import functools
import os

import numpy as np
import torch

from . import _capi as capi

_KERN = None
library = capi.library


def kernels():
    """The process-wide binding of csrc/libisls_hip.so (raises if it has not been built)."""
    global _KERN
    if _KERN is None:
        _KERN = capi.Kernels(library(), prefix="isls_", with_stream=True)
    return _KERN


ALPHAS = 10.0 ** np.linspace(0.0, -5.0, 50)            # line-search grid, isls/isls_base.py:10-11

# who wrote the A, Bm an engine holds (Engine._ab_src, None if nobody it knows of): isls_linearize for the model set now
# (STATIC: a state-independent model's, written once for every trajectory) or a caller (AB setter, get_AB, a shared LTI pair).
# The passes may take the model's structure (isls_gain_args.lin_on / isls_ff_args.lin_on) for the model's own linearisation only
LINEARIZED, STATIC, CALLER = "linearized", "static", "caller"


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


class _Timed:
    def __init__(self, eng, name):
        self.eng, self.name = eng, name

    def __enter__(self):
        ev = self.eng.profile_events
        if ev is not None:
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        ev = self.eng.profile_events
        if ev is not None:
            self.b.record()
            ev.setdefault(self.name, []).append((self.a, self.b))
        return False


class Engine:
    profile_events = None
    use_model_structure = True     # False: the passes keep the dense forms for every model (bench.py's general layout)

    def __init__(self, batch, N, x_dim, u_dim, dtype=torch.float64, device="cuda"):
        if not torch.cuda.is_available():
            raise capi.IslsError("isls.Engine needs a HIP device (torch.cuda.is_available() is False); "
                                 "there is no CPU fallback")
        self.kern = kernels()
        self.B, self.N, self.n, self.m = int(batch), int(N), int(x_dim), int(u_dim)
        # pairs with an instantiation of the row-per-lane kernels run those; any other pair with n <= 16, m <= 8 runs the generic
        # kernels (csrc/generic.hip: array form, no packed records, no time-parallel segments); beyond that the library refuses
        self.fast_dims = capi.dims_supported(self.n, self.m)
        if not self.fast_dims and not capi.dims_generic(self.n, self.m):
            raise capi.IslsError(f"libisls_hip.so has no kernels for x_dim={self.n}, u_dim={self.m}: the generic kernels serve "
                                 f"x_dim <= 16, u_dim <= 8; instantiated fast pairs: {capi.supported_dims()}")
        self.dtype, self.device = dtype, torch.device(device)
        self.sfx = "f64" if dtype == torch.float64 else "f32"
        B, N, n, m = self.B, self.N, self.n, self.m
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=self.device)          # noqa: E731
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=self.device)   # noqa: E731
        # nominal trajectory and its cost
        self.xhat, self.uhat, self.cost = z(B, N, n), z(B, N, m), z(B)
        # linearisation (the A, Bm properties and who wrote them) and cost expansion
        self._A, self._Bm, self._ab_src = z(B, N, n, n), z(B, N, n, m), None
        self.Cxx, self.Cuu, self.c0x, self.c0u = z(B, N, n, n), z(B, N, m, m), z(B, N, n), z(B, N, m)
        self.Cux = None
        self._Cxx_sh = self._Cuu_sh = self._c0_sh = None     # batch-shared Hessian tables (hessians()), made on first use ...
        self._hess_dirty = True                              # ... and written by the next expand()
        # Riccati factors and gains
        self.K, self.Quu, self.fac, self.Qux, self.k = z(B, N, m, n), z(B, N, m, m), z(B, N, m, m), z(B, N, m, n), z(B, N, m)
        # x-step result (line-search winner)
        self.xx, self.xu, self.cost_new = z(B, N, n), z(B, N, m), z(B)
        self.best, self.status = zi(B), zi(B)
        # ADMM state
        self.zx = self.lx = self.zu = self.lu = None
        self.res, self.res_prev = z(B, 2), torch.full((B, 2), 1e6, dtype=dtype, device=self.device)
        self.outer_active = torch.ones(B, dtype=torch.int32, device=self.device)
        self.admm_active = torch.ones(B, dtype=torch.int32, device=self.device)
        self.admm_iters = zi(B)                              # executed ADMM iterations of the current outer iteration
        self.out5 = z(5)
        self.cost_hist, self.hist_len = z(B, 8), zi(B)      # tail of cost_log per trajectory (isls_base.py:85)
        self.alphas = torch.as_tensor(ALPHAS, dtype=dtype, device=self.device)
        # problem description
        self.model = None
        self.model_par = None
        self.model_tab_w = 0                                  # words per step of a user model's table (models.Custom(table=)), 0: none
        self.Qtab = self.ztab = self.seq = self.q_nonzero = None
        self.u_std = 0.0
        self.cost_model, self.cost_par = capi.COST_VIA, None
        self.cost_tab = None                                  # a user cost's per-step table [N, W] / [B, N, W] (set_cost_model)
        self.allow_shared_hessian = True                      # front ends that write Cxx / Cuu themselves switch it off
        self.Qr = self.Rr = self.wq = self.wr = self.Qr_ff = self.Qr_term = None      # ADMM weights: set_weights()
        self._w_invariant, self._w_terminal = True, False
        self.x_lo = self.x_hi = self.u_lo = self.u_hi = None
        self.x_sets = self.u_sets = self.x_work = self.u_work = None
        self.x_col0 = self.u_col0 = 0
        self.relax = 1.0
        self.solve_mode = capi.SOLVE_CHOL
        # buffers made on first use, and the argument blocks cached over the engine's buffers
        self._ffrec = self._seg_bufs = self._advance_args = None
        self._rec_lean = False                               # the last gain pass wrote self._ffrec in the lean layout
        self._rec_shared = False                             # ... as the batch's ONE set of records (the outer driver: records_shared)
        self._outer_args = self._outer_rec = self._outer_seg = self._outer_lin_state = self._outer_log = None
        # per-trajectory regularisation of the gain pass (set_regularization): settings, mu, delta, and the retry loop's scratch
        self.reg = None
        self.reg_mu, self.reg_delta = z(B), torch.ones(B, dtype=dtype, device=self.device)
        self._reg_retry, self._reg_count = zi(B), zi(1)
        self.reg_gain_launches = 0                           # gain launches of the last regularised pass (1 + retries)

    # ---- optional per-kernel-family event timing (bench.py) -------------------------------------------------
    def timed(self, name):
        """Context manager: with `self.profile_events` set to a dict, HIP events are recorded on the launch stream around
        the enclosed launches and collected under `name` (the kernels run on torch's current stream); otherwise a no-op."""
        return _Timed(self, name)

    def family_ms(self):
        """{name: (total ms, launches groups)} of the events recorded since profile_events was set; synchronises."""
        torch.cuda.synchronize()
        return {k: (sum(a.elapsed_time(b) for a, b in v), len(v)) for k, v in (self.profile_events or {}).items()}

    # ---- A, Bm and who wrote them ----------------------------------------------------------------------------
    @property
    def A(self):
        return self._A

    @A.setter
    def A(self, t):
        self._A = t
        self._ab_stale()

    @property
    def Bm(self):
        return self._Bm

    @Bm.setter
    def Bm(self, t):
        self._Bm = t
        self._ab_stale()

    def _ab_stale(self):
        """A, Bm are no linearisation of the model any more (new buffers, a new model; a caller's stay a caller's)"""
        self._ab_src = CALLER if self._ab_src == CALLER else None
        self._outer_args = self._advance_args = None

    def ab_from_caller(self):
        """A, Bm were written by somebody else (AB setter, get_AB callback): the dense records are the only valid form.  Only
        an assignment of A / Bm is seen by the engine: after a write INTO the buffers (`eng.A.copy_(...)`) call this.  A cached
        isls_outer_args block keeps its pointers; run_outer() rewrites its hint fields."""
        self._ab_src = CALLER

    # ---- problem setup ---------------------------------------------------------------------------------
    def _t(self, x):
        if not isinstance(x, torch.Tensor):
            x = np.asarray(x)
            if not x.flags.writeable:                          # broadcast views: torch wants an array it may alias
                x = x.copy()
        return torch.as_tensor(x, dtype=self.dtype, device=self.device).contiguous()

    def set_model(self, model_id, par):
        """Built-in forward model (ISLS_MODEL_*) or a user model (models.Custom.model_id); par is [P] (shared) or [B,P] (per
        trajectory).  A user model with a per-step table of W words: [P + N W] or [B, P + N W], [par | row 0 | ... | row N-1]
        (models.Custom.device_params; include/isls_hip.h) -- model_table is the view of its rows."""
        W = capi.user_model_n_tab(model_id)
        par = self._t(par)
        if W and (par.ndim not in (1, 2) or not 0 <= par.shape[-1] - self.N * W <= capi.USER_MAX_PAR
                  or (par.ndim == 2 and par.shape[0] != self.B)):
            raise ValueError(f"model {model_id} reads a table of {W} words per step: its parameters are [P + {self.N} * {W}] or "
                             f"[{self.B}, P + {self.N} * {W}] (par | rows), got {tuple(par.shape)}")
        self.model, self.model_par, self.model_tab_w = int(model_id), par, W
        if self.model >= capi.MODEL_USER_BASE:                # a user model: its module goes onto the device now, outside any capture
            with torch.cuda.device(self.device):
                capi.user_model_load(self.model, self.dtype)
        self._load_user_cost()
        self._ab_stale()

    @property
    def model_table(self):
        """The rows of a table model inside model_par, as a view [N, W] or [B, N, W] (None: a model without a table): what is
        written INTO it is what the next launch reads -- the argument blocks cached over model_par stay valid."""
        if not self.model_tab_w:
            return None
        P = self.model_par.shape[-1] - self.N * self.model_tab_w
        return self.model_par[..., P:].unflatten(-1, (self.N, self.model_tab_w))

    def update_model_table(self, table):
        """New values for the model's table ([N, W], or [B, N, W] where the engine holds one block per trajectory), copied INTO
        model_par with one copy_: nothing is compiled, allocated on the device or marshalled again.  A linearisation made with the
        old rows is stale afterwards."""
        view = self.model_table
        t = table if isinstance(table, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(table), dtype=self.dtype)
        if view is None or tuple(t.shape) not in (tuple(view.shape), tuple(view.shape[-2:])):
            raise ValueError(f"update_model_table: the table is {None if view is None else tuple(view.shape)}, got {tuple(t.shape)}")
        view.copy_(t)
        if self._ab_src == LINEARIZED:
            self._ab_src = None

    @property
    def user_cost(self):
        """True when the cost is a user cost (costs.Custom): its own expansion (with Cux), per-trajectory Hessians, no model hint"""
        return self.cost_model >= capi.COST_USER_BASE

    def _load_user_cost(self):
        """A user cost with a model to run it with: the module of the pair goes onto the device now, outside any capture."""
        if self.user_cost:
            if not self.fast_dims:
                raise capi.IslsError("a user cost needs one of the (x_dim, u_dim) pairs with the row-per-lane kernels")
            with torch.cuda.device(self.device):
                # with a model: the pair's module (line search, expansion, nominal cost); without one yet: expansion and cost
                capi.user_cost_load(self.cost_model, -1 if self.model is None else self.model, self.dtype)

    def set_regularization(self, reg):
        """A `Regularization` (or None: the plain passes) for the gain passes from now on; mu restarts at mu_init, delta at 1.
        While one is set the engine runs the general layout (_structure_applies), as it does for a user cost."""
        self.reg = reg
        self.reg_mu.fill_(0.0 if reg is None else reg.mu_init)
        self.reg_delta.fill_(1.0)
        self._outer_args = self._advance_args = None

    def set_quadratic_cost(self, zs, Qs, seq, u_std):
        """Via-point quadratic cost (Base.set_quadratic_cost, isls/base.py:81-89); zs [nvia,n] or [B,nvia,n]."""
        self.ztab, self.Qtab = self._t(zs), self._t(Qs)
        seq = np.asarray(seq.cpu() if isinstance(seq, torch.Tensor) else seq).astype(np.int32)
        self.seq = torch.as_tensor(seq, device=self.device)
        qnz = (self.Qtab.reshape(-1, self.Qtab.shape[-3], self.n * self.n) != 0).any(-1).any(0).cpu().numpy()
        self.q_nonzero = torch.as_tensor(qnz[seq].astype(np.int32), device=self.device)
        self.u_std = float(u_std)
        self.cost_model, self.cost_par, self.cost_tab = capi.COST_VIA, None, None
        self._outer_args = None
        self._hess_dirty = True

    def set_cost_model(self, cost_model, par, table=None):
        """Non-quadratic cost of the line search and of the expansion: built in (ISLS_COST_PHUBER: [cu, cx, px, cf, pf]) or a
        user cost (costs.Custom.cost_model; par [P] shared or [B, P] per trajectory; table: the [N, W] or [B, N, W] per-step
        table of a cost registered with one)."""
        par = np.ascontiguousarray(par)
        if int(cost_model) >= capi.COST_USER_BASE:
            W =capi.user_cost_n_tab(cost_model)
            if (table is None) != (W == 0):
                raise ValueError(f"cost {cost_model} " + (f"reads a table of {W} words per step: table=" if W else "has no table"))
            if table is not None:
                table = np.ascontiguousarray(table)
                if table.ndim not in (2, 3) or table.shape[-2:] != (self.N, W) or (table.ndim == 3 and table.shape[0] != self.B):
                    raise ValueError(f"the cost's table: [{self.N}, {W}] or [{self.B}, {self.N}, {W}], got {table.shape}")
        elif table is not None:
            raise ValueError("table: a user cost's (costs.Custom)")
        self.cost_model, self.cost_par = int(cost_model), self._t(par)
        self.cost_tab = None if table is None else self._t(table)
        if self.user_cost:
            if self.Cux is None:
                self.Cux = torch.zeros(self.B, self.N, self.m, self.n, dtype=self.dtype, device=self.device)
            self._load_user_cost()
        # the via-point tables are ignored by this cost model; one all-zero entry keeps every argument block well formed
        self.Qtab, self.ztab = torch.zeros(1, self.n, self.n, dtype=self.dtype, device=self.device), torch.zeros(1, self.n, dtype=self.dtype, device=self.device)
        self.seq = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.q_nonzero = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.u_std = 0.0
        self._outer_args = self._advance_args = None

    def update_cost_table(self, table):
        """New values for the user cost's table, copied INTO the device tensor the engine holds: the argument blocks cached over
        it (and the raw pointer inside them) stay valid; nothing is compiled, allocated on the device or marshalled again."""
        if self.cost_tab is None or tuple(np.shape(table)) != tuple(self.cost_tab.shape):
            raise ValueError(f"update_cost_table: the table is {None if self.cost_tab is None else tuple(self.cost_tab.shape)}, "
                             f"got {tuple(np.shape(table))}")
        self.cost_tab.copy_(torch.as_tensor(np.ascontiguousarray(table), dtype=self.dtype))

    def set_nominal(self, x_nom, u_nom):
        """nominal_values setter (isls/isls_base.py:80-85): stores the nominal and evaluates its cost."""
        self.xhat.copy_(self._t(x_nom).expand(self.B, self.N, self.n))
        self.uhat.copy_(self._t(u_nom).expand(self.B, self.N, self.m))
        self.nominal_rewritten()

    def nominal_rewritten(self):
        """The nominal on the device was rewritten (set_nominal, mpc_step): its cost, a cost log of that one entry, every
        trajectory iterating again with a clean status.  Device work only, nothing is read back."""
        self.evaluate_cost()
        self.cost_hist.zero_()
        self.cost_hist[:, 0] = self.cost                  # cost_log = [initial cost]
        self.hist_len.fill_(1)
        self.outer_active.fill_(1)
        self.status.zero_()

    def mpc_step(self, plant_par=None, u_lo=None, u_hi=None, w=None, noise_std=None, seed=0, step=0, feedback=True,
                 shift_z=True, tab_next=None, x_meas_out=None, u_out=None, x_next_out=None):
        """One control step of a receding-horizon loop on the engine's own buffers (isls_mpc_step_*, csrc/mpc.hpp): the first
        control of every plan through the plant (the model with `plant_par`; None: the model's own), then xhat, uhat, K (feedback
        only: else the plan is re-rolled open loop and K stays), zx, zu (shift_z) and the user cost's table move up by one step and the plan
        is rolled out again from the measured state; then nominal_rewritten().  Everything is written INTO the tensors the engine
        holds -- the contract of update_cost_table: cached argument blocks stay valid -- and nothing is read back.  A
        linearisation along the old nominal is stale afterwards; a state-independent model keeps its one linearisation."""
        if self.model is None:
            raise capi.IslsError("Engine.mpc_step needs a device model (set_model)")
        self.kern.mpc_step(self.model, self.model_par, self.xhat, self.uhat, K=self.K if feedback else None,
                           zx=self.zx if shift_z else None, zu=self.zu if shift_z else None,
                           plant_par=plant_par, tab=self.cost_tab, tab_next=tab_next, u_lo=u_lo, u_hi=u_hi, w=w,
                           noise_std=noise_std, seed=seed, step=step, x_meas_out=x_meas_out, u_out=u_out, x_next_out=x_next_out,
                           stream=_stream_ptr())
        if self._ab_src == LINEARIZED:                         # A, Bm belong to the nominal that has just left
            self._ab_src = None
        self.nominal_rewritten()

    def sample_round(self, sigma, costs, u_lo=None, u_hi=None, temperature=1.0, seed=0, active=None, K=None, **stats):
        """One sampling round about the nominal on the engine's own buffers (isls_sample_nominal_*, csrc/sampling.hpp): costs
        [B, S] of S open-loop rollouts with controls drawn about uhat (sigma [m] or [B, m], clipped to u_lo / u_hi), then xhat,
        uhat <- their path-integral mean, or the best sample where that mean does not beat it.  Written INTO the tensors the engine
        holds, nothing is read back; `stats`: cost_before, cost_after, cost_best, ess, took_best [B] (or columns of [B, rounds]).
        The caller ends a series of rounds with nominal_rewritten().  K [N, m, n] or [B, N, m, n] (a device tensor of the engine's
        dtype): the round in closed loop about these gains (isls_sample_nominal_fb_*), controls uhat_t + K_t (x_t - xhat_t) + noise."""
        if self.model is None:
            raise capi.IslsError("Engine.sample_round needs a device model (set_model)")
        fn = self.kern.sample_nominal if K is None else functools.partial(self.kern.sample_nominal_fb, K=K)
        fn(self.model, self.model_par, self.xhat, self.uhat, self.Qtab, self.ztab, self.seq, self.u_std, sigma,
           costs, cost_model=self.cost_model, cost_par=self.cost_par, cost_tab=self.cost_tab, u_lo=u_lo,
           u_hi=u_hi, temperature=temperature, seed=seed, active=active, stream=_stream_ptr(), **stats)
        if self._ab_src == LINEARIZED:                         # A, Bm belong to the nominal that has just left
            self._ab_src = None

    def set_weights(self, Qr, Rr):
        """ADMM weights Qr [n,n] / [1|N,n,n] / [B,N,n,n], Rr likewise (or None) and what the passes take from them: the line
        search's AL weights wq, wr, the terminal-block form (Qr_ff, Qr_term) and whether they are the same at every step."""
        self.Qr, self.Rr = Qr, Rr
        # (dx*dx)@Qr precedence (isls/isls.py:473,476): the AL weights are the row sums
        self.wq = None if Qr is None else Qr.sum(-1).contiguous()
        self.wr = None if Rr is None else Rr.sum(-1).contiguous()
        # a state weight that is the same at every step but the LAST (a terminal constraint: the arm notebook's bound on the
        # final end-effector position) reaches the record feed-forward passes as one block plus the terminal block
        # (isls_ff_args.Qr_term): they then run the one-hand-off kernel instead of loading a weight row per step
        self.Qr_ff = self.Qr_term = None
        if Qr is not None and Qr.ndim == 3 and Qr.shape[0] == self.N and self.N > 2 and bool((Qr[:-1] == Qr[:1]).all()):
            self.Qr_ff, self.Qr_term = Qr[:1].contiguous(), Qr[-1].contiguous()
        q_fixed, r_fixed = (W is None or W.ndim < 3 or W.shape[-3] == 1 for W in (Qr, Rr))   # the same at every step
        self._w_invariant = q_fixed and r_fixed                     # as they are (the column passes hand them over so)
        self._w_terminal = self.Qr_term is not None and r_fixed     # in the terminal-block form
        self._outer_args = None
        self._hess_dirty = True

    def set_admm(self, rho_x=None, rho_u=None, x_box=None, u_box=None, relax=1.0, x_sets=None, u_sets=None):
        """ADMM weights (Base.compute_Rr_Qr, isls/base.py:55-79, dp=True form) and the constraint sets: boxes
        (lo, hi) or `isls.projections.ConvexSets` (project_set_convex over the time steps, on the device)."""
        B, N, n, m = self.B, self.N, self.n, self.m
        z = lambda *s: torch.zeros(*s, dtype=self.dtype, device=self.device)      # noqa: E731

        def weights(rho, d):
            if rho is None:
                return None
            if isinstance(rho, (int, float)):
                return (float(rho) * torch.eye(d, dtype=self.dtype, device=self.device)).reshape(1, d, d)
            r = self._t(rho)
            if r.ndim == 2:
                return r.reshape(1, d, d)
            if r.ndim == 3 and bool((r == r[:1]).all()):
                # given per step but the same at every step (compute_Rr_Qr's tiling of a matrix, isls/base.py:55-79): kept as
                # one time-invariant block -- the kernels then hold the rows in registers instead of loading them per step,
                # and the feed-forward pass takes its one-hand-off form
                return r[:1].contiguous()
            return r                                   # [N,d,d] or [B,N,d,d]

        has_x, has_u = x_box is not None or x_sets is not None, u_box is not None or u_sets is not None
        Qr = weights(rho_x, n) if has_x else None
        Rr = weights(rho_u, m) if has_u else None
        if has_x and Qr is None:
            raise ValueError("project_x needs rho_x")
        if has_u and Rr is None:
            raise ValueError("project_u needs rho_u")
        self.set_weights(Qr, Rr)

        def bounds(box, d):
            if box is None:
                return None, None
            lo, hi = box
            lo = self._t(lo) if not isinstance(lo, (int, float)) else torch.full((1, d), float(lo), dtype=self.dtype, device=self.device)
            hi = self._t(hi) if not isinstance(hi, (int, float)) else torch.full((1, d), float(hi), dtype=self.dtype, device=self.device)
            if lo.ndim == 1 and lo.numel() == N * d:      # flat [N*d] vectors as the reference's callbacks see them
                lo, hi = lo.reshape(N, d), hi.reshape(N, d)
            return lo, hi

        self.x_lo, self.x_hi = bounds(x_box, n)
        self.u_lo, self.u_hi = bounds(u_box, m)
        self.zx, self.lx = (z(B, N, n), z(B, N, n)) if has_x else (None, None)
        self.zu, self.lu = (z(B, N, m), z(B, N, m)) if has_u else (None, None)
        self.relax = float(relax)

        def device_sets(cs, d):
            """ConvexSets -> (isls_project_args descriptor, first column, scratch) with the operands on the device."""
            if cs is None:
                return None, 0, None
            if cs.dim != d:
                raise ValueError(f"constraint set is defined on rows of dimension {cs.dim}, expected {d}")
            work = z(B, N, d)
            wrap = lambda a: (torch.as_tensor(a, device=self.device) if a.dtype.kind in "iu" else self._t(a))   # noqa: E731
            desc = capi.Kernels.project_args_chain(work, work, cs.stages(), wrap=wrap)
            return desc, cs.cols[0], work

        self.x_sets, self.x_col0, self.x_work = device_sets(x_sets, n)
        self.u_sets, self.u_col0, self.u_work = device_sets(u_sets, m)
        if x_sets is not None:
            self.x_lo = self.x_hi = None
        if u_sets is not None:
            self.u_lo = self.u_hi = None

    def advance_sets(self, k=1, x=True, u=True):
        """Move the window of the per-row tables of the constraint sets (ConvexSets with par_rows / b_rows) k rows on: the
        sets follow a plan that moves through time.  A host-side update of the pointers in the isls_project_args descriptors
        the engine holds -- the argument blocks of build_outer keep the descriptors' addresses and the library reads them at
        each call, so they stay valid.  No kernel, no copy, no synchronisation.  x / u: which block's sets move."""
        for desc, on in ((self.x_sets, x), (self.u_sets, u)):
            if on and desc is not None and capi.Kernels.project_args_per_row(desc):
                capi.Kernels.project_args_set_row0(desc, desc._row0 + int(k))

    # ---- single kernels -----------------------------------------------------------------------------------
    def evaluate_cost(self, out=None):
        """cost of the nominal into `out` (default: self.cost); also refreshes c0x, c0u about it"""
        if self.user_cost:
            self.kern.user_cost_expand(self._expand_block(False, None, cost=self.cost if out is None else out), None, self.sfx,
                                       stream=_stream_ptr())
            return
        self.kern.expand_quadratic(self.Qtab, self.ztab, self.seq, self.u_std, self.c0x, self.c0u,
                                   xhat=self.xhat, uhat=self.uhat, cost=self.cost if out is None else out, cost_model=self.cost_model,
                                   cost_par=self.cost_par, q_nonzero=self.q_nonzero, stream=_stream_ptr())

    def linearize(self):
        # a state-independent model (double integrator, dense LTI) has ONE linearisation: it is written for every trajectory,
        # active or not, and advance() then leaves A, Bm alone for as long as they stay the model's
        static = self.model in (capi.MODEL_DI, capi.MODEL_LTI)
        self.kern.linearize(self.model, self.model_par, self.xhat, self.uhat, self.A, self.Bm,
                            active=None if static else self.outer_active, stream=_stream_ptr())
        self._ab_src = STATIC if static else LINEARIZED

    def _structure_applies(self):
        """What every model-structured pass needs of the engine: the row-per-lane kernels for these dimensions, the forms not
        switched off (use_model_structure), a model whose structure the passes know, and ADMM weights that are the same at
        every step (Qr: or all but the last, which the passes take as the terminal block Qr_term)."""
        # (a user cost has a full stage Hessian, Cux included, which the structured passes do not take: refused, not guessed)
        return (self.fast_dims and self.use_model_structure and self.model in (capi.MODEL_DI, capi.MODEL_ARM3R, capi.MODEL_CAR)
                and (self._w_invariant or self._w_terminal) and not self.user_cost and self.reg is None)

    def _structure_expected(self):
        """Will the passes of this engine get the model hint, as far as can be told before A, B are linearised: the structured
        forms apply and no A, B were handed in by a caller."""
        return self._structure_applies() and self._ab_src != CALLER

    def ff_lin(self, rec, seg=None, weights_as_is=False):
        """(model id, parameters) for isls_gain_args.lin_on / isls_ff_args.lin_on, or None.  The hint makes the gain pass write
        the LEAN records and the feed-forward passes read them, so it is given only when every pass on these records can take
        the structured form: the structured forms apply (_structure_applies; `weights_as_is`: the passes take Qr as it is,
        the same at every step), the packed records are in use, A and Bm are what isls_linearize wrote for the model set now,
        and the passes run sequentially (`seg`: the time-parallel form builds its operators from the dense records)."""
        ok = (rec is not None and seg is None and self.model_par is not None and self._ab_src in (LINEARIZED, STATIC)
              and self._structure_applies() and (self._w_invariant or not weights_as_is))
        return (self.model, self.model_par) if ok else None

    def _shared_hessian(self):
        """True when the cost Hessians are the same arrays for every trajectory of the batch: via-point cost with a batch-
        shared Q table and batch-shared ADMM weights (Cxx_t = 2 Q_seq[t] + 2 Qr_t does not depend on the nominal).  They
        are then written once as [N,n,n] / [N,m,m] and handed to the gain pass with a zero batch stride (SURVEY 8(d):
        "drop the Cxx,Cuu terms when they are shared tables"), instead of B identical copies."""
        return (self.allow_shared_hessian and self.B > 1 and self.cost_model == capi.COST_VIA
                and self.Qtab is not None and self.Qtab.ndim == 3
                and (self.Qr is None or self.Qr.ndim <= 3) and (self.Rr is None or self.Rr.ndim <= 3))

    def hessians(self):
        """(Cxx, Cuu) operands of the gain pass: the batch-shared [1,N,.,.] pair when the cost allows it (expand() then
        writes that form), else the per-trajectory arrays."""
        if not self._shared_hessian():
            return self.Cxx, self.Cuu
        if self._Cxx_sh is None:
            z = lambda *sh: torch.zeros(*sh, dtype=self.dtype, device=self.device)   # noqa: E731
            self._Cxx_sh, self._Cuu_sh = z(1, self.N, self.n, self.n), z(1, self.N, self.m, self.m)
            self._c0_sh = (z(1, self.N, self.n), z(1, self.N, self.m))
        return self._Cxx_sh, self._Cuu_sh

    def _expand_block(self, with_hessian, active, cost=None):
        return capi.Kernels.expand_args(self.Qtab, self.ztab, self.seq, self.u_std, self.c0x, self.c0u, xhat=self.xhat, uhat=self.uhat,
                                        Cxx=self.Cxx if with_hessian else None, Cuu=self.Cuu if with_hessian else None,
                                        Qr=self.Qr, Rr=self.Rr, cost=cost, active=active, cost_model=self.cost_model,
                                        cost_par=self.cost_par, q_nonzero=self.q_nonzero, cost_tab=self.cost_tab)

    def expand(self, with_hessian=True):
        if self.user_cost:                                     # user_expand_kernel: gradient and full Hessian, Cux included
            if self.Cux is None or self.Cux.shape != (self.B, self.N, self.m, self.n):
                self.Cux = torch.zeros(self.B, self.N, self.m, self.n, dtype=self.dtype, device=self.device)
                self._outer_args = None
            self.kern.user_cost_expand(self._expand_block(with_hessian, self.outer_active), self.Cux if with_hessian else None,
                                       self.sfx, stream=_stream_ptr())
            return
        shared = with_hessian and self._shared_hessian()
        self.kern.expand_quadratic(self.Qtab, self.ztab, self.seq, self.u_std, self.c0x, self.c0u,
                                   xhat=self.xhat, uhat=self.uhat,
                                   Cxx=self.Cxx if with_hessian and not shared else None,
                                   Cuu=self.Cuu if with_hessian and not shared else None,
                                   Qr=self.Qr, Rr=self.Rr, active=self.outer_active, cost_model=self.cost_model,
                                   cost_par=self.cost_par, q_nonzero=self.q_nonzero, stream=_stream_ptr())
        if shared and self._hess_dirty:                        # constants of the problem: written once per cost / weights
            Cxx, Cuu = self.hessians()
            self._hess_dirty = False
            self.kern.expand_quadratic(self.Qtab, self.ztab[:1] if self.ztab.ndim == 3 else self.ztab, self.seq, self.u_std,
                                       *self._c0_sh, Cxx=Cxx, Cuu=Cuu, Qr=self.Qr, Rr=self.Rr, stream=_stream_ptr())

    def ff_record(self):
        """Packed step records [A + B K | B | K | fac] the gain pass writes for the feed-forward passes (isls_gain_args.rec /
        isls_ff_args.rec), or None for the generic kernels, which have none.  Only the drivers that run the gain pass
        themselves right before the feed-forward passes use it: the records are stale once K / fac are replaced."""
        if not self.fast_dims:
            return None
        if self._ffrec is None:
            self._ffrec = torch.zeros(capi.ff_record_elems(self.B, self.N, self.n, self.m), dtype=self.dtype, device=self.device)
        return self._ffrec

    # ---- argument blocks of the passes, for the single launches below and for build_outer -------------------------
    def _gain_block(self, active, rec, lin):
        # with the records, nothing after this pass reads Quu / fac / Qux: the gain pass then skips those stores
        full = rec is None
        return capi.Kernels.gain_args(self.A, self.Bm, *self.hessians(), self.K, self.Quu if full else None,
                                      self.fac if full else None, self.Qux if full else None, Cux=self.Cux,
                                      solve_mode=self.solve_mode, status=self.status, active=active, rec=rec, lin=lin)

    def _ff_block(self, active, rec, seg, lin):
        # on the packed records the weights take the terminal-block form where it applies
        Qr, Qr_term = (self.Qr_ff, self.Qr_term) if rec is not None and self._w_terminal else (self.Qr, None)
        return capi.Kernels.ff_args(self.A, self.Bm, self.c0x, self.c0u, self.K, self.Quu, self.fac, self.Qux, self.k,
                                    Qr=Qr, Qr_term=Qr_term, Rr=self.Rr, xhat=self.xhat, uhat=self.uhat, zx=self.zx, lx=self.lx,
                                    zu=self.zu, lu=self.lu, solve_mode=self.solve_mode, active=active, seg=seg, rec=rec, lin=lin)

    def _rollout_block(self, L, active, flags=0, cost_all=None):
        return capi.Kernels.rollout_args(self.model, self.model_par, self.K, self.k, self.xhat, self.uhat, self.alphas[:L],
                                         self.Qtab, self.ztab, self.seq, self.u_std, self.xx, self.xu, best=self.best,
                                         cost_new=self.cost_new, cost_all=cost_all, wq=self.wq, wr=self.wr, zx=self.zx,
                                         lx=self.lx, zu=self.zu, lu=self.lu, cost_cur=self.cost, flags=flags,
                                         status=self.status, active=active, q_nonzero=self.q_nonzero,
                                         cost_model=self.cost_model, cost_par=self.cost_par, cost_tab=self.cost_tab)

    def _admm_block(self, tol_abs, tol_rel, active):
        return capi.Kernels.admm_args(self.xx, self.xu, self.res, zx=self.zx, lx=self.lx, zu=self.zu, lu=self.lu,
                                      x_lo=self.x_lo, x_hi=self.x_hi, u_lo=self.u_lo, u_hi=self.u_hi, relax=self.relax,
                                      tol_abs=tol_abs, tol_rel=tol_rel, res_prev=self.res_prev, active=active,
                                      iters=self.admm_iters, x_sets=self.x_sets, x_col0=self.x_col0, x_work=self.x_work,
                                      u_sets=self.u_sets, u_col0=self.u_col0, u_work=self.u_work)

    def gain(self, active=None, rec=None, seg=None, weights_as_is=False):
        """Gain pass; with `rec` the caller promises to run its feed-forward passes on the records, and Quu / fac / Qux
        (which only those passes would read) are not written.  `seg`: the segment plan those passes will use (ff_lin);
        `weights_as_is`: the caller's passes take Qr, Rr as they are, not in the terminal-block form."""
        lin = self.ff_lin(rec, seg, weights_as_is)
        self._rec_lean, self._rec_shared = lin is not None, False      # the single launch writes a record per trajectory
        if self.reg is not None:
            self._gain_regularised(active, rec)
            return
        self.kern._call("riccati_gain", self.sfx, self._gain_block(active, rec, lin), _stream_ptr())

    def _gain_regularised(self, active, rec, ff=None):
        """The gain pass on Cuu + mu I with the retry loop: pass, schedule (mu rises where Quu was not positive definite, the bit is
        cleared), read the one counter, launch again while it is non-zero.  Every launch takes the caller's mask, so the records
        and K of every active trajectory end as one pass given the final mu would leave them (a trajectory that never failed
        recomputes with its mu unchanged).  A trajectory at the end of the ladder keeps ISLS_ST_NOT_PD and gets ISLS_ST_REG_MAX."""
        r = self.reg
        g = self._gain_block(active, rec, None)
        self.reg_gain_launches = 0
        while True:
            self.kern.riccati_gain_reg(g, ff, self.reg_mu, r.on_x, self.sfx, stream=_stream_ptr())
            self.reg_gain_launches += 1
            self._reg_count.zero_()
            self.kern.reg_update(capi.REG_AFTER_GAIN, self.status, self.reg_mu, self.reg_delta, r.factor, r.mu_min, r.mu_max,
                                 active=active, retry=self._reg_retry, count=self._reg_count, stream=_stream_ptr())
            if int(self._reg_count.item()) == 0:
                return

    def backward_pass_regularised(self, active=None):
        """K and k of one regularised backward sweep, as iterate_once_dp needs them.  On the pairs whose gain pass carries the
        first feed-forward pass (row-per-lane kernels, n n + n (n + m) <= 100) and with ADMM weights that are the same at every
        step, both come from the one launch on the packed records (a retry repeats both); otherwise the gain pass on the arrays
        and the feed-forward pass behind it."""
        rec = self.ff_record()
        fused = (rec is not None and self.n * self.n + self.n * (self.n + self.m) <= 100 and self._w_invariant)
        if not fused:
            self.gain(active=active)
            self.feedforward(active=active)
            return
        self._rec_lean = self._rec_shared = False
        self._gain_regularised(active, rec, self._ff_block(active, rec, None, None))

    def reg_after_line_search(self, active=None):
        """The schedule behind a line search with the acceptance test: mu rises where it was rejected, falls where it was accepted."""
        r = self.reg
        self.kern.reg_update(capi.REG_AFTER_LS, self.status, self.reg_mu, self.reg_delta, r.factor, r.mu_min, r.mu_max,
                             active=active, stream=_stream_ptr())

    def rec_lin(self, rec, seg=None):
        """The hint for a feed-forward pass on `rec` as the last gain pass left it: lean records need the structured form (and
        raise when it does not apply any more), dense ones the dense form."""
        if rec is not None and self._rec_shared:
            raise capi.IslsError("the outer driver left one set of records for the whole batch (records_shared), which a feed-forward "
                                 "pass of its own cannot read: run the gain pass again")
        if rec is None or not self._rec_lean:
            return None
        lin = self.ff_lin(rec, seg)
        if lin is None:
            raise capi.IslsError("the gain pass wrote the records in the model-structured layout, which this feed-forward pass cannot "
                                 "read (weights, segments or A, B changed since): run the gain pass again")
        return lin

    @property
    def records_shared(self):
        """True when the last gain pass on ff_record() was the outer driver's and it kept ONE set of records for the whole batch:
        the argument block declared the same A, B, Cxx, Cuu (Cux) for every trajectory -- the double integrator's structured form
        with one parameter row, batch-shared Hessian tables, the sequential recursion (csrc/capi.hip decides from the same
        fields).  Only the driver's own passes read that layout."""
        return self._rec_shared

    def _outer_shares_records(self):
        a = self._outer_args
        g, f = a.gain, a.ff
        return bool(a.J > 0 and not a.skip_gain and self.fast_dims and self._outer_rec is not None and self._outer_seg is None
                    and g.lin_on and g.lin_model == capi.MODEL_DI and g.lin_par and g.lin_par_sb == 0
                    and g.Cxx.sb == 0 and g.Cuu.sb == 0 and (not g.Cux.p or g.Cux.sb == 0)
                    and f.lin_on and f.lin_par_sb == 0)

    def feedforward(self, active=None, seg=None, rec=None):
        self.kern._call("riccati_ff", self.sfx, self._ff_block(active, rec, seg, self.rec_lin(rec, seg)), _stream_ptr())

    def rollout(self, L, flags=0, cost_all=None, active=None):
        self.kern._call("rollout_ls", self.sfx, self._rollout_block(L, active, flags, cost_all), _stream_ptr())

    def admm_update(self, tol_abs, tol_rel, active=None):
        self.kern._call("admm_update", self.sfx, self._admm_block(tol_abs, tol_rel, active), _stream_ptr())

    # ---- time-parallel feed-forward pass (isls_ffseg): operators from the gain pass, reused by J ADMM iterations
    def ff_seg(self, nseg_requested=None, ncol=1, weights_as_is=False):
        """Segment descriptor over engine-owned buffers, or None for the sequential recursion.  `ncol`: columns per trajectory
        the passes solve (ColumnSolver); `weights_as_is`: the passes take Qr, Rr as they are (ff_lin)."""
        if not self.fast_dims:
            return None                                        # the generic kernels recurse sequentially
        if nseg_requested is None:
            # measured on MI355X: from ~2k trajectories on the pass is bound by HBM throughput whatever its
            # shape (82-87 us for 1, 2 or 3 segments at B=4096; 45 / 36+29 / 39+26 us pass+prepare at B=2048), so the
            # sequential recursion wins: no operators to prepare per gain pass, no stitch launch per ADMM iteration.
            # Smaller batches are bound by the N dependent steps and keep the time-parallel form (B=512: 42 us sequential,
            # 30 us in four segments).  Where the model-structured passes apply (ff_lin) they exist for the sequential
            # recursion only and carry the cheaper gain pass with them: outer iteration at n=6, m=3 (tools/kbench.py, one box)
            # B=256: 504 us segmented / 511 us structured, 512: 517 / 510, 1024: 553 / 535, 1536: 608 / 559 -- sequential from 512.
            # The C columns of B problems stream like a batch of C B trajectories: at 4 x 1024 arm columns the structured
            # sequential pass takes 83 us, the dense one in four segments 107 us.
            seq_from = 512 if self._structure_expected() else 2048
            seq = self.B >= seq_from or (ncol * self.B >= 2048 and self.ff_lin(self.ff_record(), None, weights_as_is) is not None)
            nseg_requested = int(os.environ.get("ISLS_FF_NSEG", "1" if seq else "4"))
        nseg, seg_len = self.kern.ff_segments(self.N, nseg_requested)
        if nseg < 2:
            return None
        if self._seg_bufs is None or self._seg_bufs[1].shape[1] != nseg:
            z = lambda *shape: torch.zeros(*shape, dtype=self.dtype, device=self.device)
            self._seg_bufs = (z(self.B, self.N, self.m, self.n), z(self.B, nseg, self.n, self.n), z(self.B, nseg, self.n))
        return capi.Kernels.ff_seg(*self._seg_bufs, seg_len)

    def feedforward_prepare(self, seg, active=None, rec=None):
        self.kern.riccati_ff_prepare(self.A, self.Bm, self.K, self.Quu, self.fac, self.Qux, seg,
                                     solve_mode=self.solve_mode, active=active, rec=rec, stream=_stream_ptr())

    # ---- one outer iteration, enqueued by the C driver in one call --------------------------------------------
    def build_outer(self, L, J, tol_abs=0.0, tol_rel=0.0, log=None, ff_nseg=None, begin_done=False):
        """Marshal the argument block of isls_ilqr_admm_outer once; it stays valid while buffers are not re-allocated.
        begin_done: the caller ends every outer iteration with `advance()`, which also makes the ADMM restart of the next one."""
        rec = self.ff_record()
        if self.reg is not None and rec is None:
            raise capi.IslsError("a regularisation needs the row-per-lane kernels in the outer driver (the generic (x_dim, u_dim) pairs "
                                 "have no packed records): use solve / iterate_once_dp")
        # regularised: the gain pass runs ahead of the driver with its retry loop (run_outer), the driver skips its own and reads the
        # records sequentially (the segment operators would have to be prepared behind that pass)
        if self.reg is not None and begin_done:
            raise capi.IslsError("a regularisation and begin_done: the ADMM restart must follow the regularised gain pass, which may "
                                 "stop trajectories (build_outer(begin_done=False))")
        seg = None if self.reg is not None else self.ff_seg(ff_nseg)
        lin = self.ff_lin(rec, seg)
        act = self.admm_active
        self._outer_args = capi.OuterArgs(gain=self._gain_block(act, rec, lin), ff=self._ff_block(act, rec, seg, lin),
                                          ro=self._rollout_block(L, act), admm=self._admm_block(tol_abs, tol_rel, act),
                                          J=int(J), skip_gain=int(self.reg is not None), begin_done=int(bool(begin_done)), log=capi._ptr(log),
                                          outer_active=capi._ptr(self.outer_active))
        self._outer_rec, self._outer_seg, self._outer_log = rec, seg, log
        self._outer_lin_state = (self._ab_src, self.use_model_structure)
        self._advance_args = None
        return self._outer_args

    def run_outer(self):
        """gain -> J x [ff -> rollout/line-search -> ADMM update] on the current stream (no host sync)."""
        if self._outer_args is None:
            raise capi.IslsError("no isls_outer_args block for the engine's buffers as they are now: call build_outer()")
        state = (self._ab_src, self.use_model_structure)
        if state != self._outer_lin_state:                     # A, Bm changed hands since the block was marshalled / last run
            lin = self.ff_lin(self._outer_rec, self._outer_seg)
            for a in (self._outer_args.gain, self._outer_args.ff):
                capi.Kernels._set_lin(a, lin, self.B, self.dtype)
            self._outer_lin_state = state
        if self.reg is not None:
            # the regularised gain pass, with retries, on the driver's records and the mask the driver's passes will use (its start
            # sets admm_active <- outer_active); a trajectory at the end of the ladder stops here, the others go on
            self._rec_lean = self._rec_shared = False
            self._gain_regularised(self.outer_active, self._outer_rec)
            self.outer_active.mul_(((self.status & capi.ST_NOT_PD) == 0).to(torch.int32))
            self.kern._call("ilqr_admm_outer", self.sfx, self._outer_args, _stream_ptr())
            return
        if self._outer_rec is not None:                        # the driver's gain pass leaves the records in this layout
            self._rec_lean = bool(self._outer_args.gain.lin_on)
            self._rec_shared = self._outer_shares_records()
        self.kern._call("ilqr_admm_outer", self.sfx, self._outer_args, _stream_ptr())

    def accept_x_step(self, tol_cost=-1.0, tol_osc=-1.0):
        """nominal_values <- last x-step of the ADMM (isls/isls.py:488), cost_log tail and the outer stop
        rules (isls/isls.py:493-499) for the trajectories still iterating; all on the device."""
        self.kern.accept_step(self.xx, self.xu, self.cost_new, self.xhat, self.uhat, self.cost,
                              cost_hist=self.cost_hist, hist_len=self.hist_len, tol_cost=tol_cost, tol_osc=tol_osc,
                              outer_active=self.outer_active, stream=_stream_ptr())

    def begin_outer(self):
        """The ADMM restart at the start of an outer iteration (isls/isls.py:414-415,482; admm.py:25-26) for a driver built with
        begin_done=True: made once before the first iteration (set-up path, torch ops); `advance()` makes the later ones."""
        act = self.outer_active.to(torch.bool)
        self.admm_active.copy_(self.outer_active)
        self.admm_iters.masked_fill_(act, 0)
        for lam in (self.lx, self.lu):
            if lam is not None:
                lam.masked_fill_(act.view(-1, 1, 1), 0.0)
        self.res_prev.masked_fill_(act.view(-1, 1), 1e6)

    def advance(self, tol_cost=-1.0, tol_osc=-1.0, linearize=True):
        """End of an outer iteration and start of the next in one launch (isls_outer_advance_*): accept_x_step(), the ADMM
        restart (admm_active, lambda, residual history), then linearize() and expand() about the new nominal for the
        trajectories still iterating.  Pair it with build_outer(..., begin_done=True).  `linearize=False` leaves A, B alone (a
        shared LTI pair).  The cost Hessians must be the batch-shared tables (written once by expand())."""
        K = capi.Kernels
        if linearize and self.use_model_structure and self._ab_src == STATIC:
            linearize = False                                  # the model's one linearisation is in place: nothing to rewrite
        key = (float(tol_cost), float(tol_osc), bool(linearize))
        if self._advance_args is None or self._advance_args[0] != key:
            if not self.user_cost:
                if not self._shared_hessian():
                    raise capi.IslsError("Engine.advance() serves the batch-shared cost Hessians; use accept_x_step / linearize / expand")
                if self._hess_dirty:
                    self.expand()                              # writes the shared Hessian tables once
            acc = K.accept_args(self.xx, self.xu, self.cost_new, self.xhat, self.uhat, self.cost, cost_hist=self.cost_hist,
                                hist_len=self.hist_len, tol_cost=tol_cost, tol_osc=tol_osc, outer_active=self.outer_active)
            lin = K.linearize_args(self.model, self.model_par, self.xhat, self.uhat, self.A, self.Bm) if linearize else None
            # a built-in cost's expansion (gradients: the Hessians are the shared tables) is fused into the launch; a user cost's
            # follows it on the same stream for the trajectories still iterating (outer_active after the stop rules), about the
            # nominal just written
            exp, after = (None, self._expand_block(True, self.outer_active)) if self.user_cost else (self._expand_block(False, None), None)
            self._advance_args = (key, K.advance_args(acc, lin, exp, admm_active=self.admm_active, iters=self.admm_iters,
                                                      lx=self.lx, lu=self.lu, res_prev=self.res_prev), after)
        self.kern.outer_advance(self._advance_args[1], self.sfx, stream=_stream_ptr())
        if self._advance_args[2] is not None:
            self.kern.user_cost_expand(self._advance_args[2], self.Cux, self.sfx, stream=_stream_ptr())
        if linearize and self._ab_src != STATIC:
            self._ab_src = LINEARIZED                          # the launch linearised the trajectories still iterating

    def reduce(self, table=None, rank=0):
        """[sum cost, max prim, max dual, #active, #failed] of the local shard, left on the device: in `out5`, or straight
        in row `rank` of the all-reduce's [W,5] `table` (its other rows zeroed) -- one launch either way."""
        if table is not None:
            self.kern.reduce_convergence_table(self.cost, self.res, self.outer_active, self.status, table, rank,
                                               stream=_stream_ptr())
            return table
        self.kern.reduce_convergence(self.cost, self.res, self.outer_active, self.status, self.out5, stream=_stream_ptr())
        return self.out5
