"""The backward passes at every slot-packing edge and frozen-lane pattern: riccati_gain_kernel (plain, with the first feed-forward
pass inside, regularised, model-structured), riccati_ff_kernel, riccati_ffrec_kernel, riccati_ffrec2_kernel, the time-parallel
form and columns_rollout_rows_kernel, under masks that switch off slot 0 of a wavefront (the shadowed slot is then not slot 0),
leave whole wavefronts empty between live ones, leave only the last slot alive, or leave one trajectory in the tail wavefront --
for all eight (n, m) pairs of csrc/families.def (T = 64 // (n + m) trajectories per wavefront) and (5, 2) on the generic kernels.

Reference: the C oracle's gain pass followed by its sequential feed-forward pass on the dense arrays (tests/reg_reference.py for
the regularised pass), in the precision of the launch.  Active trajectories compare per trajectory (helpers.compare_batched) at
1e-10 in fp64 and 1e-4 in fp32; inactive ones must keep a random pre-fill bit for bit; every output lies between 64 guard words
on either side; the record and operator buffers start as NaN.

Every trajectory and every step has its own A, B, Hessians (M M' + I, with a Cux block), gradients and ADMM state, so that an
operand taken from a neighbour shows at the tolerance.  The random parts of A and B carry the factor AB_SCALE = 1.0 of
tests/test_regularization_gpu.py's recipe: on these inputs the fp32 oracle stays within a tenth of the fp32 tolerance of the fp64
oracle for every (pair, N, mask) (asserted in every fp32 test on the test's own inputs; worst margin measured 5.3e-6, at (2, 1),
N = 2, against the 1e-5 allowed), so the 1e-4 bound measures the kernel and not the problem."""
import numpy as np
import pytest

from helpers import compare_batched
from isls import _capi as capi
from reg_reference import ST_NOT_PD, materialise

pytestmark = pytest.mark.gpu

PAIRS = [(6, 3), (2, 1), (4, 2), (9, 3), (3, 1), (6, 2), (2, 2), (3, 3)]      # csrc/families.def
FUSED = [(6, 3), (2, 1), (4, 2), (3, 1), (6, 2), (2, 2), (3, 3)]              # pairs whose gain pass takes the first feed-forward pass inside
DI = [(2, 1), (4, 2), (6, 3)]                                                 # double integrators (model hint)
NS = (2, 7, 8)                     # one recursion step; an odd and an even number of steps (loops in pairs with a peeled step)
DTYPES = [("f64", 1e-10), ("f32", 1e-4)]
MODES = [capi.SOLVE_CHOL, capi.SOLVE_INV]
GUARD, SENTINEL = 64, -777
AB_SCALE = 1.0                     # factor on the random parts of A, B (see the module's head)
WORST = {}                         # (form, dtype) -> worst per-trajectory error of the session (printed by every test)
MARGIN = {}                        # (n, m, N) -> fp32 oracle against fp64 oracle


def tpw(n, m):
    return 64 // (n + m) if (n, m) in PAIRS else 1


def plan_mask(plan, T):
    """The mask plans, as functions of the trajectories per wavefront."""
    if plan == 1:                                              # the tail wavefront holds one trajectory
        return np.ones(T + 1, dtype=np.int32)
    if plan == 2:                                              # slot 0 of both full wavefronts off; the tail wavefront empty
        act = np.ones(2 * T + 1, dtype=np.int32)
        act[::T] = 0
        return act
    if plan == 3:                                              # only the last slot | nothing | slot 0 and every second slot off
        act = np.zeros(3 * T, dtype=np.int32)
        act[T - 1] = 1
        act[2 * T + 1::2] = 1
        return act
    if plan == 4:                                              # one wavefront, not full, only its last trajectory
        act = np.zeros(T - 1, dtype=np.int32)
        act[-1] = 1
        return act
    if plan == 5:                                              # nothing
        return np.zeros(2 * T, dtype=np.int32)
    if plan == "010":                                          # one trajectory per wavefront (generic kernels)
        return np.array([0, 1, 0], dtype=np.int32)
    assert plan == "off"
    return np.zeros(3, dtype=np.int32)


def bad_trajectory(plan, T):
    """The trajectory that gets Cuu = -I at a middle step: never slot 0 of its wavefront where a wavefront has more than one slot.
    Plan 2: the first valid slot of wavefront 1, the one every idle slot there shadows.  Plan 3: a valid slot of wavefront 2 that is
    not the shadowed one.  Plan 5 and "off": an inactive one (nothing may report)."""
    return {1: 1, 2: T + 1, 3: 2 * T + 3, 4: T - 2, 5: 1, "010": 1, "off": 1}[plan]


def problem(n, m, B, N, f, seed, di=False):
    """The recipe of test_regularization_gpu._problem (per-trajectory, time-varying A, B, Hessian stack M M' + I with a Cux block)
    plus the ADMM state; di: A, B of a double integrator with its own (a, b0, b1) per trajectory."""
    rng = np.random.default_rng(seed + 100 * n + m)
    rn = lambda *s: rng.standard_normal(s)                     # noqa: E731
    A = np.eye(n) + AB_SCALE * 0.1 * rn(B, N, n, n) / np.sqrt(n)
    Bm = AB_SCALE * 0.1 * rn(B, N, n, m)
    M = rn(B, N, n + m, n + m) / np.sqrt(n + m)
    C = M @ M.transpose(0, 1, 3, 2) + np.eye(n + m)
    c = dict(A=A, Bm=Bm, Cxx=C[..., :n, :n], Cuu=C[..., n:, n:], Cux=0.3 * C[..., n:, :n], c0x=rn(B, N, n), c0u=rn(B, N, m),
             xhat=rn(B, N, n), uhat=0.3 * rn(B, N, m), zx=rn(B, N, n), lx=0.1 * rn(B, N, n), zu=rn(B, N, m), lu=0.1 * rn(B, N, m))
    c["zu2"] = c["zu"] + 0.2 * rn(B, N, m)                      # the moved consensus variable of a later ADMM iteration
    sym = lambda d: (lambda S: 0.05 * (S + S.transpose(0, 2, 1)))(rn(N, d, d))   # noqa: E731
    ramp = lambda d, w: w * (1 + 0.1 * np.arange(N))[:, None, None] * np.eye(d)  # noqa: E731
    c["Qr"], c["Rr"] = ramp(n, 0.3) + sym(n), ramp(m, 0.5) + sym(m)            # [N,d,d] time-varying
    c["Qr1"], c["Rr1"] = c["Qr"][3 % N][None].copy(), c["Rr"][3 % N][None].copy()   # one [1,d,d] block
    if di:
        d = m
        par = np.array([0.1, 0.005, 0.1]) * (1 + 0.3 * rng.uniform(-1, 1, (B, 3)))
        eye, zero = np.eye(d), np.zeros((d, d))
        c["A"] = np.stack([np.tile(np.block([[eye, p[0] * eye], [zero, eye]]), (N, 1, 1)) for p in par])
        c["Bm"] = np.stack([np.tile(np.vstack([p[1] * eye, p[2] * eye]), (N, 1, 1)) for p in par])
        c["par"] = par
    return {k: np.ascontiguousarray(v).astype(f) for k, v in c.items()}


def prefill(n, m, B, N, f, seed):
    """What the outputs hold before a launch: random words (a constant would hide a copied neighbour)."""
    rng = np.random.default_rng(7919 * seed + n + m)
    shapes = dict(K=(B, N, m, n), Quu=(B, N, m, m), fac=(B, N, m, m), Qux=(B, N, m, n), k=(B, N, m))
    pre = {key: (3.0 + rng.standard_normal(s)).astype(f) for key, s in shapes.items()}
    pre["st"] = (rng.integers(1, 1 << 20, B) << 4).astype(np.int32)            # bits above the defined status bits
    return pre


WEIGHTS = {"tv": ("Qr", "Rr", "zu"), "ti": ("Qr1", "Rr1", "zu"), "ti2": ("Qr1", "Rr1", "zu2")}


def reference(okern, c, pre, act, mode, mu=None, on_x=False, passes=("tv", "ti", "ti2")):
    """The oracle's gain pass, then its sequential feed-forward pass per weight layout, started from the pre-fill."""
    N = c["A"].shape[1]
    out = {key: pre[key].copy() for key in ("K", "Quu", "fac", "Qux", "st")}
    Cxx, Cuu = (c["Cxx"], c["Cuu"]) if mu is None else materialise(c["Cxx"], c["Cuu"], mu, on_x)
    okern.riccati_gain(c["A"], c["Bm"], Cxx, Cuu, out["K"], out["Quu"], out["fac"], out["Qux"], Cux=c["Cux"], solve_mode=mode,
                       status=out["st"], active=act)
    tile = lambda W: np.ascontiguousarray(np.broadcast_to(W, (N,) + W.shape[1:]))   # noqa: E731
    for name in passes:
        Qr, Rr, zu = WEIGHTS[name]
        k = pre["k"].copy()
        okern.riccati_ff(c["A"], c["Bm"], c["c0x"], c["c0u"], out["K"], out["Quu"], out["fac"], out["Qux"], k, Qr=tile(c[Qr]),
                         Rr=tile(c[Rr]), xhat=c["xhat"], uhat=c["uhat"], zx=c["zx"], lx=c["lx"], zu=c[zu], lu=c["lu"], solve_mode=mode,
                         active=act)
        out["k_" + name] = k
    return out


def reference_checked(okern, cs, act, mode, **kw):
    """reference() in the precision of the case.  fp32: the precondition of the 1e-4 bound as well -- on these very inputs and this
    very mask the fp32 oracle stays within a tenth of the tolerance of the fp64 oracle, per trajectory (both are the reference)."""
    ref = reference(okern, cs.c, cs.pre, act, mode, **kw)
    if cs.dtype == "f32" and cs.on.size:
        up = lambda d: {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in d.items()}   # noqa: E731
        kw64 = dict(kw, mu=kw["mu"].astype(np.float64)) if kw.get("mu") is not None else kw
        r64 = reference(okern, up(cs.c), up(cs.pre), act, mode, **kw64)
        margin = max(compare_batched(f"fp32 oracle against fp64 oracle, {key}", ref[key][cs.on], r64[key][cs.on], np.inf)
                     for key in ref if key != "st")
        key = (cs.n, cs.m, cs.N)
        MARGIN[key] = max(MARGIN.get(key, 0.0), margin)
        assert margin < 0.1 * cs.tol, f"fp32 oracle against fp64 oracle at (n, m, N) = {key}: {margin:.3e}"
    return ref


class Guarded:
    """Output arrays inside flat device buffers with GUARD sentinel words in front and behind."""

    def __init__(self):
        self.kept = []

    def _flat(self, size, dt):
        import torch
        flat = torch.full((size + 2 * GUARD,), SENTINEL, dtype=dt, device="cuda")
        self.kept.append(flat)
        return flat[GUARD:GUARD + size]

    def __call__(self, a):
        """a copy of the host array (the pre-fill of an output)"""
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a))
        view = self._flat(t.numel(), t.dtype).view(*a.shape)
        view.copy_(t)
        return view

    def nan(self, dt, *shape):
        view = self._flat(int(np.prod(shape)), dt).view(*shape)
        view.fill_(float("nan"))
        return view

    def assert_intact(self):
        import torch
        edges = torch.cat([torch.cat([f[:GUARD], f[-GUARD:]]).double() for f in self.kept])
        assert bool((edges == SENTINEL).all()), "a guard word was overwritten"
        self.kept = []


class Case:
    """One (pair, mask, N, precision, solve mode): inputs on the device, the comparisons, the forms."""

    def __init__(self, okern, hk, n, m, act, N, dtype, tol, mode, seed, di=False):
        import torch
        self.okern, self.hk, self.n, self.m, self.N, self.dtype, self.tol, self.mode = okern, hk, n, m, N, dtype, tol, mode
        self.f = np.float64 if dtype == "f64" else np.float32
        self.tdt = torch.float64 if dtype == "f64" else torch.float32
        self.act, self.B, self.T = act, int(act.shape[0]), tpw(n, m)
        self.on, self.off = np.flatnonzero(act), np.flatnonzero(act == 0)
        self.c = problem(n, m, self.B, N, self.f, seed, di=di)
        self.pre = prefill(n, m, self.B, N, self.f, seed)
        self.d = {k: torch.from_numpy(v).cuda() for k, v in self.c.items()}
        self.dact = torch.from_numpy(act).cuda()
        self.g = Guarded()
        self.fast = (n, m) in PAIRS

    # -- device buffers ---------------------------------------------------------------------------------------------------------
    def outputs(self, *names):
        return [self.g(self.pre[k]) for k in names]

    def records(self):
        """exactly capi.ff_record_elems words, NaN-filled, between the guard bands"""
        return self.g.nan(self.tdt, capi.ff_record_elems(self.B, self.N, self.n, self.m))

    def gain_args(self, K, Quu=None, fac=None, Qux=None, st=None, rec=None, lin=None, Cuu=None):
        d = self.d
        return capi.Kernels.gain_args(d["A"], d["Bm"], d["Cxx"], d["Cuu"] if Cuu is None else Cuu, K, Quu, fac, Qux, Cux=d["Cux"],
                                      solve_mode=self.mode, status=st, active=self.dact, rec=rec, lin=lin)

    def ff_args(self, K, k, weights, Quu=None, fac=None, Qux=None, rec=None, lin=None, seg=None):
        d = self.d
        Qr, Rr, zu = WEIGHTS[weights]
        return capi.Kernels.ff_args(d["A"], d["Bm"], d["c0x"], d["c0u"], K, Quu, fac, Qux, k, Qr=d[Qr], Rr=d[Rr], xhat=d["xhat"],
                                    uhat=d["uhat"], zx=d["zx"], lx=d["lx"], zu=d[zu], lu=d["lu"], solve_mode=self.mode, active=self.dact,
                                    rec=rec, lin=lin, seg=seg)

    # -- comparisons ------------------------------------------------------------------------------------------------------------
    def check(self, form, name, got, ref):
        """active trajectories per trajectory against the oracle (every word finite), inactive ones bit-equal to the pre-fill"""
        got = got.cpu().numpy()
        pre = self.pre["k" if name.startswith("k") else name]
        assert np.array_equal(got[self.off], pre[self.off]), f"{form} {name} N = {self.N}: an inactive trajectory was written"
        on = self.on
        tag = f"{form} {name} N = {self.N}, active trajectories {on.tolist()}"
        if on.size == 0:
            return
        assert np.isfinite(got[on]).all(), f"{tag}: non-finite words in trajectories {on[~np.isfinite(got[on]).reshape(on.size, -1).all(axis=1)].tolist()}"
        err = compare_batched(tag, got[on], ref[on], self.tol)
        key = (form, self.dtype)
        WORST[key] = max(WORST.get(key, 0.0), err)

    def check_status(self, form, st, ref):
        assert np.array_equal(st.cpu().numpy(), ref), f"{form}: status {st.cpu().numpy().tolist()} != oracle {ref.tolist()}"

    def check_records(self, form, rec, lean=False):
        """[blocks][N][T][stride]: finite for t < N-1 where the trajectory is active; a wavefront without one writes nothing"""
        n, m, N, T = self.n, self.m, self.N, self.T
        mw = 6 if (n, m) in ((9, 3), (4, 2)) else 0
        used = m * n + m * m if lean else n * n + 2 * n * m + m * m + mw   # (lean: [K | fac]; the structured pass stages no model words)
        stride = ((m * n + m * m if lean else n * n + 2 * n * m + m * m) + mw + 1) & ~1
        blocks = -(-self.B // T)
        r = rec.cpu().numpy()
        assert np.isnan(r[blocks * N * T * stride:]).all(), f"{form}: words behind the records were written"
        r = r[:blocks * N * T * stride].reshape(blocks, N, T, stride)
        for b in range(blocks * T):
            blk, s = divmod(b, T)
            if b < self.B and self.act[b]:
                assert np.isfinite(r[blk, :N - 1, s, :used]).all(), f"{form}: record words of trajectory {b} are not finite"
        for blk in range(blocks):
            if not self.act[blk * T:(blk + 1) * T].any():
                assert np.isnan(r[blk]).all(), f"{form}: wavefront {blk} has no trajectory and wrote records"

    def finish(self):
        import torch
        torch.cuda.synchronize()
        self.g.assert_intact()

    # -- the forms --------------------------------------------------------------------------------------------------------------
    def form_arrays(self, ref, reg=None, passes=("tv", "ti")):
        """a (e with reg = (mu, on_x)): gain into K, Quu, fac, Qux, status; riccati_ff on the arrays"""
        form = "arrays" if reg is None else "reg arrays"
        K, Quu, fac, Qux, st = self.outputs("K", "Quu", "fac", "Qux", "st")
        g = self.gain_args(K, Quu, fac, Qux, st)
        self.hk._call("riccati_gain", self.dtype, g, None) if reg is None else self.hk.riccati_gain_reg(g, None, reg[0], reg[1], self.dtype)
        ks = {}
        for w in passes:
            ks[w], = self.outputs("k")
            self.hk._call("riccati_ff", self.dtype, self.ff_args(K, ks[w], w, Quu, fac, Qux), None)
        for name, got in (("K", K), ("Quu", Quu), ("fac", fac), ("Qux", Qux)):
            self.check(form, name, got, ref[name])
        for w in passes:
            self.check(form, "k_" + w, ks[w], ref["k_" + w])
        self.check_status(form, st, ref["st"])
        return K, Quu, fac, Qux

    def form_records(self, ref, reg=None, lin=None):
        """b (d with lin, e with reg): gain into K and the records; feed-forward passes on the records with time-varying weights
        (riccati_ffrec_kernel), with one block (riccati_ffrec2_kernel), and once more with a moved zu"""
        form = "records" if reg is None and lin is None else ("reg records" if lin is None else "hint records")
        (K, st), rec = self.outputs("K", "st"), self.records()
        g = self.gain_args(K, st=st, rec=rec, lin=lin)
        self.hk._call("riccati_gain", self.dtype, g, None) if reg is None else self.hk.riccati_gain_reg(g, None, reg[0], reg[1], self.dtype)
        ks = {}
        for w in (("tv", "ti", "ti2") if lin is None else ("ti", "ti2")):      # the hint goes with one-block weights only
            ks[w], = self.outputs("k")
            self.hk._call("riccati_ff", self.dtype, self.ff_args(K, ks[w], w, rec=rec, lin=lin), None)
        self.check(form, "K", K, ref["K"])
        for w, k in ks.items():
            self.check(form, "k_" + w, k, ref["k_" + w])
        self.check_status(form, st, ref["st"])
        self.check_records(form, rec, lean=lin is not None)
        return K, rec

    def form_fused(self, ref, reg=None, lin=None):
        """c (d, e): the first feed-forward pass inside the gain pass, then a record pass with the moved zu"""
        form = "fused" if reg is None and lin is None else ("reg fused" if lin is None else "hint fused")
        (K, k, k2, st), rec = self.outputs("K", "k", "k", "st"), self.records()
        g, ff = self.gain_args(K, st=st, rec=rec, lin=lin), self.ff_args(K, k, "ti", rec=rec, lin=lin)
        if (self.n, self.m) not in FUSED:                      # the refusal include/isls_hip.h documents for both entry points
            with pytest.raises(capi.IslsError, match=f"-> {capi.ERR_UNSUPPORTED}"):
                self.hk.riccati_gain_ff(g, ff, self.dtype) if reg is None else self.hk.riccati_gain_reg(g, ff, reg[0], reg[1], self.dtype)
            for name, got in (("K", K), ("k", k), ("st", st)):
                assert np.array_equal(got.cpu().numpy(), self.pre[name]), f"{form}: the refused call wrote {name}"
            return None
        self.hk.riccati_gain_ff(g, ff, self.dtype) if reg is None else self.hk.riccati_gain_reg(g, ff, reg[0], reg[1], self.dtype)
        self.hk._call("riccati_ff", self.dtype, self.ff_args(K, k2, "ti2", rec=rec, lin=lin), None)
        self.check(form, "K", K, ref["K"])
        self.check(form, "k_ti", k, ref["k_ti"])
        self.check(form, "k_ti2", k2, ref["k_ti2"])
        self.check_status(form, st, ref["st"])
        self.check_records(form, rec, lean=lin is not None)
        return K

    def form_segments(self, ref, arrays, K_rec, rec):
        """f: isls_riccati_ff_prepare, the segmented pass and the stitch in two segments, from the arrays and from the records"""
        nseg, seg_len = self.hk.ff_segments(self.N, 2)
        assert nseg == 2
        B, N, n, m = self.B, self.N, self.n, self.m
        K, Quu, fac, Qux = arrays
        for src, Ks, kw_ff in (("arrays", K, dict(Quu=Quu, fac=fac, Qux=Qux)), ("records", K_rec, dict(rec=rec))):
            ops = [self.g.nan(self.tdt, B, N, m, n), self.g.nan(self.tdt, B, nseg, n, n), self.g.nan(self.tdt, B, nseg, n)]
            seg = capi.Kernels.ff_seg(*ops, seg_len)
            if src == "arrays":
                self.hk.riccati_ff_prepare(self.d["A"], self.d["Bm"], K, Quu, fac, Qux, seg, solve_mode=self.mode, active=self.dact)
            else:
                self.hk.riccati_ff_prepare(self.d["A"], self.d["Bm"], Ks, None, None, None, seg, solve_mode=self.mode, active=self.dact, rec=rec)
            for w in ("tv", "ti"):
                k, = self.outputs("k")
                self.hk._call("riccati_ff", self.dtype, self.ff_args(Ks, k, w, seg=seg, **kw_ff), None)
                self.check("segments " + src, "k_" + w, k, ref["k_" + w])
            for name, op in zip(("G", "Psi", "v"), ops):       # an inactive trajectory has no operators
                assert np.isnan(op.cpu().numpy()[self.off]).all(), f"segments {src}: {name} of an inactive trajectory was written"

    def form_not_pd(self, ref, bad, K_arrays, K_records):
        """Cuu = -I at a middle step of trajectory `bad`: exactly that trajectory reports NOT_PD (if it is active), in the oracle too;
        every other active trajectory keeps the K of the run without it, bit for bit"""
        import torch
        t_bad = (self.N - 1) // 2                              # <= N-2: a step of the recursion
        Cuu = self.c["Cuu"].copy()
        Cuu[bad, t_bad] = -np.eye(self.m, dtype=self.f)
        ost = self.pre["st"].copy()
        junk = [self.pre[k].copy() for k in ("K", "Quu", "fac", "Qux")]
        with np.errstate(all="ignore"):
            self.okern.riccati_gain(self.c["A"], self.c["Bm"], self.c["Cxx"], Cuu, *junk, Cux=self.c["Cux"], solve_mode=self.mode, status=ost, active=self.act)
        want = self.pre["st"].copy()
        if self.act[bad]:
            want[bad] |= ST_NOT_PD
        # (SOLVE_INV: the oracle inverts Quu by LU like the reference's np.linalg.inv, sls.py:149, and reports a singular block only;
        # -I + B'VB is invertible, so there it reports nothing.  The device factors by Cholesky in both modes and reports.)
        assert np.array_equal(ost, want if self.mode == capi.SOLVE_CHOL else self.pre["st"]), "oracle: NOT_PD is not reported for exactly the bad trajectory"
        dCuu = torch.from_numpy(Cuu).cuda()
        others = self.on[self.on != bad]
        for form, base in (("arrays", K_arrays), ("records", K_records)):
            if base is None:
                continue
            K, st = self.outputs("K", "st")
            if form == "arrays":
                Quu, fac, Qux = self.outputs("Quu", "fac", "Qux")
                g = self.gain_args(K, Quu, fac, Qux, st, Cuu=dCuu)
            else:
                g = self.gain_args(K, st=st, rec=self.records(), Cuu=dCuu)
            self.hk._call("riccati_gain", self.dtype, g, None)
            self.check_status("not-PD " + form, st, want)
            got, ref_K = K.cpu().numpy(), base.cpu().numpy()
            assert np.array_equal(got[others], ref_K[others]), f"not-PD {form}: a neighbour's K changed"
            assert np.array_equal(got[self.off], self.pre["K"][self.off]), f"not-PD {form}: an inactive trajectory was written"


def _mu(B, f, seed):
    """six decades, no two equal, in an order that has nothing to do with the slots"""
    mu = 10.0 ** np.linspace(-3.0, 3.0, max(B, 2))[:B]
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(mu).astype(f))


def _report():
    print("worst per-trajectory error so far: " + ", ".join(f"{form} {dt}: {e:.2e}" for (form, dt), e in sorted(WORST.items())))
    if MARGIN:
        print(f"fp32 oracle against fp64 oracle, worst (pair, N): {max(MARGIN.values()):.2e}")


def _run(okern, n, m, plan, dtype, tol, mode):
    import torch
    from dual import hip_kernels
    hk = hip_kernels()
    T = tpw(n, m)
    act, bad = plan_mask(plan, T), bad_trajectory(plan, T)
    for N in NS:
        seed = 10 * N + (plan if isinstance(plan, int) else 6)
        cs = Case(okern, hk, n, m, act, N, dtype, tol, mode, seed)
        ref = reference_checked(okern, cs, act, mode)
        arrays = cs.form_arrays(ref)                                           # a
        K_rec = rec = None
        if cs.fast:
            K_rec, rec = cs.form_records(ref)                                  # b
            cs.form_fused(ref)                                                 # c
            if N > 2:
                cs.form_segments(ref, arrays, K_rec, rec)                      # f
        cs.form_not_pd(ref, bad, arrays[0], K_rec)
        cs.finish()
        # e: the regularised pass, every trajectory with its own mu; on Cxx as well except at N = 7
        mu, on_x = _mu(cs.B, cs.f, seed), N != 7
        reg = (torch.from_numpy(mu).cuda(), on_x)
        ref = reference_checked(okern, cs, act, mode, mu=mu, on_x=on_x)
        cs.form_arrays(ref, reg=reg, passes=("tv",))
        if cs.fast:
            cs.form_records(ref, reg=reg)
            cs.form_fused(ref, reg=reg)
        cs.finish()
        # d: the model hint on a double integrator with its own parameters per trajectory: lean records in both passes
        if (n, m) in DI:
            cd = Case(okern, hk, n, m, act, N, dtype, tol, mode, seed, di=True)
            ref = reference_checked(okern, cd, act, mode, passes=("ti", "ti2"))
            lin = (capi.MODEL_DI, cd.d["par"])
            K_lean, _ = cd.form_records(ref, lin=lin)
            K_fused = cd.form_fused(ref, lin=lin)
            (K_dense, st), rec = cd.outputs("K", "st"), cd.records()
            hk._call("riccati_gain", dtype, cd.gain_args(K_dense, st=st, rec=rec), None)
            cd.check("hint dense", "K", K_dense, ref["K"])
            if dtype == "f64":                                 # the contract of the hint: the dense pass's bits on the same mask
                assert np.array_equal(K_lean.cpu().numpy(), K_dense.cpu().numpy()), "K with the hint differs from the dense pass"
                assert np.array_equal(K_fused.cpu().numpy(), K_dense.cpu().numpy()), "K with the hint (fused) differs from the dense pass"
            cd.finish()
    _report()


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("plan", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n,m", PAIRS)
def test_slot_edges(oracle, n, m, plan, mode, dtype, tol):
    _run(oracle, n, m, plan, dtype, tol, mode)


@pytest.mark.parametrize("dtype,tol", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("plan", ["010", "off"])
def test_slot_edges_generic(oracle, plan, mode, dtype, tol):
    """(5, 2): the generic kernels, one trajectory per wavefront, array forms only"""
    _run(oracle, 5, 2, plan, dtype, tol, mode)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 1e-4)])
@pytest.mark.parametrize("plan", [2, 3])
@pytest.mark.parametrize("n,m,C", [(6, 3, 4), (2, 1, 2), (6, 3, 2)])
def test_columns_rollout_rows_masks(n, m, C, plan, dtype, tol):
    """g: columns_rollout_rows_kernel with C = 1 + dim columns ((6, 3): dim 3, (2, 1): dim 1; (6, 3) with two columns as well, where
    three problems share a wavefront).  Its slots hold 64 // (C (n + m)) problems: the plans are taken at that count."""
    from columns_reference import check_columns_rollout
    for N in (7, 8):
        check_columns_rollout(n, m, C, N, dtype, tol, active=plan_mask(plan, 64 // (C * (n + m))))
