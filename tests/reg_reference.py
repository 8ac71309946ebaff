"""numpy restatement of the regularisation schedule (include/isls_hip.h: isls_reg_update_*) and of the gain pass's retry loop,
built on the unchanged C oracle: the oracle's gain pass is handed materialised per-trajectory tables Cuu + mu I (and
Cxx + mu I for t <= N-2)."""
import numpy as np

ST_NOT_PD, ST_LS_REJECT, ST_REG_MAX = 1, 4, 8


class Schedule:
    """mu / delta per trajectory in the solver's dtype; every step is one rounded operation, as on the device."""

    def __init__(self, B, dtype, mu_init=0.0, mu_min=1e-6, mu_max=1e10, factor=1.6):
        f = np.dtype(dtype).type
        self.f, self.factor, self.mu_min, self.mu_max = f, f(factor), f(mu_min), f(mu_max)
        self.mu, self.delta = np.full(B, mu_init, dtype=f), np.ones(B, dtype=f)

    def raise_(self, b):
        """True when mu[b] rose; False when the raise would pass mu_max (mu, delta stay)."""
        d = max(self.factor, self.f(self.delta[b] * self.factor))
        v = max(self.mu_min, self.f(self.mu[b] * d))
        if not v <= self.mu_max:
            return False
        self.delta[b], self.mu[b] = d, v
        return True

    def lower(self, b):
        d = min(self.f(self.f(1) / self.factor), self.f(self.delta[b] / self.factor))
        v = self.f(self.mu[b] * d)
        self.delta[b], self.mu[b] = d, (v if v >= self.mu_min else self.f(0))


def materialise(Cxx, Cuu, mu, on_x):
    """Per-trajectory tables [B,N,.,.] with mu_b on the diagonal for t <= N-2 (the terminal block is left alone)."""
    B = mu.shape[0]
    Cxx = np.array(np.broadcast_to(Cxx, (B,) + Cxx.shape[-3:]), dtype=Cxx.dtype)
    Cuu = np.array(np.broadcast_to(Cuu, (B,) + Cuu.shape[-3:]), dtype=Cuu.dtype)
    n, m = Cxx.shape[-1], Cuu.shape[-1]
    iu, ix = np.arange(m), np.arange(n)
    Cuu[:, :-1, iu, iu] += mu[:, None, None]
    if on_x:
        Cxx[:, :-1, ix, ix] += mu[:, None, None]
    return Cxx, Cuu


def gain(okern, A, Bm, Cxx, Cuu, mu, on_x, out, solve_mode=0, status=None, active=None, Cux=None):
    """The oracle's gain pass on the materialised tables; out = (K, Quu, fac, Qux)."""
    Cx, Cu = materialise(Cxx, Cuu, mu, on_x)
    okern.riccati_gain(A, Bm, Cx, Cu, *out, Cux=Cux, solve_mode=solve_mode, status=status, active=active)


def gain_with_retries(okern, A, Bm, Cxx, Cuu, sched, on_x, out, status, solve_mode=0, active=None):
    """The retry loop: pass, raise mu where Quu was not positive definite (and clear the bit), again while anything rose.
    Returns the number of gain passes."""
    B = status.shape[0]
    act = np.ones(B, dtype=bool) if active is None else active.astype(bool)
    launches = 0
    while True:
        gain(okern, A, Bm, Cxx, Cuu, sched.mu, on_x, out, solve_mode=solve_mode, status=status, active=active)
        launches += 1
        retry = 0
        for b in range(B):
            if act[b] and (status[b] & ST_NOT_PD) and not (status[b] & ST_REG_MAX):
                if sched.raise_(b):
                    status[b] &= ~ST_NOT_PD
                    retry += 1
                else:
                    status[b] |= ST_REG_MAX
        if retry == 0:
            return launches


# ---- the regularised `solve` loop (isls/isls.py `solve` with regularization=), fp64 ---------------------------------------
ALPHAS = 10.0 ** np.linspace(0.0, -5.0, 50)


class ViaCost:
    """sum_t (x_t - z_t)'Q_t(x_t - z_t) + u_std |u_t|^2 (no 1/2) and its expansion"""

    def __init__(self, zs, Qs, seq, u_std):
        self.z, self.Q, self.u_std = np.asarray(zs)[seq], np.asarray(Qs)[seq], float(u_std)

    def value(self, x, u):
        d = x - self.z
        return np.einsum("...ti,tij,...tj->...", d, self.Q, d) + self.u_std * np.sum(u * u, axis=(-1, -2))

    def expand(self, x, u):
        B, N, n = x.shape
        m = u.shape[-1]
        Qs = self.Q + self.Q.transpose(0, 2, 1)
        c0x = np.einsum("tij,btj->bti", Qs, x - self.z)
        Cxx = np.broadcast_to(Qs, (B, N, n, n)).copy()
        Cuu = np.broadcast_to(2 * self.u_std * np.eye(m), (B, N, m, m)).copy()
        return c0x, 2 * self.u_std * u, Cxx, Cuu, np.zeros((B, N, m, n))


def solve(okern, f, get_AB, cost, x_nom, u_nom, max_iter, L, tol_fun=1e-5, reg=None, on_x=False):
    """iLQR with the reference's stop rules per trajectory; reg = dict(mu_init, mu_min, mu_max, factor) or None (the plain loop: a
    Quu that is not positive definite raises LinAlgError, a rejected trajectory stops).  f(x [.., n], u [.., m]) -> x+ ;
    get_AB(x [N, n], u [N, m]) -> (A [N, n, n], B [N, n, m]); cost.value / cost.expand.  Gain and feed-forward passes: the C oracle
    on materialised tables.  Returns dict(costs [it + 1, B], ok [it, B], active [it, B] (going into the iteration), mu [it, B]
    (after it), mu_final, status, x, u)."""
    x, u = np.array(x_nom, dtype=np.float64), np.array(u_nom, dtype=np.float64)
    B, N, n = x.shape
    m = u.shape[-1]
    z = lambda *s: np.zeros(s)                                 # noqa: E731
    sched = Schedule(B, np.float64, **reg) if reg is not None else None
    act, status = np.ones(B, dtype=bool), np.zeros(B, dtype=np.int32)
    cur = cost.value(x, u)
    prev = cur.copy()
    log = dict(costs=[cur.copy()], ok=[], active=[], mu=[])
    K, Quu, fac, Qux, k = z(B, N, m, n), z(B, N, m, m), z(B, N, m, m), z(B, N, m, n), z(B, N, m)
    for _ in range(max_iter):
        log["active"].append(act.copy())
        AB = [get_AB(x[b], u[b]) for b in range(B)]
        A, Bm = np.stack([a[0] for a in AB]), np.stack([a[1] for a in AB])
        c0x, c0u, Cxx, Cuu, Cux = cost.expand(x, u)
        status[act] = 0
        a32 = act.astype(np.int32)
        if sched is None:
            okern.riccati_gain(A, Bm, Cxx, Cuu, K, Quu, fac, Qux, Cux=Cux, status=status, active=a32)
            if (status & ST_NOT_PD).any():
                raise np.linalg.LinAlgError(f"Quu not positive definite for trajectories {np.nonzero(status & ST_NOT_PD)[0].tolist()}")
        else:
            while True:                                        # gain_with_retries, with Cux
                Cx, Cu = materialise(Cxx, Cuu, sched.mu, on_x)
                okern.riccati_gain(A, Bm, Cx, Cu, K, Quu, fac, Qux, Cux=Cux, status=status, active=a32)
                retry = 0
                for b in np.nonzero(act)[0]:
                    if (status[b] & ST_NOT_PD) and not (status[b] & ST_REG_MAX):
                        if sched.raise_(b):
                            status[b] &= ~ST_NOT_PD
                            retry += 1
                        else:
                            status[b] |= ST_REG_MAX
                if retry == 0:
                    break
            act &= (status & ST_NOT_PD) == 0                   # the end of the ladder: that trajectory stops
            a32 = act.astype(np.int32)
        okern.riccati_ff(A, Bm, c0x, c0u, K, Quu, fac, Qux, k, active=a32)
        ok = np.zeros(B, dtype=bool)
        for b in np.nonzero(act)[0]:                           # line search over alphas[:L]: NaN rule, first minimum, acceptance test
            xc, uc = np.zeros((L, N, n)), np.zeros((L, N, m))
            xt = np.tile(x[b, 0], (L, 1))
            for t in range(N):
                ut = (xt - x[b, t]) @ K[b, t].T + ALPHAS[:L, None] * k[b, t] + u[b, t]
                xc[:, t], uc[:, t] = xt, ut
                xt = f(xt, ut)
            costs = cost.value(xc, uc)
            costs[np.isnan(costs)] = 1e5
            best = int(np.argmin(costs))
            if costs[best] < cur[b]:
                ok[b], x[b], u[b], cur[b] = True, xc[best], uc[best], costs[best]
            else:
                status[b] |= ST_LS_REJECT
            if sched is not None:
                if ok[b]:
                    sched.lower(b)
                elif not sched.raise_(b):
                    status[b] |= ST_REG_MAX
        log["ok"].append(ok.copy())
        log["costs"].append(cur.copy())
        log["mu"].append(sched.mu.copy() if sched is not None else np.zeros(B))
        small = np.abs(cur - prev) < tol_fun
        stop = act & ((ok & small) | ((status & ST_REG_MAX) != 0)) if sched is not None else act & ((ok & small) | ~ok)
        prev = np.where(act & ok, cur, prev)
        act = act & ~stop
        if not act.any():
            break
    log = {k_: np.array(v) for k_, v in log.items()}
    log.update(mu_final=sched.mu.copy() if sched is not None else np.zeros(B), status=status, x=x, u=u)
    return log


class BumpCost:
    """Double integrator in the plane, state [px, py, vx, vy]: w_u |u|^2 + w_o exp(-|p - o|^2 / r^2) + w_x |x - g|^2, and
    w_f |x - g|^2 more at the last step (g = [gx, gy, 0, 0]).  par = [w_u, w_o, ox, oy, r, w_x, w_f, gx, gy]: the README's bump."""
    SOURCE = r"""
template <typename S, typename P>
__device__ S stage(const S *x, const S *u, const P *par, int t, int N) {
    const S dx = x[0] - par[2], dy = x[1] - par[3], ex = x[0] - par[7], ey = x[1] - par[8];
    S c = par[0] * (u[0] * u[0] + u[1] * u[1]) + par[1] * exp(-(dx * dx + dy * dy) / (par[4] * par[4]));
    const S d2 = ex * ex + ey * ey + x[2] * x[2] + x[3] * x[3];
    c += par[5] * d2;
    if (t == N - 1) c += par[6] * d2;
    return c;
}"""

    def __init__(self, par):
        self.par = np.asarray(par, dtype=np.float64)

    def _w(self, N):
        w = np.full(N, self.par[5])
        w[-1] += self.par[6]
        return w

    def value(self, x, u):
        wu, wo, ox, oy, r = self.par[:5]
        g = np.array([self.par[7], self.par[8], 0.0, 0.0])
        d2 = (x[..., 0] - ox) ** 2 + (x[..., 1] - oy) ** 2
        st = wu * np.sum(u * u, axis=-1) + wo * np.exp(-d2 / r ** 2) + self._w(x.shape[-2]) * np.sum((x - g) ** 2, axis=-1)
        return st.sum(axis=-1)

    def expand(self, x, u):
        B, N, n = x.shape
        m = u.shape[-1]
        wu, wo, ox, oy, r = self.par[:5]
        g = np.array([self.par[7], self.par[8], 0.0, 0.0])
        w = self._w(N)
        d = x[..., :2] - np.array([ox, oy])
        e = wo * np.exp(-np.sum(d * d, axis=-1) / r ** 2)
        c0x = 2 * w[None, :, None] * (x - g)
        c0x[..., :2] += (-2 / r ** 2) * e[..., None] * d
        Cxx = np.zeros((B, N, n, n))
        Cxx[..., np.arange(n), np.arange(n)] = 2 * w[None, :, None]
        Cxx[..., :2, :2] += e[..., None, None] * (4 / r ** 4 * d[..., :, None] * d[..., None, :] - 2 / r ** 2 * np.eye(2))
        Cuu = np.broadcast_to(2 * wu * np.eye(m), (B, N, m, m)).copy()
        return c0x, 2 * wu * u, Cxx, Cuu, np.zeros((B, N, m, n))
