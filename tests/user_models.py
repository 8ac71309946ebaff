"""Sources of user models (isls.models.Custom) shared by the user-model tests and tools/user_model_bench.py: the car and the
3R arm restated with the built-ins' operation order, and a planar quadrotor that has no built-in model, with its numpy form."""
import numpy as np

# ISLS_MODEL_CAR (csrc/rollout_kernel.hpp), operation for operation
CAR = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    const P dt = par[0];
    S sn, cs;
    isls::sin_cos(x[2], sn, cs);
    xn[0] = x[0] + dt * x[3] * cs;
    xn[1] = x[1] + dt * x[3] * sn;
    xn[2] = isls::py_mod(x[2] + dt * x[3] * u[0], P(2 * 3.14159265358979323846));
    xn[3] = x[3] + dt * u[1];
}
'''

# ISLS_MODEL_ARM3R, operation for operation
ARM3R = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    const P dt = par[0];
    S c = S(0), ex = S(0), ey = S(0);
    for (int j = 0; j < 3; ++j) {
        xn[j] = x[j] + x[3 + j] * dt + P(0.5) * u[j] * (dt * dt);
        xn[3 + j] = x[3 + j] + u[j] * dt;
    }
    for (int j = 0; j < 3; ++j) {
        c += xn[j];
        S sn, cs;
        isls::sin_cos(c, sn, cs);
        ex += cs;
        ey += sn;
    }
    xn[6] = ex; xn[7] = ey; xn[8] = S(0);
}
'''

# planar quadrotor [px, py, theta, vx, vy, omega], u = [thrust 1, thrust 2]; par = [dt, mass, inertia, arm, g]
QUAD = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    const P dt = par[0], mass = par[1], inertia = par[2], arm = par[3], g = par[4];
    const S f = u[0] + u[1];
    const S s = sin(x[2]), c = cos(x[2]);
    const S ax = -(f * s) / mass, ay = (f * c) / mass - g, al = arm * (u[0] - u[1]) / inertia;
    xn[0] = x[0] + dt * x[3];
    xn[1] = x[1] + dt * x[4];
    xn[2] = x[2] + dt * x[5];
    xn[3] = x[3] + dt * ax;
    xn[4] = x[4] + dt * ay;
    xn[5] = x[5] + dt * al;
}
'''
QUAD_PAR = np.array([0.05, 1.0, 0.02, 0.15, 9.81])


def quad_numpy(par=QUAD_PAR):
    """(f, get_AB) of QUAD on numpy in the reference's calling convention."""
    dt, mass, inertia, arm, g = par

    def f(x, u):
        fz = u[..., 0] + u[..., 1]
        s, c = np.sin(x[..., 2]), np.cos(x[..., 2])
        ax, ay, al = -(fz * s) / mass, (fz * c) / mass - g, arm * (u[..., 0] - u[..., 1]) / inertia
        return np.stack([x[..., 0] + dt * x[..., 3], x[..., 1] + dt * x[..., 4], x[..., 2] + dt * x[..., 5],
                         x[..., 3] + dt * ax, x[..., 4] + dt * ay, x[..., 5] + dt * al], axis=-1)

    def get_AB(x, u):
        N = x.shape[0]
        fz = u[:, 0] + u[:, 1]
        s, c = np.sin(x[:, 2]), np.cos(x[:, 2])
        A, B = np.tile(np.eye(6), (N, 1, 1)), np.zeros((N, 6, 2))
        A[:, 0, 3] = A[:, 1, 4] = A[:, 2, 5] = dt
        A[:, 3, 2], A[:, 4, 2] = -dt * fz * c / mass, -dt * fz * s / mass
        B[:, 3, 0] = B[:, 3, 1] = -dt * s / mass
        B[:, 4, 0] = B[:, 4, 1] = dt * c / mass
        B[:, 5, 0], B[:, 5, 1] = dt * arm / inertia, -dt * arm / inertia
        return A, B
    return f, get_AB


# ---- the contract zoo -------------------------------------------------------------------------------------------------------
# Five sources that, with CAR, ARM3R and QUAD, use every item of the contract of csrc/user_model_ad.hpp at least once and cover the
# eight supported (n, m) pairs.  Each has a restatement as a plain Python function f(x, u, par, M) on scalars: M supplies the
# elementary functions (mpmath for the 60-digit reference, torch for the same-precision baseline, numpy for the host path), and
# `margin(x, u, par)` gives the distances of a point from the model's kinks and wraps.  Every literal is exact in fp32, so that
# the fp32 instantiation evaluates the same function.

# (6, 3): arithmetic and comparisons.  par = [a, mode]
Z63 = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    const P a = par[0];
    S t = x[0];
    t += u[0]; t -= 0.25; t *= x[1]; t /= x[1] * x[1] + 1.0; t += 1.5; t -= u[1]; t *= 2; t /= 4;
    xn[0] = t;
    xn[1] = x[1] / (x[0] * x[0] + 1.0) + 2.0 / (u[0] * u[0] + 2.0);
    xn[2] = (0.5 - x[2]) * u[1] - (x[1] - 0.5) + x[2] / 2 + S(1.5) + a * x[0];
    xn[3] = -x[3] + (+x[4]) * u[2] - (-(x[3] * x[3]));
    S r;
    if (x[4] < 0.25) r = x[4] * x[4]; else r = 3.0 * x[4];
    if (x[5] <= x[3]) r += x[5] * u[0];
    if (1.0 > x[5]) r -= 0.5 * x[5] * x[5];
    if (x[4] >= x[5]) r += x[4] * x[5];
    if (0.25 <= x[3]) r *= 2.0;
    xn[4] = r;
    const S mode = S(par[1]);
    if (mode == 1.0) xn[5] = x[5] * x[0];
    else if (2.0 != mode) xn[5] = x[5] + x[0] * x[0];
    else xn[5] = x[5] - u[2] * x[0];
    if (mode != S(0)) xn[5] += u[1];
}
'''


def z63_f(x, u, par, M):
    a, mode = par
    t = x[0]
    t = t + u[0]; t = t - 0.25; t = t * x[1]; t = t / (x[1] * x[1] + 1.0); t = t + 1.5; t = t - u[1]; t = t * 2; t = t / 4
    x1 = x[1] / (x[0] * x[0] + 1.0) + 2.0 / (u[0] * u[0] + 2.0)
    x2 = (0.5 - x[2]) * u[1] - (x[1] - 0.5) + x[2] / 2 + 1.5 + a * x[0]
    x3 = -x[3] + x[4] * u[2] + x[3] * x[3]
    r = x[4] * x[4] if x[4] < 0.25 else 3.0 * x[4]
    if x[5] <= x[3]:
        r = r + x[5] * u[0]
    if 1.0 > x[5]:
        r = r - 0.5 * x[5] * x[5]
    if x[4] >= x[5]:
        r = r + x[4] * x[5]
    if 0.25 <= x[3]:
        r = r * 2.0
    if mode == 1.0:
        x5 = x[5] * x[0]
    elif mode != 2.0:
        x5 = x[5] + x[0] * x[0]
    else:
        x5 = x[5] - u[2] * x[0]
    if mode != 0:
        x5 = x5 + u[1]
    return [t, x1, x2, x3, r, x5]


def z63_margin(x, u, par):
    return [abs(x[4] - 0.25), abs(x[5] - x[3]), abs(x[5] - 1.0), abs(x[4] - x[5]), abs(x[3] - 0.25)]


# (3, 3): sqrt, log, exp; the parameters enter nonlinearly.  par = [k, c]
Z33 = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    const P k = par[0], c = par[1];
    xn[0] = sqrt(x[0]) + u[0];
    xn[1] = log(x[1]) * u[1];
    xn[2] = exp(k * x[2]) * u[2] + c / (k * k + 1);
}
'''


def z33_f(x, u, par, M):
    k, c = par
    return [M.sqrt(x[0]) + u[0], M.log(x[1]) * u[1], M.exp(k * x[2]) * u[2] + c / (k * k + 1)]


def z33_margin(x, u, par):
    return [1.0 if x[0] > 0 and x[1] > 0 else 0.0]                     # no kink inside the domain: only stay in it


# (3, 1): tanh, asin, fabs.  par = [a]
Z31 = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    xn[0] = tanh(x[0]) * u[0] + par[0];
    xn[1] = asin(x[1]) + x[0];
    xn[2] = fabs(x[2]) * x[0] + fabs(u[0] - 0.5);
}
'''


def z31_f(x, u, par, M):
    return [M.tanh(x[0]) * u[0] + par[0], M.asin(x[1]) + x[0], M.fabs(x[2]) * x[0] + M.fabs(u[0] - 0.5)]


def z31_margin(x, u, par):
    return [abs(x[2]), abs(u[0] - 0.5), 1.0 - abs(x[1])]


# (2, 2): the three forms of atan2.  par = [a]
Z22 = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    xn[0] = atan2(x[0], x[1]);
    xn[1] = par[0] * atan2(1.0, u[0]) + atan2(u[1], 2.0);
}
'''


def z22_f(x, u, par, M):
    return [M.atan2(x[0], x[1]), par[0] * M.atan2(1.0, u[0]) + M.atan2(u[1], 2.0)]


def z22_margin(x, u, par):
    # the cut of atan2(y, x) is the negative x axis; the origin is its end
    return [abs(x[0]) if x[1] <= 0 else max(abs(x[0]), abs(x[1]))]


# (2, 1): py_mod with a dual divisor, a negative plain divisor and a plain dividend, and plain numbers of another type inside
# the calls of the two helpers (for S = float their sums are doubles).  par = [d]
Z21 = r'''
template <typename S, typename P>
__device__ void step(const S *x, const S *u, const P *par, S *xn) {
    xn[0] = isls::py_mod(x[0], x[1] * x[1] + 1.0);
    S s, c;
    isls::sin_cos(x[0] + 1.0, s, c);
    xn[1] = isls::py_mod(u[0], -par[0]) + s * c + isls::py_mod(7.25, x[1] * x[1] + 1.5);
}
'''


def z21_f(x, u, par, M):
    return [M.mod(x[0], x[1] * x[1] + 1.0),
            M.mod(u[0], -par[0]) + M.sin(x[0] + 1.0) * M.cos(x[0] + 1.0) + M.mod(7.25, x[1] * x[1] + 1.5)]


def _wrap_margin(a, b):
    """distance of a from the next multiple of b, over max(1, |quotient|): how far b may move before a wraps as well"""
    q = np.floor(a / b)
    r = a - q * b
    return min(abs(r), abs(b) - abs(r)) / max(1.0, abs(q))


def z21_margin(x, u, par):
    return [_wrap_margin(x[0], x[1] * x[1] + 1.0), _wrap_margin(u[0], -par[0]), _wrap_margin(7.25, x[1] * x[1] + 1.5)]


def car_f(x, u, par, M):
    dt = par[0]
    return [x[0] + dt * x[3] * M.cos(x[2]), x[1] + dt * x[3] * M.sin(x[2]),
            M.mod(x[2] + dt * x[3] * u[0], 2 * 3.14159265358979323846), x[3] + dt * u[1]]


def car_margin(x, u, par):
    return [_wrap_margin(x[2] + par[0] * x[3] * u[0], 2 * np.pi)]


def arm_f(x, u, par, M):
    dt = par[0]
    q = [x[j] + x[3 + j] * dt + 0.5 * u[j] * (dt * dt) for j in range(3)]
    qd = [x[3 + j] + u[j] * dt for j in range(3)]
    c, ex, ey = 0, 0, 0
    for j in range(3):
        c = c + q[j]
        ex, ey = ex + M.cos(c), ey + M.sin(c)
    return q + qd + [ex, ey, 0 * x[8]]


def quad_f(x, u, par, M):
    dt, mass, inertia, arm, g = par
    f = u[0] + u[1]
    s, c = M.sin(x[2]), M.cos(x[2])
    ax, ay, al = -(f * s) / mass, (f * c) / mass - g, arm * (u[0] - u[1]) / inertia
    return [x[0] + dt * x[3], x[1] + dt * x[4], x[2] + dt * x[5], x[3] + dt * ax, x[4] + dt * ay, x[5] + dt * al]


def _no_kinks(x, u, par):
    return []


# name -> (n, m, source, f, margin); the parameter rows and the points are the fixture's (tests/golden/make_ad_contract.py)
NPAR = {"z63": 2, "z33": 2, "z31": 1, "z22": 1, "z21": 1, "car": 1, "arm": 1, "quad": 5}
ZOO = {
    "z63": (6, 3, Z63, z63_f, z63_margin),
    "z33": (3, 3, Z33, z33_f, z33_margin),
    "z31": (3, 1, Z31, z31_f, z31_margin),
    "z22": (2, 2, Z22, z22_f, z22_margin),
    "z21": (2, 1, Z21, z21_f, z21_margin),
    "car": (4, 2, CAR, car_f, car_margin),
    "arm": (9, 3, ARM3R, arm_f, _no_kinks),
    "quad": (6, 2, QUAD, quad_f, _no_kinks),
}
