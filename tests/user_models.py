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
