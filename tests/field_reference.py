"""The 2-D field of costs.Custom(field=) in plain numpy, one point at a time: value, gradient and Hessian analytically from the
weight polynomials of the tensor-product cubic convolution (Keys' kernel at a = -1/2, Catmull-Rom).  A restatement of the
interpolant's definition, not of the device header:

    per axis, p = (pos - origin) / spacing:  pc = clamp(p, 0, n-1),  i = min(floor(pc), n-2),  s = pc - i,
    taps i-1 .. i+2 with their indices clamped to [0, n-1], weights
        w(-1) = (-s^3 + 2 s^2 - s) / 2   w(0) = (3 s^3 - 5 s^2 + 2) / 2   w(1) = (-3 s^3 + 4 s^2 + s) / 2   w(2) = (s^3 - s^2) / 2
    where the clamp acts (p < 0 or p > n-1) the derivative along that axis is zero: a constant continuation outside the grid.
"""
import numpy as np


def axis(pos, origin, spacing, n):
    """(tap indices [4], w [4], dw/dpos [4], d2w/dpos2 [4], the cell i) of one axis"""
    p = (pos - origin) / spacing
    pc = min(max(p, 0.0), n - 1.0)
    i = min(int(np.floor(pc)), n - 2)
    s = pc - i
    w = np.array([-s ** 3 + 2 * s ** 2 - s, 3 * s ** 3 - 5 * s ** 2 + 2, -3 * s ** 3 + 4 * s ** 2 + s, s ** 3 - s ** 2]) / 2
    d1 = np.array([-3 * s ** 2 + 4 * s - 1, 9 * s ** 2 - 10 * s, -9 * s ** 2 + 8 * s + 1, 3 * s ** 2 - 2 * s]) / 2
    d2 = np.array([-6 * s + 4, 18 * s - 10, -18 * s + 8, 6 * s - 2]) / 2
    live = 0.0 if (p < 0.0 or p > n - 1.0) else 1.0
    taps = np.clip(np.arange(i - 1, i + 3), 0, n - 1)
    return taps, w, live * d1 / spacing, live * d2 / spacing ** 2, i


def field(values, origin, spacing, c, px, py):
    """(f, [f_x, f_y], [[f_xx, f_xy], [f_xy, f_yy]]) of channel c of values [C, nx, ny] (or [nx, ny]) at (px, py)"""
    values = np.asarray(values, dtype=np.float64)
    values = values[None] if values.ndim == 2 else values
    c = min(max(int(c), 0), values.shape[0] - 1)
    tx, wx, dx, ddx, _ = axis(float(px), origin[0], spacing[0], values.shape[1])
    ty, wy, dy, ddy, _ = axis(float(py), origin[1], spacing[1], values.shape[2])
    v = values[c][np.ix_(tx, ty)]
    return (wx @ v @ wy, np.array([dx @ v @ wy, wx @ v @ dy]),
            np.array([[ddx @ v @ wy, dx @ v @ dy], [dx @ v @ dy, wx @ v @ ddy]]))


def cell(pos, origin, spacing, n):
    """the cell i of a position (the interpolant is exact on quadratics where 1 <= i <= n-3 on both axes)"""
    return axis(float(pos), origin, spacing, n)[4]


def stage_reference(values, origin, spacing, w, x, u, read=None):
    """(c, gradient [n+m], Hessian [n+m, n+m]) of the stage  w field(0, x0, x1)^2 + field(1, x1, 0.5 x0 + u0)  at one (x, u);
    read(c, px, py) -> (f, grad, Hessian) in the place of the interpolant (a closed form)"""
    n, m = len(x), len(u)
    if read is not None:
        field = lambda values, origin, spacing, c, px, py: read(c, px, py)   # noqa: E731
    else:
        field = globals()["field"]
    f, g, H = field(values, origin, spacing, 0, x[0], x[1])
    J0 = np.zeros((2, n + m))                                # d (x0, x1) / d [x; u]
    J0[0, 0] = J0[1, 1] = 1.0
    h, gh, Hh = field(values, origin, spacing, 1, x[1], 0.5 * x[0] + u[0])
    J1 = np.zeros((2, n + m))                                # d (x1, 0.5 x0 + u0) / d [x; u]
    J1[0, 1], J1[1, 0], J1[1, n] = 1.0, 0.5, 1.0
    gf = J0.T @ g
    grad = 2 * w * f * gf + J1.T @ gh
    hess = 2 * w * (np.outer(gf, gf) + f * (J0.T @ H @ J0)) + J1.T @ Hh @ J1
    return w * f * f + h, grad, hess
