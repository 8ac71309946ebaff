"""Generate tests/golden/g14_ad_contract.npz and g14_sin_cos_{pts,sin,cos}.npz: high-precision references for the dual-number
contract of user models (csrc/user_model_ad.hpp) and for the fp64 isls::sin_cos.  CPU only; needs mpmath.

    python tests/golden/make_ad_contract.py          # writes the files and prints the baseline table

For every model of tests/user_models.ZOO, at 4 x 16 points (4 parameter rows, 16 points each):
  *_x, *_u, *_par   the points and parameter rows: fp64 numbers that are exact in fp32
  *_val             f(x, u) with mpmath at 60 digits
  *_J               [.., n, n+m] central differences of that function in 60-digit arithmetic, step 1e-20 (truncation ~1e-40): no
                    derivative rule is involved, so they share no mistake with the header
  *_base_f64/_f32   per output row, the largest error over the points of torch.autograd.functional.jacobian on the CPU in that
                    dtype against *_J, relative to the largest entry of the reference row: what an independent implementation
                    at the same precision achieves
  *_vbase_f64/_f32  the same for the values (torch on the CPU in that dtype against *_val, relative to the largest component)
Every point is at least 1e-3 away from a kink or a wrap of its model (asserted), so that the central difference and the fp32
evaluation stay on one branch.

sin_cos: 62 000 points (random up to 1e5; at, one ulp beside and within 1e-9 of the first 2000 multiples of pi/2, both signs)
and five edge arguments, with sin and cos from a 200-bit evaluation stored as hi (fp64) + lo (fp32)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import user_models as um  # noqa: E402

sys.path.pop(0)

NB, NP = 4, 16                                                # parameter rows, points per row
MARGIN = 1e-3
D = 2.0 ** -9                                                 # deliberate points sit this far from a switch (1.95e-3)


def r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


class MpOps:
    def __init__(self):
        import mpmath as mp
        self.mp = mp
        for k in ("sin", "cos", "sqrt", "exp", "log", "tanh", "asin", "atan2", "fabs"):
            setattr(self, k, getattr(mp, k))

    def mod(self, a, b):
        a, b = self.mp.mpf(a), self.mp.mpf(b)
        return a - self.mp.floor(a / b) * b


class TorchOps:
    def __init__(self, dtype):
        import torch
        self.t, self.dtype = torch, dtype
        for k in ("sin", "cos", "sqrt", "exp", "log", "tanh", "asin"):
            setattr(self, k, getattr(torch, k))
        self.fabs = torch.abs

    def _t(self, a):
        return a if isinstance(a, self.t.Tensor) else self.t.tensor(a, dtype=self.dtype)

    def atan2(self, y, x):
        return self.t.atan2(self._t(y), self._t(x))

    def mod(self, a, b):
        a, b = self._t(a), self._t(b)
        return a - self.t.floor(a / b) * b


# ---- points -----------------------------------------------------------------------------------------------------------------
def uni(lo, hi):
    return lambda rng, k: rng.uniform(lo, hi, k)


def logu(lo, hi):
    return lambda rng, k: np.exp(rng.uniform(np.log(lo), np.log(hi), k))


def z22_state(rng, k):
    r, a = np.exp(rng.uniform(np.log(0.1), np.log(10.0))), rng.uniform(-np.pi, np.pi)
    return np.array([r * np.sin(a), r * np.cos(a)])

# name -> (draw x, draw u, parameter rows, deliberate points {"x3": value, "u0": value, ...})
SPEC = {
    "z63": (uni(-2, 2), uni(-2, 2), [[0.75, 0], [0.75, 1], [0.75, 2], [-1.5, 1]],
            [{"x4": 0.25 - D}, {"x4": 0.25 + D}, {"x5": 1 - D}, {"x5": 1 + D}, {"x3": 0.25 - D}, {"x3": 0.25 + D},
             {"x3": 0.5, "x5": 0.5 - D}, {"x3": 0.5, "x5": 0.5 + D}, {"x4": -0.75, "x5": -0.75 - D}, {"x4": -0.75, "x5": -0.75 + D}]),
    "z33": (lambda rng, k: np.array([logu(1e-6, 1e6)(rng, 1)[0], logu(1e-6, 1e6)(rng, 1)[0], rng.uniform(-3, 3)]), uni(-2, 2),
            [[0.5, 1.0], [0.25, -2.0], [-0.5, 0.5], [0.125, 3.0]],
            [{"x0": 1e-6, "x1": 1e6}, {"x0": 1e6, "x1": 1e-6}, {"x0": 1.0, "x1": 1.0}]),
    "z31": (lambda rng, k: np.array([rng.uniform(-3, 3), rng.uniform(-0.99, 0.99), rng.uniform(-2, 2)]), uni(-2, 2),
            [[0.5], [0.5], [-1.0], [2.0]],
            [{"x1": 0.99}, {"x1": -0.99}, {"x2": D}, {"x2": -D}, {"u0": 0.5 + D}, {"u0": 0.5 - D}, {"x1": 0.0, "x0": 0.0}]),
    "z22": (z22_state, uni(-3, 3), [[1.5], [1.5], [-0.5], [2.0]],
            [{"x0": 1.0, "x1": 0.0}, {"x0": -1.0, "x1": 0.0}, {"x0": 0.0, "x1": 1.0}, {"x0": 0.0078125, "x1": -1.0},
             {"x0": -0.0078125, "x1": -1.0}, {"x0": 1.0, "x1": 1.0}, {"x0": 1.0, "x1": -1.0}, {"x0": -1.0, "x1": -1.0},
             {"x0": -1.0, "x1": 1.0}, {"u0": 0.0, "u1": 0.0}]),
    "z21": (lambda rng, k: np.array([rng.uniform(-20, 20), rng.uniform(-2, 2)]), uni(-10, 10), [[2.5], [2.5], [1.25], [3.0]],
            [{"x1": 1.0, "x0": 4 - 2 * D}, {"x1": 1.0, "x0": 4 + 2 * D}, {"x1": 1.0, "x0": -4 - 2 * D}, {"x1": 1.0, "x0": -4 + 2 * D},
             {"x1": -1.0, "x0": -0.5}, {"u0": 5 - 2 * D}, {"u0": 5 + 2 * D}, {"u0": -5 - 2 * D}, {"u0": -5 + 2 * D}]),
    "car": (lambda rng, k: np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-7, 7), rng.uniform(-3, 3)]), uni(-1, 1),
            [[0.125], [0.125], [0.0625], [0.25]], []),
    "arm": (uni(-2, 2), uni(-1, 1), [[0.0625], [0.0625], [0.125], [0.03125]], []),
    "quad": (uni(-2, 2), uni(0, 8), [r32(um.QUAD_PAR), r32(um.QUAD_PAR), r32([0.0625, 1.5, 0.03125, 0.25, 9.81]),
                                     r32([0.03125, 0.75, 0.015625, 0.125, 1.625])], []),
}


def points(name):
    n, m, _, _, margin = um.ZOO[name]
    dx, du, par, special = SPEC[name]
    rng = np.random.default_rng([14, sorted(SPEC).index(name)])
    par = r32(par)
    X, U = np.zeros((NB, NP, n)), np.zeros((NB, NP, m))
    for i in range(NB * NP):
        b, t = divmod(i, NP)
        for _ in range(1000):
            x, u = r32(dx(rng, n)), r32(du(rng, m))
            if i < len(special):
                for key, v in special[i].items():
                    (x if key[0] == "x" else u)[int(key[1:])] = r32(v)
            if all(d >= MARGIN for d in margin(x, u, par[b])):
                break
        else:
            raise AssertionError(f"{name}: no admissible point {i}")
        X[b, t], U[b, t] = x, u
    return X, U, par


# ---- references ---------------------------------------------------------------------------------------------------------------
def mp_reference(f, x, u, par, ops):
    mp = ops.mp
    n = len(x)
    z = [mp.mpf(float(v)) for v in list(x) + list(u)]
    p = [mp.mpf(float(v)) for v in par]
    h = mp.mpf(10) ** -20
    val = f(z[:n], z[n:], p, ops)
    J = np.zeros((n, len(z)))
    for j in range(len(z)):
        zp, zm = list(z), list(z)
        zp[j] += h
        zm[j] -= h
        fp, fm = f(zp[:n], zp[n:], p, ops), f(zm[:n], zm[n:], p, ops)
        J[:, j] = [float((a - b) / (2 * h)) for a, b in zip(fp, fm)]
    return np.array([float(v) for v in val]), J


def torch_baseline(f, x, u, par, dtype):
    import torch
    ops = TorchOps(dtype)
    n = len(x)
    p = [torch.tensor(float(v), dtype=dtype) for v in par]
    z = torch.tensor(np.concatenate([x, u]), dtype=dtype)

    def g(q):
        out = f([q[i] for i in range(n)], [q[n + i] for i in range(len(u))], p, ops)
        return torch.stack([o if isinstance(o, torch.Tensor) else torch.tensor(o, dtype=dtype) for o in out])

    with torch.no_grad():
        val = g(z).double().numpy()
    return val, torch.autograd.functional.jacobian(g, z).double().numpy()


def row_rel(err, ref):
    """largest |err| of each row over the largest |ref| of that row; a row whose reference is zero must have no error"""
    e, s = np.abs(err).max(-1), np.abs(ref).max(-1)
    assert (e[s == 0] == 0).all(), "an identically zero row is not reproduced exactly"
    return np.where(s > 0, e / np.where(s > 0, s, 1.0), 0.0)


def contract_arrays(table=None):
    import mpmath as mp
    import torch
    mp.mp.dps = 60
    ops = MpOps()
    out = {}
    for name in um.ZOO:
        n, m, _, f, _ = um.ZOO[name]
        X, U, par = points(name)
        val, J = np.zeros((NB, NP, n)), np.zeros((NB, NP, n, n + m))
        base = {torch.float64: np.zeros(n), torch.float32: np.zeros(n)}
        vbase = {torch.float64: 0.0, torch.float32: 0.0}
        for b in range(NB):
            for t in range(NP):
                val[b, t], J[b, t] = mp_reference(f, X[b, t], U[b, t], par[b], ops)
                for dt in base:
                    v, Jt = torch_baseline(f, X[b, t], U[b, t], par[b], dt)
                    base[dt] = np.maximum(base[dt], row_rel(Jt - J[b, t], J[b, t]))
                    vbase[dt] = max(vbase[dt], float(row_rel(v - val[b, t], val[b, t])))
        out.update({f"{name}_x": X, f"{name}_u": U, f"{name}_par": par, f"{name}_val": val, f"{name}_J": J,
                    f"{name}_base_f64": base[torch.float64], f"{name}_base_f32": base[torch.float32],
                    f"{name}_vbase_f64": np.float64(vbase[torch.float64]), f"{name}_vbase_f32": np.float64(vbase[torch.float32])})
        if table is not None:
            e64, e32 = np.finfo(np.float64).eps, np.finfo(np.float32).eps
            table.append(f"{name:5s} ({n},{m})  J fp64 " + " ".join(f"{v / e64:5.2f}" for v in base[torch.float64]) +
                         f" | val {vbase[torch.float64] / e64:5.2f}\n{'':12s} J fp32 " +
                         " ".join(f"{v / e32:5.2f}" for v in base[torch.float32]) + f" | val {vbase[torch.float32] / e32:5.2f}")
    return out


# ---- sin_cos ----------------------------------------------------------------------------------------------------------------------
SC_EDGE = np.array([0.0, -0.0, 1e-300, 1e5, -1e5])


def sin_cos_points():
    import mpmath as mp
    rng = np.random.default_rng(1414)
    with mp.workprec(200):
        mult = np.array([float(k * mp.pi / 2) for k in range(1, 2001)])          # the doubles nearest to k pi/2
    near = np.concatenate([mult, np.nextafter(mult, np.inf), np.nextafter(mult, -np.inf),
                           mult + rng.uniform(0, 1e-9, 2000), mult - rng.uniform(0, 1e-9, 2000)])
    rnd = np.concatenate([rng.uniform(-1e5, 1e5, 21000),
                          np.exp(rng.uniform(np.log(1e-8), np.log(1e5), 21000)) * rng.choice([-1.0, 1.0], 21000)])
    a = np.concatenate([rnd, near, -near, SC_EDGE])
    assert a.size == 62005 and (np.abs(a) <= 1e5).all()
    return a


def sin_cos_arrays():
    import mpmath as mp
    a = sin_cos_points()
    out = {k: np.zeros(a.size, dtype=np.float64 if k.endswith("hi") else np.float32) for k in ("s_hi", "s_lo", "c_hi", "c_lo")}
    with mp.workprec(200):
        for i, v in enumerate(a):
            for k, fn in (("s", mp.sin), ("c", mp.cos)):
                r = fn(mp.mpf(float(v)))
                hi = float(r)
                out[k + "_hi"][i], out[k + "_lo"][i] = hi, float(r - mp.mpf(hi))
    return {"pts": {"a": a}, "sin": {"hi": out["s_hi"], "lo": out["s_lo"]}, "cos": {"hi": out["c_hi"], "lo": out["c_lo"]}}


if __name__ == "__main__":
    table = []
    np.savez(os.path.join(HERE, "g14_ad_contract.npz"), **contract_arrays(table))
    for k, arrs in sin_cos_arrays().items():
        np.savez(os.path.join(HERE, f"g14_sin_cos_{k}.npz"), **arrs)
    print("same-precision CPU baseline (torch autograd against the 60-digit reference), per output row, in units of eps:")
    print("\n".join(table))
