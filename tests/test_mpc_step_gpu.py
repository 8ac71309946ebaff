"""GPU tests of the receding-horizon control step (isls_mpc_step_*, csrc/mpc.hpp) through Kernels.mpc_step against the numpy
restatement tests/mpc_reference.py.  Everything that is a copy -- the moved K, zx, zu, table and x_meas_out -- compares with ==
(an in-place shift that overwrites a row before reading it fails there); x_next_out, u_out and the re-rolled xhat / uhat take the
bounds of tests/test_monte_carlo_gpu.py for the same arithmetic chain (K dx + uhat, then a model step): rel < 1e-10 in fp64,
< 1e-4 in fp32, rel = max-abs error over max(1, |ref|_max).  Every array holds values distinct per (b, t, component) and lies
between guard words that must stay as they are."""
import numpy as np
import pytest
import torch

import user_models as um
from isls import _capi as capi
from isls import models
from mpc_reference import model_f, mpc_step

pytestmark = pytest.mark.gpu
GUARD = 64
TOL = {torch.float64: 1e-10, torch.float32: 1e-4}
# 1: a single trajectory; 3, 4, 5: around the four slots of a wavefront; 65: one more than a wavefront of lanes; 130: several
# workgroups with a partial last one
BS, NS = (1, 3, 4, 5, 65, 130), (1, 2, 3, 17)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


def di_model(p):
    eye, zero = np.eye(3), np.zeros((3, 3))
    return models.LTI(np.block([[eye, p[0] * eye], [zero, eye]]), np.vstack([p[1] * eye, p[2] * eye]))


def lti52_model(p):
    return models.LTI(p[:25].reshape(5, 5), p[25:].reshape(5, 2))


def quad_f(x, u, par):
    par = np.broadcast_to(par, (x.shape[0], par.shape[-1]))
    return np.stack([um.quad_numpy(par[b])[0](x[b], u[b]) for b in range(x.shape[0])])


def setup(name, rng):
    """(model id, n, m, f, base parameter row, relative spread of the plant's rows)"""
    if name == "di":
        return capi.MODEL_DI, 6, 3, model_f(di_model), np.array([0.05, 0.00125, 0.05]), 0.2
    if name == "car":
        return capi.MODEL_CAR, 4, 2, model_f(lambda p: models.CarSimple(p[0])), np.array([0.05]), 0.2
    if name == "arm":
        return capi.MODEL_ARM3R, 9, 3, model_f(lambda p: models.Planar3R(p[0])), np.array([0.01]), 0.2
    if name == "lti52":
        A, B = np.eye(5) + 0.1 * rng.standard_normal((5, 5)), 0.3 * rng.standard_normal((5, 2))
        return capi.MODEL_LTI, 5, 2, model_f(lti52_model), np.concatenate([A.ravel(), B.ravel()]), 0.05
    quad = models.Custom(6, 2, um.QUAD_PAR, um.QUAD)
    return quad.model_id, 6, 2, quad_f, um.QUAD_PAR.copy(), 0.1


class Dev:
    """host arrays on the device between guard words"""

    def __init__(self, dtype):
        self.dtype, self.dev, self.kept = dtype, torch.device("cuda:0"), []

    def __call__(self, a):
        if a is None:
            return None
        a = np.asarray(a)
        flat = torch.full((a.size + 2 * GUARD,), -777.0, dtype=self.dtype, device=self.dev)
        view = flat[GUARD:GUARD + a.size].view(*a.shape)
        view.copy_(torch.as_tensor(a, dtype=self.dtype))
        self.kept.append(flat)
        return view

    def guards_intact(self):
        return all(bool((f[:GUARD] == -777.0).all()) and bool((f[-GUARD:] == -777.0).all()) for f in self.kept)


def distinct(rng, shape, scale):
    """values distinct per element: a random part plus a ramp over the flat index"""
    size = int(np.prod(shape))
    return (scale * rng.standard_normal(size) + 1e-3 * scale * np.arange(size)).reshape(shape)


# every option of the step appears in these for every model and precision (they cycle over the (B, N) grid)
CONFIGS = [
    dict(K=True, z=True, tab="shared", W=16, nxt=True, clip=True, noise="w", plant=False, outs=True),
    dict(K=False, z=False, tab=None, W=0, nxt=False, clip=False, noise=None, plant=True, outs=True),
    dict(K=True, z=False, tab="per", W=1, nxt=True, clip=False, noise="philox", plant=True, outs=False),
    dict(K=True, z=True, tab="per", W=16, nxt=False, clip=True, noise="philox", plant=False, outs=True),
    dict(K=False, z=True, tab="shared", W=1, nxt=False, clip=True, noise="w", plant=True, outs=True),
    dict(K=True, z=True, tab=None, W=0, nxt=False, clip=False, noise=None, plant=False, outs=True),
    dict(K=True, z=False, tab="shared", W=16, nxt=True, clip=True, noise=None, plant=True, outs=True),
]


def make_case(name, rng, B, N, cfg):
    model, n, m, f, par0, spread = setup(name, rng)
    c = dict(model=model, n=n, m=m, f=f, B=B, N=N)
    c["par"] = par0
    c["plant_par"] = par0 * (1 + spread * rng.uniform(-1, 1, size=(B, par0.size))) if cfg["plant"] else None
    sx = 0.3
    c["xhat"], c["uhat"] = distinct(rng, (B, N, n), sx), distinct(rng, (B, N, m), sx)
    if name == "quad":
        c["uhat"] += 4.9                                        # about hover
    c["K"] = distinct(rng, (B, N, m, n), 0.05)                 # always there: not passed, it must stay as it is
    c["zx"], c["zu"] = distinct(rng, (B, N, n), 1.0), distinct(rng, (B, N, m), 1.0)
    W = cfg["W"]
    c["tab"] = None if cfg["tab"] is None else distinct(rng, ((N, W) if cfg["tab"] == "shared" else (B, N, W)), 1.0)
    c["tab_next"] = (distinct(rng, ((W,) if cfg["tab"] == "shared" else (B, W)), 1.0) + 50.0) if cfg["nxt"] else None
    lo, hi = np.quantile(c["uhat"][:, 0], 0.3, axis=0), np.quantile(c["uhat"][:, 0], 0.7, axis=0)
    c["u_lo"], c["u_hi"] = (lo, np.maximum(hi, lo)) if cfg["clip"] else (None, None)
    c["w"] = distinct(rng, (B, n), 0.01) if cfg["noise"] == "w" else None
    c["noise_std"] = 0.01 * (1 + np.arange(n)) if cfg["noise"] == "philox" else None
    return c


def launch(c, cfg, dtype, seed=5, problem0=0, step=3, rows=None):
    """run the step on the device; returns the device-side arrays after the launch (numpy) and the guard check"""
    d = Dev(dtype)
    sl = slice(None) if rows is None else rows
    cut = lambda a, per=True: None if a is None else (a[sl] if per else a)    # noqa: E731
    per_tab = cfg["tab"] == "per"
    t = {k: d(cut(c[k])) for k in ("xhat", "uhat", "K", "zx", "zu")}
    t["tab"], t["tab_next"] = d(cut(c["tab"], per_tab)), d(cut(c["tab_next"], per_tab))
    par, plant = d(c["par"]), d(cut(c["plant_par"]))
    Bl, n, m = t["xhat"].shape[0], c["n"], c["m"]
    outs = {k: d(np.full((Bl, w_), -5.0)) for k, w_ in (("x_meas_out", n), ("u_out", m), ("x_next_out", n))} if cfg["outs"] else {}
    capi.Kernels(capi.library()).mpc_step(
        c["model"], par, t["xhat"], t["uhat"], K=t["K"] if cfg["K"] else None, zx=t["zx"] if cfg["z"] else None,
        zu=t["zu"] if cfg["z"] else None, plant_par=plant, tab=t["tab"], tab_next=t["tab_next"], u_lo=d(c["u_lo"]), u_hi=d(c["u_hi"]),
        w=d(cut(c["w"])), noise_std=d(c["noise_std"]), seed=seed, problem0=problem0, step=step,
        stream=torch.cuda.current_stream().cuda_stream, **outs)
    torch.cuda.synchronize()
    got = {k: None if v is None else v.cpu().numpy() for k, v in {**t, **outs}.items()}
    return got, d.guards_intact()


def rounded(c, dtype):
    """the case as the device holds it: every input rounded to the entry point's precision"""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    return {k: (v.astype(npdt).astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def check(c, cfg, dtype, got, seed=5, problem0=0, step=3):
    npdt = np.float32 if dtype == torch.float32 else np.float64
    r = rounded(c, dtype)
    ref = mpc_step(r["f"], r["par"], r["xhat"], r["uhat"], K=r["K"] if cfg["K"] else None, zx=r["zx"] if cfg["z"] else None,
                   zu=r["zu"] if cfg["z"] else None, plant_par=r["plant_par"], tab=r["tab"], tab_next=r["tab_next"], u_lo=r["u_lo"],
                   u_hi=r["u_hi"], w=r["w"], noise_std=r["noise_std"], seed=seed, problem0=problem0, step=step, dtype=npdt)
    # ---- copies: exact; arrays that were not passed: as they were --------------------------------------------------------------
    assert np.array_equal(got["K"], ref["K"] if cfg["K"] else r["K"]), "K"
    assert np.array_equal(got["zx"], ref["zx"] if cfg["z"] else r["zx"]), "zx"
    assert np.array_equal(got["zu"], ref["zu"] if cfg["z"] else r["zu"]), "zu"
    if cfg["tab"] is not None:
        assert np.array_equal(got["tab"], ref["tab"]), "table"
    if cfg["nxt"]:
        assert np.array_equal(got["tab_next"], r["tab_next"])
    tol = TOL[dtype]
    if cfg["outs"]:
        assert np.array_equal(got["x_meas_out"], ref["x_meas"]), "x_meas_out"
        if cfg["clip"]:
            assert np.all(got["u_out"] >= r["u_lo"]) and np.all(got["u_out"] <= r["u_hi"])
            assert np.any(got["u_out"] != r["uhat"][:, 0]) or c["B"] < 3              # the bounds bite
        ex, eu = rel(got["x_next_out"], ref["x_next"]), rel(got["u_out"], ref["u_app"])
        assert ex < tol and eu < tol, ("x_next / u_out", ex, eu)
        assert np.array_equal(got["xhat"][:, 0], got["x_next_out"])                   # the plan starts at the measurement
    ex, eu = rel(got["xhat"], ref["xhat"]), rel(got["uhat"], ref["uhat"])
    assert ex < tol and eu < tol, ("re-rolled plan", ex, eu)
    if not cfg["K"]:                                           # open loop: the moved controls, exactly
        assert np.array_equal(got["uhat"], np.concatenate([r["uhat"][:, 1:], r["uhat"][:, -1:]], axis=1))
    return max(ex, eu)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["di", "car", "arm", "lti52", "quad"])
def test_step_against_numpy(name, dtype):
    rng = np.random.default_rng(17)
    worst, i = 0.0, 0
    for N in NS:
        for B in BS:
            cfg = CONFIGS[i % len(CONFIGS)]
            i += 1
            c = make_case(name, rng, B, N, cfg)
            got, guards = launch(c, cfg, dtype)
            assert guards, (B, N, cfg)
            try:
                worst = max(worst, check(c, cfg, dtype, got))
            except AssertionError as e:
                raise AssertionError(f"{name} B={B} N={N} cfg={cfg}: {e}") from e
    print(f"{name} {dtype}: worst rel err of the re-rolled plan {worst:.2e}")


@pytest.mark.parametrize("name", ["di", "car"])
def test_every_option_at_one_shape(name):
    """every configuration at the shape with several workgroups and a partial last one, N no multiple of the ring depth"""
    rng = np.random.default_rng(3)
    for cfg in CONFIGS:
        c = make_case(name, rng, 130, 17, cfg)
        got, guards = launch(c, cfg, torch.float64)
        assert guards
        check(c, cfg, torch.float64, got)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_chunk_invariance_and_counters(dtype):
    """B = 130 in one launch == two launches of 65 with problem0 = 0 and 65, bit for bit; another step or seed: other draws"""
    rng = np.random.default_rng(9)
    cfg = dict(K=True, z=True, tab="per", W=16, nxt=True, clip=True, noise="philox", plant=True, outs=True)
    c = make_case("car", rng, 130, 17, cfg)
    full, g0 = launch(c, cfg, dtype)
    a, g1 = launch(c, cfg, dtype, problem0=0, rows=slice(0, 65))
    b, g2 = launch(c, cfg, dtype, problem0=65, rows=slice(65, 130))
    assert g0 and g1 and g2
    for k, v in full.items():
        if v is not None and v.shape[:1] == (130,):
            assert np.array_equal(v, np.concatenate([a[k], b[k]])), k
    check(c, cfg, dtype, full)
    other_step, _ = launch(c, cfg, dtype, step=4)
    other_seed, _ = launch(c, cfg, dtype, seed=6)
    assert np.array_equal(other_step["x_meas_out"], full["x_meas_out"]) and np.array_equal(other_step["u_out"], full["u_out"])
    assert not np.array_equal(other_step["x_next_out"], full["x_next_out"])
    assert not np.array_equal(other_seed["x_next_out"], full["x_next_out"])
    wrong, _ = launch(c, cfg, dtype, problem0=1, rows=slice(65, 130))
    assert not np.array_equal(wrong["x_next_out"], b["x_next_out"])


def test_outputs_into_log_columns():
    """the outputs with a batch stride of their own: column s of [B, T, .] logs, the other columns as they were"""
    rng = np.random.default_rng(2)
    cfg = CONFIGS[0]
    c = make_case("di", rng, 5, 3, cfg)
    plain, _ = launch(c, cfg, torch.float64)
    d = Dev(torch.float64)
    t = {k: d(c[k]) for k in ("xhat", "uhat", "K", "zx", "zu", "tab", "tab_next", "u_lo", "u_hi", "w", "par")}
    T_, s = 4, 2
    xl, ul = d(np.full((5, T_ + 1, 6), -3.0)), d(np.full((5, T_, 3), -3.0))
    capi.Kernels(capi.library()).mpc_step(c["model"], t["par"], t["xhat"], t["uhat"], K=t["K"], zx=t["zx"], zu=t["zu"], tab=t["tab"],
                                          tab_next=t["tab_next"], u_lo=t["u_lo"], u_hi=t["u_hi"], w=t["w"], seed=5, step=3,
                                          x_meas_out=xl[:, s], u_out=ul[:, s], x_next_out=xl[:, s + 1],
                                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    xl, ul = xl.cpu().numpy(), ul.cpu().numpy()
    assert d.guards_intact()
    assert np.array_equal(xl[:, s], plain["x_meas_out"]) and np.array_equal(xl[:, s + 1], plain["x_next_out"])
    assert np.array_equal(ul[:, s], plain["u_out"])
    keep = [i for i in range(T_ + 1) if i not in (s, s + 1)]
    assert np.all(xl[:, keep] == -3.0) and np.all(ul[:, [i for i in range(T_) if i != s]] == -3.0)


def test_unsupported_model_and_dimensions():
    d = Dev(torch.float64)
    x, u, par = d(np.zeros((2, 3, 5))), d(np.zeros((2, 3, 2))), d(np.zeros(1))
    with pytest.raises(capi.IslsError, match="unsupported"):    # the car has no kernel at (5, 2)
        capi.Kernels(capi.library()).mpc_step(capi.MODEL_CAR, par, x, u, stream=torch.cuda.current_stream().cuda_stream)
