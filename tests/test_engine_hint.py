"""Who wrote A, Bm decides the model hint (isls_gain_args.lin_on / isls_ff_args.lin_on) of the outer driver: `Engine._ab_src`
walked through its transitions on a small double integrator, with the hint fields of the driver's block read after each
event.  The hint rides on the sequential feed-forward passes only, which a batch this small gets from ISLS_FF_NSEG=1."""
import numpy as np
import pytest

import isls_problems as P

pytestmark = pytest.mark.gpu
B, N, J, L = 48, 100, 3, 10


def hint(eng):
    a = eng._outer_args
    return int(a.gain.lin_on), int(a.ff.lin_on)


def step(eng):
    eng.run_outer()
    h = hint(eng)
    eng.advance()
    return h


def test_model_hint_follows_who_wrote_A_B(monkeypatch):
    import torch
    from isls import _capi as capi
    from isls import engine as E
    from isls import models
    monkeypatch.setenv("ISLS_FF_NSEG", "1")
    cfg = P.config2(batch=B, N=N, seed=0)
    mdl = models.LTI(cfg["A"], cfg["B"])
    eng = E.Engine(B, N, cfg["n"], cfg["m"], dtype=torch.float64, device="cuda")
    eng.set_model(mdl.model_id, mdl.params())
    assert eng.model == capi.MODEL_DI and eng._ab_src is None
    eng.set_quadratic_cost(cfg["zs"], cfg["Qs"], cfg["seq"], cfg["u_std"])
    eng.set_nominal(np.repeat(cfg["x0"][:, None, :], N, axis=1), cfg["u0"])
    eng.set_admm(rho_u=cfg["rho_u"], u_box=(cfg["u_lo"], cfg["u_hi"]), relax=cfg["relax"])
    build = lambda: eng.build_outer(L, J, begin_done=True)   # noqa: E731

    # build_outer before linearize (bench.py's order): no hint in the block, it appears at run_outer
    build()
    assert eng._outer_seg is None and hint(eng) == (0, 0)
    eng.linearize()
    eng.expand()
    eng.begin_outer()
    assert eng._ab_src == E.STATIC
    assert step(eng) == (1, 1) and step(eng) == (1, 1)      # advance() leaves the static linearisation in place

    # ab_from_caller: the cached block keeps its hint until run_outer rewrites it
    eng.ab_from_caller()
    assert eng._ab_src == E.CALLER and hint(eng) == (1, 1)
    assert step(eng) == (0, 0)
    # ... advance() linearises again (the pair is not the model's static one any more)
    assert eng._ab_src == E.LINEARIZED and step(eng) == (1, 1)

    # assignment of A: the cached blocks go, run_outer refuses to launch on them
    old = eng.A                                             # kept alive: the old block would read live memory, not freed memory
    eng.A = old.clone()
    assert eng._ab_src is None and eng._outer_args is None
    with pytest.raises(capi.IslsError):
        eng.run_outer()
    build()
    assert hint(eng) == (0, 0) and step(eng) == (0, 0)      # no hint until the next linearize ...
    assert eng._ab_src == E.LINEARIZED and step(eng) == (1, 1)   # ... here the one advance() makes
    eng.linearize()
    assert eng._ab_src == E.STATIC and step(eng) == (1, 1)

    # set_model: no hint until the next linearize
    eng.set_model(mdl.model_id, mdl.params())
    assert eng._ab_src is None and eng._outer_args is None
    build()
    assert hint(eng) == (0, 0) and step(eng) == (0, 0)
    eng.linearize()
    assert eng._ab_src == E.STATIC and step(eng) == (1, 1)

    # a caller's A, B stay a caller's through set_model and an assignment of A
    eng.ab_from_caller()
    eng.set_model(mdl.model_id, mdl.params())
    assert eng._ab_src == E.CALLER
    eng.Bm = eng.Bm.clone()
    assert eng._ab_src == E.CALLER
    build()
    assert hint(eng) == (0, 0) and step(eng) == (0, 0)
    eng.linearize()
    assert eng._ab_src == E.STATIC and step(eng) == (1, 1)
    torch.cuda.synchronize()
    assert not (eng.status.cpu().numpy() & capi.ST_NOT_PD).any()
