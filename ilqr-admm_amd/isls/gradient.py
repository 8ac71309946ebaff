"""Gradients of the nominal's cost by an adjoint sweep on the device (iSLS.gradient).

J = sum_t c_t(x_t, u_t) along the nominal, x_0 given, x_{t+1} = f(x_t, u_t, row_t): what `q.cost` reports.  The sweep
(isls_adjoint_sweep_*, csrc/adjoint.hip) runs the costate recursion on the A_t, B_t of a linearisation and the c0x, c0u of an
expansion about the nominal; the parameter and table directions of a models.Custom / costs.Custom come from the source's gradient
program (isls_user_*_grad_*, csrc/user_grad.hpp), compiled on the first request.
"""
import torch

from . import _capi as capi
from .engine import LINEARIZED, STATIC

WRT = ("u", "x0", "cost_params", "model_params", "cost_table", "model_table")


class Gradient:
    """What iSLS.gradient returns.  cost [B], costate [B, N, n] always; u [B, N, m], x0 [B, n], cost_params [B, Pc], model_params
    [B, Pm], cost_table [B, N, Wc], model_table [B, N, Wm] where asked for, else None."""

    def __init__(self):
        self.cost = self.costate = None
        for name in WRT:
            setattr(self, name, None)


def _check(q, wrt):
    """The refusals, ahead of any launch: returns (model object or None, cost object or None) for the directions asked for"""
    from .costs import Custom as CustomCost
    from .models import Custom as CustomModel
    unknown = [w for w in wrt if w not in WRT]
    if unknown:
        raise capi.IslsError(f"gradient: unknown wrt {unknown}; known: {WRT}")
    if q._host_model or q.engine.model is None:
        raise capi.IslsError("gradient needs a device forward model (an isls.models descriptor, models.Custom for one of your own): "
                             "a Python callable has no linearisation the adjoint sweep could read")
    if q._host_cost:
        raise capi.IslsError("gradient needs a device cost (the via-point cost, an isls.costs object, costs.Custom for one of your "
                             "own): a Python callable has no gradient on the device")
    model, cost = q._forward_model, q._cost_function
    if "model_params" in wrt or "model_table" in wrt:
        if not isinstance(model, CustomModel):
            raise capi.IslsError("gradient: model_params / model_table need a models.Custom forward model (a built-in model's "
                                 "parameters have no gradient program)")
        if "model_params" in wrt and model.params().shape[-1] == 0:
            raise capi.IslsError("gradient: model_params of a models.Custom without parameters")
        if "model_table" in wrt and model.table is None:
            raise capi.IslsError("gradient: model_table needs a models.Custom(table=): this model has no table")
    if "cost_params" in wrt or "cost_table" in wrt:
        if not isinstance(cost, CustomCost):
            raise capi.IslsError("gradient: cost_params / cost_table need a costs.Custom cost_function (the built-in costs' "
                                 "parameters have no gradient program)")
        if "cost_params" in wrt and cost.params().shape[-1] == 0:
            raise capi.IslsError("gradient: cost_params of a costs.Custom without parameters")
        if "cost_table" in wrt and cost.table is None:
            raise capi.IslsError("gradient: cost_table needs a costs.Custom(table=): this cost has no table")
    return model, cost


def gradient(q, wrt=("u", "x0"), as_tensors=False):
    """See iSLS.gradient."""
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    model, cost = _check(q, wrt)
    e = q.engine
    # the gradient programs first: a source outside the contract raises here, with its log, before anything runs
    if "model_params" in wrt or "model_table" in wrt:
        capi.user_model_grad_build(model.model_id, e.dtype)
    if "cost_params" in wrt or "cost_table" in wrt:
        capi.user_cost_grad_build(cost.cost_model, e.dtype)
    q._sync_tables()
    B, N, n, m = e.B, e.N, e.n, e.m
    stream = torch.cuda.current_stream().cuda_stream
    z = lambda *s: torch.zeros(*s, dtype=e.dtype, device=e.device)   # noqa: E731
    # A_t, B_t about the nominal for EVERY trajectory (a solver's own linearisation skips the ones that stopped); a caller's pair
    # (the AB setter: a shared LTI pair, a get_AB's) is taken as it stands
    if not q._user_AB:
        static = e.model in (capi.MODEL_DI, capi.MODEL_LTI)
        e.kern.linearize(e.model, e.model_par, e.xhat, e.uhat, e.A, e.Bm, stream=stream)
        e._ab_src = STATIC if static else LINEARIZED
    # c0x, c0u and the cost about the nominal: no Hessians, no ADMM weights (Qr, Rr are not part of J)
    g = Gradient()
    g.cost = z(B)
    if e.Qtab is None:
        raise capi.IslsError("gradient: set the cost and the nominal first (set_cost_variables / cost_function, nominal_values)")
    blk = capi.Kernels.expand_args(e.Qtab, e.ztab, e.seq, e.u_std, e.c0x, e.c0u, xhat=e.xhat, uhat=e.uhat, cost=g.cost,
                                   cost_model=e.cost_model, cost_par=e.cost_par, q_nonzero=e.q_nonzero, cost_tab=e.cost_tab)
    if e.user_cost:
        e.kern.user_cost_expand(blk, None, e.sfx, stream=stream)
    else:
        e.kern._call("expand_quadratic", e.sfx, blk, stream)
    g.costate, gu, gx0 = z(B, N, n), z(B, N, m), z(B, n)
    e.kern.adjoint_sweep(e.A, e.Bm, e.c0x, e.c0u, g.costate, gu, gx0, stream=stream)
    if "u" in wrt:
        g.u = gu
    if "x0" in wrt:
        g.x0 = gx0
    if "model_params" in wrt or "model_table" in wrt:
        W = e.model_tab_w
        P = e.model_par.shape[-1] - N * W
        g.model_params = z(B, P) if "model_params" in wrt else None
        g.model_table = z(B, N, W) if "model_table" in wrt else None
        e.kern.user_grad("model", e.model, e.model_par, e.xhat, e.uhat, lam=g.costate, g_par=g.model_params, g_tab=g.model_table,
                         stream=stream)
    if "cost_params" in wrt or "cost_table" in wrt:
        g.cost_params = z(B, e.cost_par.shape[-1]) if "cost_params" in wrt else None
        g.cost_table = z(B, N, cost.n_tab) if "cost_table" in wrt else None   # (a cost with constraints: the user's columns only)
        e.kern.user_grad("cost", e.cost_model, e.cost_par, e.xhat, e.uhat, tab=e.cost_tab, g_par=g.cost_params,
                         g_tab=g.cost_table, stream=stream)
    if not as_tensors:
        for name in ("cost", "costate") + WRT:
            v = getattr(g, name)
            if v is not None:
                setattr(g, name, v.cpu().numpy())
    return g
