"""Per-trajectory Levenberg-Marquardt regularisation of the Riccati gain pass (include/isls_hip.h: isls_riccati_gain_reg_*,
isls_reg_update_*).  Pure Python: the settings object the solvers take as `regularization=`."""
import math


class Regularization:
    """mu_b >= 0 per trajectory, folded into the stage cost as mu/2 |du|^2 (`on='u'`) or mu/2 (|du|^2 + |dx|^2) (`on='xu'`): the
    gain pass runs on Cuu_t + mu_b I (and Cxx_t + mu_b I) for t <= N-2.  The schedule is iLQG.m's (Tassa, Erez, Todorov 2012):
    raise: delta = max(factor, delta factor), mu = max(mu_min, mu delta); lower: delta = min(1/factor, delta/factor),
    mu = mu delta if that is >= mu_min, else 0.  mu rises after a gain pass that met a Quu that is not positive definite (the pass
    is repeated) and after a rejected line search of `solve`; it falls after an accepted step.  A trajectory whose raise would
    pass mu_max stops with ISLS_ST_REG_MAX next to its failure bit; the others go on."""

    def __init__(self, mu_init=0.0, mu_min=1e-6, mu_max=1e10, factor=1.6, on='u'):
        vals = dict(mu_init=mu_init, mu_min=mu_min, mu_max=mu_max, factor=factor)
        for name, v in vals.items():
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"Regularization: {name} must be a finite number, got {v!r}")
        if mu_init < 0:
            raise ValueError("Regularization: mu_init >= 0")
        if not mu_min > 0:
            raise ValueError("Regularization: mu_min > 0")
        if not mu_max >= mu_min or mu_init > mu_max:
            raise ValueError("Regularization: mu_min <= mu_max and mu_init <= mu_max")
        if not factor > 1:
            raise ValueError("Regularization: factor > 1")
        if on not in ('u', 'xu'):
            raise ValueError("Regularization: on must be 'u' or 'xu'")
        self.mu_init, self.mu_min, self.mu_max, self.factor, self.on = float(mu_init), float(mu_min), float(mu_max), float(factor), on

    @property
    def on_x(self):
        return self.on == 'xu'

    def __repr__(self):
        return (f"Regularization(mu_init={self.mu_init}, mu_min={self.mu_min}, mu_max={self.mu_max}, factor={self.factor}, "
                f"on={self.on!r})")
