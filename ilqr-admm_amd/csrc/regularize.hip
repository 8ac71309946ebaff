// regularize.hip -- per-trajectory Levenberg-Marquardt regularisation of the Riccati gain pass (include/isls_hip.h:
// isls_riccati_gain_reg_*, isls_reg_update_*).  The REG instantiations of riccati_gain_kernel live in this object, next to the
// schedule kernel.
#include "riccati_gain_kernel.hpp"

namespace isls {

// The REG forms: dense arithmetic, a record per trajectory; records + K with or without the first feed-forward pass inside, or
// the arrays.
template <typename T>
int launch_gain_reg(const isls_gain_args &a, hipStream_t s, const isls_ff_args *ff, const isls_reg_args &reg)
{
    if (const int rc = gain_args_check(a); rc != ISLS_OK) return rc;
    if (!reg.mu) return ISLS_ERR_ARG;
    if (a.lin_on || (ff && ff->lin_on)) return ISLS_ERR_UNSUPPORTED;           // the model-structured forms carry no such term
    if (a.rec && a.Qux) return ISLS_ERR_UNSUPPORTED;                           // records + K, or the arrays
    if (a.B == 0) return ISLS_OK;
    if (!dims_supported(a.n, a.m)) return ff ? ISLS_ERR_UNSUPPORTED : launch_gain_generic<T>(a, s, &reg);
    const bool with_ff = gain_ff_rides(a, ff);
    if (ff && !with_ff) return ISLS_ERR_UNSUPPORTED;
    GainP<T> p;
    gain_args_fill(a, p);
    if (with_ff) gain_ff_fill(ff, p);
    p.reg_mu = (const T *)reg.mu; p.reg_on_x = reg.on_x != 0;
    const GainForm form = {with_ff, a.rec != nullptr, a.Qux != nullptr, LIN_NONE, false, false};
#define CALL(NX_, NU_)                                                                                      \
    {                                                                                                       \
        const int grid = (a.B + kWave / (NX_ + NU_) - 1) / (kWave / (NX_ + NU_));                           \
        if (a.solve_mode == ISLS_SOLVE_CHOL) launch_gain_form<T, NX_, NU_, ISLS_SOLVE_CHOL, true>(form, grid, s, p); \
        else launch_gain_form<T, NX_, NU_, ISLS_SOLVE_INV, true>(form, grid, s, p);                         \
    }
    ISLS_DISPATCH_DIMS(a.n, a.m, CALL)
#undef CALL
    return check_launch();
}
template int launch_gain_reg<double>(const isls_gain_args &, hipStream_t, const isls_ff_args *, const isls_reg_args &);
template int launch_gain_reg<float>(const isls_gain_args &, hipStream_t, const isls_ff_args *, const isls_reg_args &);

// ---- the schedule: one lane per trajectory -----------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void reg_update_kernel(int B, int mode, int32_t *status, const int32_t *active, T *mu, T *delta,
                                                         int32_t *retry, int32_t *count, T factor, T mu_min, T mu_max)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (mode == ISLS_REG_AFTER_GAIN && retry) retry[b] = 0;
    if (active && active[b] == 0) return;
    const int32_t st = status[b];
    if (st & ISLS_ST_REG_MAX) return;                          // the ladder ended earlier
    const int32_t fail = mode == ISLS_REG_AFTER_GAIN ? ISLS_ST_NOT_PD : ISLS_ST_LS_REJECT;
    if (st & fail) {
        const T d = fmax(factor, delta[b] * factor);
        const T v = fmax(mu_min, mu[b] * d);
        if (!(v <= mu_max)) { status[b] = st | ISLS_ST_REG_MAX; return; }
        delta[b] = d; mu[b] = v;
        if (mode == ISLS_REG_AFTER_GAIN) {
            status[b] = st & ~ISLS_ST_NOT_PD;
            if (retry) retry[b] = 1;
            if (count) atomicAdd(count, 1);
        }
    } else if (mode == ISLS_REG_AFTER_LS && !(st & ISLS_ST_NOT_PD)) {
        const T d = fmin(T(1) / factor, delta[b] / factor);
        const T v = mu[b] * d;
        delta[b] = d; mu[b] = v >= mu_min ? v : T(0);
    }
}

template <typename T>
int launch_reg_update(const isls_reg_update_args &a, hipStream_t s)
{
    if (a.B < 0 || !a.status || !a.mu || !a.delta) return ISLS_ERR_ARG;
    if (a.mode != ISLS_REG_AFTER_GAIN && a.mode != ISLS_REG_AFTER_LS) return ISLS_ERR_ARG;
    if (!(a.factor > 1.0) || !(a.mu_min > 0.0) || !(a.mu_max >= a.mu_min)) return ISLS_ERR_ARG;
    if (a.B == 0) return ISLS_OK;
    hipLaunchKernelGGL((reg_update_kernel<T>), dim3((a.B + 255) / 256), dim3(256), 0, s, (int)a.B, (int)a.mode, a.status, a.active,
                       (T *)a.mu, (T *)a.delta, a.retry, a.count, (T)a.factor, (T)a.mu_min, (T)a.mu_max);
    return check_launch();
}
template int launch_reg_update<double>(const isls_reg_update_args &, hipStream_t);
template int launch_reg_update<float>(const isls_reg_update_args &, hipStream_t);

}  // namespace isls
