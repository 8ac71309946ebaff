// riccati.hip -- the launcher of the Riccati gain pass (the kernel: riccati_gain_kernel.hpp; its REG forms: regularize.hip).
#include "riccati_gain_kernel.hpp"

namespace isls {

template <typename T>
int launch_gain(const isls_gain_args &a, hipStream_t s, const isls_ff_args *ff, bool *did_ff, bool require_ff, bool shared, int32_t *memo_hdr,
                void *memo_table)
{
    if (did_ff) *did_ff = false;
    if (const int rc = gain_args_check(a); rc != ISLS_OK) return rc;
    if (a.B == 0) return ISLS_OK;
    if (!dims_supported(a.n, a.m)) return require_ff ? ISLS_OK : launch_gain_generic<T>(a, s);   // generic.hip (no ff pass inside)
    GainP<T> p;
    gain_args_fill(a, p);
    // model-structured form (isls_gain_args.lin_on): on the record forms the drivers use; the caller switches it off by not
    // giving the hint (isls.Engine.use_model_structure, for the gain pass and its readers together)
    if (ff && !lin_hints_agree(a, *ff)) return ISLS_ERR_ARG;
    // lin_on also selects the LEAN record layout, which the feed-forward passes of the same hint read: no silent fall-back
    if (a.lin_on && (!a.rec || a.Quu || a.fac || a.Qux)) return ISLS_ERR_UNSUPPORTED;   // record form without the arrays only
    int lin = LIN_NONE;
    if (const int rc = lin_form(a.lin_on, a.lin_model, a.n, a.m, &lin); rc != ISLS_OK) return rc;
    if (lin == LIN_DI && !a.lin_par) return ISLS_ERR_ARG;
    p.lin_par = (const T *)a.lin_par; p.lin_par_sb = a.lin_par_sb;
    // shared records (gain_inputs_shared): the structured double-integrator form has them; the caller's readers rely on it
    if (shared && (lin != LIN_DI || !gain_inputs_shared(a) || !dims_supported(a.n, a.m))) return ISLS_ERR_ARG;
    if ((memo_hdr && !shared) || (memo_hdr != nullptr) != (memo_table != nullptr)) return ISLS_ERR_ARG;
    p.memo = memo_hdr; p.memo_table = (T *)memo_table;
    const bool with_ff = gain_ff_rides(a, ff);
    if (require_ff && !with_ff) return ISLS_OK;
    if (with_ff) gain_ff_fill(ff, p);
    // the arm and the car (LIN_ARM3R, LIN_CAR) run the dense arithmetic and write lean records
    const GainForm form = {with_ff, a.rec != nullptr, a.Qux != nullptr, lin == LIN_DI ? LIN_DI : LIN_NONE, lin != LIN_NONE, shared};
#define CALL(NX_, NU_)                                                                                      \
    {                                                                                                       \
        const int grid = (a.B + kWave / (NX_ + NU_) - 1) / (kWave / (NX_ + NU_));                           \
        if (a.solve_mode == ISLS_SOLVE_CHOL) launch_gain_form<T, NX_, NU_, ISLS_SOLVE_CHOL>(form, grid, s, p); \
        else launch_gain_form<T, NX_, NU_, ISLS_SOLVE_INV>(form, grid, s, p);                               \
    }
    ISLS_DISPATCH_DIMS(a.n, a.m, CALL)
#undef CALL
    if (did_ff) *did_ff = with_ff;
    return check_launch();
}
template int launch_gain<double>(const isls_gain_args &, hipStream_t, const isls_ff_args *, bool *, bool, bool, int32_t *, void *);
template int launch_gain<float>(const isls_gain_args &, hipStream_t, const isls_ff_args *, bool *, bool, bool, int32_t *, void *);

}  // namespace isls
