// user_grad.hip -- the parameter and table directions of the nominal's cost for user-written models and costs: the launches of
// user_model_grad_kernel / user_cost_grad_kernel (the device side is user_grad.hpp) and the isls_user_*_grad_* entry points.  The
// program of a source's gradient is built and kept by user_rtc.hip, apart from the source's other programs.
#include "entry.hpp"
#include "user_grad.hpp"
#include "user_rtc.hpp"

namespace isls {

template <typename T>
static int launch_user_grad(urtc::Kind kind, const isls_user_grad_args &a, hipStream_t s)
{
    const bool model = kind == urtc::KIND_MODEL;
    if (a.B < 0 || a.N < 1 || !a.par || a.par_sb < 0 || a.tab_sb < 0 || !a.xhat || !a.uhat || (model && !a.lam)) return ISLS_ERR_ARG;
    if (model ? !is_user_model(a.id) : !is_user_cost(a.id)) return ISLS_ERR_ARG;
    int P, W, NTAB;
    int rc = urtc::grad_prepare(kind, a.id, urtc::dtype_of<T>(), a.n, a.m, s, nullptr, &P, &W, &NTAB);
    if (rc != ISLS_OK) return rc;
    // the table as every other launch of the source takes it
    rc = model ? urtc::check_model_table(a.id, a.N, a.par, a.par_sb) : urtc::check_table(a.id, a.N, a.tab, a.tab_sb, -1);
    if (rc != ISLS_OK) return rc;
    const bool want_par = a.g_par != nullptr && P > 0, want_tab = a.g_tab != nullptr && W > 0;
    if (a.B == 0 || (!want_par && !want_tab)) return ISLS_OK;
    hipFunction_t fn;
    if ((rc = urtc::grad_prepare(kind, a.id, urtc::dtype_of<T>(), a.n, a.m, s, &fn, &P, &W, &NTAB)) != ISLS_OK) return rc;
    UserGradP<T> p;
    p.B = a.B; p.N = a.N;
    p.d0 = want_par ? 0 : P;
    p.nd = (want_par ? P : 0) + (want_tab ? W : 0);
    p.par = (const T *)a.par; p.par_sb = a.par_sb;
    p.tab = (const T *)a.tab; p.tab_sb = a.tab_sb;
    p.xhat = (const T *)a.xhat; p.uhat = (const T *)a.uhat; p.lam = (const T *)a.lam;
    p.g_par = (T *)a.g_par; p.g_tab = (T *)a.g_tab; p.active = a.active;
    const int64_t grid = (int64_t)a.B * p.nd;
    if (grid > 0x7fffffff) return ISLS_ERR_UNSUPPORTED;
    void *args[] = {&p};
    return urtc::launch(fn, (int)grid, 0, s, args);
}

}  // namespace isls

using namespace isls;

ISLS_API int isls_user_model_grad_build(int32_t id, int32_t dtype)
{
    return is_user_model(id) ? urtc::grad_build(urtc::KIND_MODEL, id, dtype) : ISLS_ERR_ARG;
}
ISLS_API int isls_user_cost_grad_build(int32_t id, int32_t dtype)
{
    return is_user_cost(id) ? urtc::grad_build(urtc::KIND_COST, id, dtype) : ISLS_ERR_ARG;
}
ISLS_TYPED_PAIR(user_model_grad, (const isls_user_grad_args *a, void *stream),
                return a ? launch_user_grad<T>(urtc::KIND_MODEL, *a, (hipStream_t)stream) : ISLS_ERR_ARG;)
ISLS_TYPED_PAIR(user_cost_grad, (const isls_user_grad_args *a, void *stream),
                return a ? launch_user_grad<T>(urtc::KIND_COST, *a, (hipStream_t)stream) : ISLS_ERR_ARG;)
