// user_cost.hip -- user-written cost functions: the launches of a cost's own kernels -- expansion, value and, for a cost with
// constraints, the multiplier update (the device side is user_cost.hpp) -- and the isls_user_cost_* entry points.  Registry,
// run-time compilation, module loading and the line search are user_rtc.hip's: the programs of a cost are the keys (model or
// none, cost) there, and every one of them holds these kernels.
#include "entry.hpp"
#include "user_rtc.hpp"

namespace isls {

// the kernels of cost `id` for a launch of dims (n, m): whichever of its programs is on the device
template <typename T>
static int prepare(int id, int n, int m, hipStream_t s, urtc::Kernels *k)
{
    return urtc::prepare(urtc::kNone, id, urtc::dtype_of<T>(), n, m, s, k);
}

template <typename T>
static int user_cost_value(int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *tab, int64_t tab_sb,
                           const void *x, const void *u, void *cost, const int32_t *active, hipStream_t s)
{
    if (R < 0 || N < 1 || !par || !cost || par_sb < 0) return ISLS_ERR_ARG;
    int n, m;
    int rc = urtc::dims(urtc::KIND_COST, id, &n, &m);
    if (rc == ISLS_OK) rc = urtc::check_table(id, N, tab, tab_sb, -1);   // (a cost with a table through the entry without one: NULL)
    if (rc != ISLS_OK || R == 0) return rc;
    urtc::Kernels k;
    if ((rc = prepare<T>(id, n, m, s, &k)) != ISLS_OK) return rc;
    int R_ = R, N_ = N;
    const T *par_ = (const T *)par, *x_ = (const T *)x, *u_ = (const T *)u, *tab_ = (const T *)tab;
    T *cost_ = (T *)cost;
    void *args[] = {&R_, &N_, &par_, &par_sb, &x_, &u_, &cost_, &active, &tab_, &tab_sb};
    return urtc::launch(k.of(urtc::ROLE_VAL), (R + 63) / 64, 0, s, args);
}

// ---- launches (dispatched from misc.hip on a.cost_model >= ISLS_COST_USER_BASE) ----------------------------------------------
template <typename T>
int launch_expand_user_cost(const isls_expand_args &a, void *Cux, hipStream_t s)
{
    if (a.B < 0 || a.N < 1 || !a.c0x || !a.c0u || !a.cost_par || a.cost_par_sb < 0) return ISLS_ERR_ARG;
    if (a.B == 0) return ISLS_OK;
    int rc = urtc::check_table(a.cost_model, a.N, a.ztab, a.ztab_sb, a.nvia);   // the table: ztab, ztab_sb, nvia (isls_hip.h)
    if (rc != ISLS_OK) return rc;
    urtc::Kernels k;
    if ((rc = prepare<T>(a.cost_model, a.n, a.m, s, &k)) != ISLS_OK) return rc;
    const int K = a.n + a.m, NP = K * (K + 1) / 2, steps = NP <= kWave ? kWave / NP : 4;   // user_expand_kernel's S
    UserExpP<T> p;
    p.B = a.B; p.N = a.N; p.nbt = (a.N + steps - 1) / steps;
    p.par = (const T *)a.cost_par; p.par_sb = a.cost_par_sb;
    p.xhat = (const T *)a.xhat; p.uhat = (const T *)a.uhat;
    p.Qr = View<T>(a.Qr); p.Rr = View<T>(a.Rr);
    p.Cxx = (T *)a.Cxx; p.Cuu = (T *)a.Cuu; p.Cux = (T *)Cux; p.c0x = (T *)a.c0x; p.c0u = (T *)a.c0u;
    p.active = a.active;
    p.tab = (const T *)a.ztab; p.tab_sb = a.ztab_sb;          // read by a cost with a table only
    const int64_t grid = (int64_t)a.B * p.nbt;
    if (grid > 0x7fffffff) return ISLS_ERR_UNSUPPORTED;
    void *args[] = {&p};
    if ((rc = urtc::launch(k.of(urtc::ROLE_EXP), (int)grid, 0, s, args)) != ISLS_OK || !a.cost) return rc;
    return user_cost_value<T>(a.cost_model, a.B, a.N, a.cost_par, a.cost_par_sb, a.ztab, a.ztab_sb, a.xhat, a.uhat, a.cost, a.active, s);
}
template int launch_expand_user_cost<double>(const isls_expand_args &, void *, hipStream_t);
template int launch_expand_user_cost<float>(const isls_expand_args &, void *, hipStream_t);


// ---- the multiplier and penalty update of a cost with constraints (user_constraint_update_kernel, user_cost.hpp) ----------------
template <typename T>
static int launch_constraint_update(const isls_constraint_update_args &a, hipStream_t s)
{
    if (a.B < 0 || a.N < 1 || !a.cost_par || a.cost_par_sb < 0 || !a.tab || !a.xhat || !a.uhat || !a.viol || !a.viol_prev)
        return ISLS_ERR_ARG;
    int n, m;
    int rc = urtc::dims(urtc::KIND_COST, a.cost_model, &n, &m);
    if (rc != ISLS_OK || n != a.n || m != a.m || urtc::n_con(a.cost_model) <= 0) return ISLS_ERR_ARG;
    // the multipliers are state of a trajectory: one table each
    if (a.tab_sb != (int64_t)a.N * urtc::n_tab(a.cost_model) && a.B > 1) return ISLS_ERR_ARG;
    if (a.update && !(a.phi >= 1.0 && a.mu_max >= 0.0 && a.eta >= 0.0)) return ISLS_ERR_ARG;
    if (a.B == 0) return ISLS_OK;
    urtc::Kernels k;
    if ((rc = prepare<T>(a.cost_model, n, m, s, &k)) != ISLS_OK) return rc;
    UserConP<T> p;
    p.B = a.B; p.N = a.N; p.update = a.update ? 1 : 0;
    p.par = (const T *)a.cost_par; p.par_sb = a.cost_par_sb;
    p.tab = (T *)a.tab; p.tab_sb = a.tab_sb;
    p.xhat = (const T *)a.xhat; p.uhat = (const T *)a.uhat;
    p.viol = (T *)a.viol; p.viol_prev = (T *)a.viol_prev; p.g_out = (T *)a.g_out;
    p.eta = (T)a.eta; p.phi = (T)a.phi; p.mu_max = (T)a.mu_max;
    p.active = a.active;
    void *args[] = {&p};
    return urtc::launch(k.of(urtc::ROLE_CON_UPDATE), a.B, 0, s, args);
}

}  // namespace isls

using namespace isls;

ISLS_API int isls_user_cost_create(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t *id)
{
    return urtc::create(urtc::KIND_COST, source, n, m, n_par, 0, id);
}

ISLS_API int isls_user_cost_create_tab(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t n_tab, int32_t *id)
{
    return urtc::create(urtc::KIND_COST, source, n, m, n_par, n_tab, id);
}

ISLS_API int isls_user_cost_create_con(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t n_tab, int32_t n_con, int32_t *id)
{
    return urtc::create(urtc::KIND_COST, source, n, m, n_par, n_tab, id, n_con);
}

ISLS_API int isls_user_cost_create_field(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t n_tab, int32_t n_con,
                                         int32_t n_field, int32_t nx, int32_t ny, int32_t *id)
{
    if (n_field < 1) return ISLS_ERR_UNSUPPORTED;             // (0 is the other creates')
    return urtc::create(urtc::KIND_COST, source, n, m, n_par, n_tab, id, n_con, n_field, nx, ny);
}

ISLS_API int isls_user_cost_set_field(int32_t id, const void *values, int32_t dtype_of_values, const double origin[2],
                                      const double spacing[2], void *stream)
{
    return urtc::set_field(id, values, dtype_of_values, origin, spacing, (hipStream_t)stream);
}

ISLS_API int isls_user_cost_field_dims(int32_t id, int32_t *n_field, int32_t *nx, int32_t *ny)
{
    return urtc::field_dims(id, n_field, nx, ny);
}

ISLS_API int isls_user_cost_field_ptr(int32_t id, int32_t dtype, void **ptr) { return urtc::field_ptr(id, dtype, ptr); }

ISLS_API int isls_user_cost_release_field(int32_t id) { return urtc::release_field(id); }

ISLS_API int isls_user_cost_n_tab(int32_t id) { return urtc::n_tab(id); }

ISLS_API int isls_user_cost_n_con(int32_t id) { return urtc::n_con(id); }

ISLS_API int64_t isls_user_cost_log(int32_t id, char *buf, int64_t len) { return urtc::copy_log(urtc::KIND_COST, id, buf, len); }

// (a negative model: the cost's own program, expansion and value only)
ISLS_API int isls_user_cost_code(int32_t id, int32_t model, int32_t dtype, void *buf, int64_t *len)
{
    return is_user_cost(id) ? urtc::copy_code(model < 0 ? urtc::kNone : model, id, dtype, buf, len) : ISLS_ERR_ARG;
}

ISLS_API int isls_user_cost_load(int32_t id, int32_t model, int32_t dtype)
{
    return is_user_cost(id) ? urtc::load(model < 0 ? urtc::kNone : model, id, dtype) : ISLS_ERR_ARG;
}

ISLS_TYPED_PAIR(user_cost_value, (int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *x, const void *u, void *cost,
                                  void *stream),
                return user_cost_value<T>(id, R, N, par, par_sb, nullptr, 0, x, u, cost, nullptr, (hipStream_t)stream);)
ISLS_TYPED_PAIR(user_cost_value_tab, (int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *tab, int64_t tab_sb,
                                      const void *x, const void *u, void *cost, void *stream),
                return user_cost_value<T>(id, R, N, par, par_sb, tab, tab_sb, x, u, cost, nullptr, (hipStream_t)stream);)
ISLS_TYPED_PAIR(user_cost_expand, (const isls_expand_args *a, void *Cux, void *stream),
                return a && is_user_cost(a->cost_model) ? launch_expand_user_cost<T>(*a, Cux, (hipStream_t)stream) : ISLS_ERR_ARG;)
ISLS_TYPED_PAIR(user_constraint_update, (const isls_constraint_update_args *a, void *stream),
                return a && is_user_cost(a->cost_model) ? launch_constraint_update<T>(*a, (hipStream_t)stream) : ISLS_ERR_ARG;)
