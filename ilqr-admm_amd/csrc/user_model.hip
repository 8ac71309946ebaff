// user_model.hip -- user-written forward models: the launches of a model's own kernels -- linearisation, dense closed loop,
// row-wise step (the device side is user_model.hpp) -- and the isls_user_model_* entry points.  Registry, run-time compilation,
// module loading and the line search are user_rtc.hip's: a model's program is the key (model, no cost) there.
#include "entry.hpp"
#include "mpc.hpp"
#include "user_rtc.hpp"

namespace isls {

// the kernels of model `id`'s own program for a launch of dims (n, m)
template <typename T>
static int prepare(int id, int n, int m, hipStream_t s, urtc::Kernels *k)
{
    return urtc::prepare(id, urtc::kNone, urtc::dtype_of<T>(), n, m, s, k);
}

// ---- launches (dispatched from misc.hip / rollout.hip on a.model >= ISLS_MODEL_USER_BASE) -----------------------------------
template <typename T>
int launch_linearize_user(const isls_linearize_args &a, hipStream_t s)
{
    if (a.B < 0 || a.N < 1 || !a.model_par || !a.A || !a.Bm || !a.xhat || !a.uhat) return ISLS_ERR_ARG;
    int rc = urtc::check_model_table(a.model, a.N, a.model_par, a.model_par_sb);
    if (rc != ISLS_OK) return rc;
    if (a.B == 0) return ISLS_OK;
    urtc::Kernels k;
    rc = prepare<T>(a.model, a.n, a.m, s, &k);
    if (rc != ISLS_OK) return rc;
    const int steps = kWave / (a.n + a.m);                   // steps per workgroup (user_linearize_kernel's S)
    UserLinP<T> p;
    p.B = a.B; p.N = a.N; p.nbt = (a.N + steps - 1) / steps;
    p.par = (const T *)a.model_par; p.par_sb = a.model_par_sb;
    p.xhat = (const T *)a.xhat; p.uhat = (const T *)a.uhat; p.A = (T *)a.A; p.Bm = (T *)a.Bm; p.active = a.active;
    const int64_t grid = (int64_t)a.B * p.nbt;
    if (grid > 0x7fffffff) return ISLS_ERR_UNSUPPORTED;
    void *args[] = {&p};
    return urtc::launch(k.of(urtc::ROLE_LIN), (int)grid, 0, s, args);
}
template int launch_linearize_user<double>(const isls_linearize_args &, hipStream_t);
template int launch_linearize_user<float>(const isls_linearize_args &, hipStream_t);

template <typename T>
int launch_dense_closed_loop_user(const DenseLoopP<T> &p0, const isls_dense_loop_args &a, hipStream_t s)
{
    if (urtc::model_n_tab(a.model) != 0) return ISLS_ERR_UNSUPPORTED;   // a table model: not served (isls_hip.h)
    urtc::Kernels k;
    const int rc = prepare<T>(a.model, a.n, a.m, s, &k);
    if (rc != ISLS_OK) return rc;
    DenseLoopP<T> p = p0;
    void *args[] = {&p};
    return urtc::launch(k.of(urtc::ROLE_LOOP), (a.M + 63) / 64, sizeof(T), s, args);
}
template int launch_dense_closed_loop_user<double>(const DenseLoopP<double> &, const isls_dense_loop_args &, hipStream_t);
template int launch_dense_closed_loop_user<float>(const DenseLoopP<float> &, const isls_dense_loop_args &, hipStream_t);

template <typename T>
int launch_mc_closed_loop_user(const McP<T> &p0, int model, int grid, int lanes, size_t smem, hipStream_t s)
{
    if (urtc::model_n_tab(model) != 0) return ISLS_ERR_UNSUPPORTED;     // a table model: not served (isls_hip.h)
    urtc::Kernels k;
    const int rc = prepare<T>(model, p0.n, p0.m, s, &k);
    if (rc != ISLS_OK) return rc;
    McP<T> p = p0;
    void *args[] = {&p};
    return urtc::launch(k.of(urtc::ROLE_MC), grid, smem, s, args, lanes);
}
template int launch_mc_closed_loop_user<double>(const McP<double> &, int, int, int, size_t, hipStream_t);
template int launch_mc_closed_loop_user<float>(const McP<float> &, int, int, int, size_t, hipStream_t);

template <typename T>
int launch_mpc_step_user(const MpcP<T> &p0, int model, int grid, size_t smem, hipStream_t s)
{
    // a table model: the window [par | N rows] in par, and a plant buffer that reaches row 0 at least
    int rc = urtc::check_model_table(model, p0.N, p0.par, p0.par_sb);
    if (rc == ISLS_OK) rc = urtc::check_model_table(model, p0.N, p0.plant, p0.plant_sb, 1);
    if (rc != ISLS_OK) return rc;
    urtc::Kernels k;
    rc = prepare<T>(model, p0.n, p0.m, s, &k);
    if (rc != ISLS_OK) return rc;
    MpcP<T> p = p0;
    void *args[] = {&p};
    return urtc::launch(k.of(urtc::ROLE_MPC), grid, smem, s, args);
}
template int launch_mpc_step_user<double>(const MpcP<double> &, int, int, size_t, hipStream_t);
template int launch_mpc_step_user<float>(const MpcP<float> &, int, int, size_t, hipStream_t);

// run = 0: the entry point without a table (one parameter row per state row); run >= 1: isls_user_model_step_tab_*
template <typename T>
static int user_step(int32_t id, int32_t R, const void *par, int64_t par_sb, const void *x, const void *u, void *xn, hipStream_t s,
                     int32_t run = 0, int32_t N = 0, const int32_t *tix = nullptr)
{
    if (R < 0 || !par || !x || !u || !xn || par_sb < 0) return ISLS_ERR_ARG;
    int n, m;
    int rc = urtc::dims(urtc::KIND_MODEL, id, &n, &m);
    if (rc != ISLS_OK) return rc;
    const int W = urtc::model_n_tab(id);
    if ((W > 0) != (run > 0)) return ISLS_ERR_ARG;             // a table model steps through the _tab entry, and only it
    if (W > 0 && ((rc = urtc::check_model_table(id, N, par, par_sb)) != ISLS_OK || (!tix && run > N))) return ISLS_ERR_ARG;
    if (R == 0) return rc;
    urtc::Kernels k;
    if ((rc = prepare<T>(id, n, m, s, &k)) != ISLS_OK) return rc;
    int R_ = R;
    const T *par_ = (const T *)par, *x_ = (const T *)x, *u_ = (const T *)u;
    T *xn_ = (T *)xn;
    int run_ = run > 0 ? run : 1;
    void *args[] = {&R_, &par_, &par_sb, &x_, &u_, &xn_, &run_, &tix};
    return urtc::launch(k.of(W > 0 ? urtc::ROLE_STEP_TAB : urtc::ROLE_STEP), (R + 63) / 64, 0, s, args);
}

}  // namespace isls

using namespace isls;

ISLS_API int isls_user_model_create(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t *id)
{
    return urtc::create(urtc::KIND_MODEL, source, n, m, n_par, 0, id);
}

ISLS_API int isls_user_model_create_tab(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t n_tab, int32_t *id)
{
    return urtc::create(urtc::KIND_MODEL, source, n, m, n_par, n_tab, id);
}

ISLS_API int isls_user_model_n_tab(int32_t id) { return is_user_model(id) ? urtc::model_n_tab(id) : ISLS_ERR_ARG; }

ISLS_API int64_t isls_user_model_log(int32_t id, char *buf, int64_t len) { return urtc::copy_log(urtc::KIND_MODEL, id, buf, len); }

ISLS_API int isls_user_model_code(int32_t id, int32_t dtype, void *buf, int64_t *len)
{
    return urtc::copy_code(id, urtc::kNone, dtype, buf, len);
}

ISLS_API int isls_user_model_load(int32_t id, int32_t dtype) { return urtc::load(id, urtc::kNone, dtype); }

ISLS_TYPED_PAIR(user_model_step, (int32_t id, int32_t R, const void *par, int64_t par_sb, const void *x, const void *u, void *xn, void *stream),
                return user_step<T>(id, R, par, par_sb, x, u, xn, (hipStream_t)stream);)
ISLS_TYPED_PAIR(user_model_step_tab, (int32_t id, int32_t R, int32_t run, int32_t N, const void *par, int64_t par_sb, const int32_t *t,
                                      const void *x, const void *u, void *xn, void *stream),
                return run < 1 ? ISLS_ERR_ARG : user_step<T>(id, R, par, par_sb, x, u, xn, (hipStream_t)stream, run, N, t);)
