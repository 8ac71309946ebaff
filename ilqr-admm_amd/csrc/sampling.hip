// sampling.hip -- isls_sample_nominal_*: argument checks and dispatch of one sampling round about the nominal (kernel templates:
// sampling.hpp).  The (n, m, model) families of families.def run the library's instantiations; a user model and / or a user
// cost runs the sampling kernels of its run-time compiled (model, cost) program (user_rtc.hip).  isls_sample_nominal_fb_* is the same
// round in closed loop about the caller's gains: the same checks and dispatch, the *_fb_kernel pair and its argument block.
#include "sampling.hpp"
#include "user_rtc.hpp"

namespace isls {

constexpr size_t kSmpMaxLds = 48 * 1024;                      // the update keeps u_new [N][m] in LDS (closed loop: and x_new [N][n])

template <typename T>
int launch_sample_user(const SampleP<T> &p0, int model, int cost, int n, int m, size_t smem_cost, size_t smem_update, int phase, hipStream_t s,
                       const T *K, int64_t K_sb)
{
    urtc::Kernels k;
    const int rc = urtc::prepare(model, cost, urtc::dtype_of<T>(), n, m, s, &k);
    if (rc != ISLS_OK) return rc;
    SampleP<T> p = p0;
    SampleFbP<T> q = {p0, K, K_sb};
    void *args[] = {K ? (void *)&q : (void *)&p};
    const int64_t grid = (int64_t)p.B * p.chunks;
    const int rc1 = phase == 2 ? ISLS_OK : urtc::launch(k.of(K ? urtc::ROLE_SMP_COST_FB : urtc::ROLE_SMP_COST), (int)grid, smem_cost, s, args);
    return rc1 != ISLS_OK || phase == 1 ? rc1 : urtc::launch(k.of(K ? urtc::ROLE_SMP_UPDATE_FB : urtc::ROLE_SMP_UPDATE), p.B, smem_update, s, args);
}
template int launch_sample_user<double>(const SampleP<double> &, int, int, int, int, size_t, size_t, int, hipStream_t, const double *, int64_t);
template int launch_sample_user<float>(const SampleP<float> &, int, int, int, int, size_t, size_t, int, hipStream_t, const float *, int64_t);

// both entry points: fb = the closed-loop round about the gains K [.,N,m,n] (batch stride K_sb)
template <typename T>
static int launch_sample_round(const isls_sample_args &a, bool fb, const T *K, int64_t K_sb, hipStream_t s)
{
    if (fb && (!K || K_sb < 0)) return ISLS_ERR_ARG;
    if (a.B < 0 || a.N < 1 || a.S < 1 || a.n < 1 || a.m < 1) return ISLS_ERR_ARG;
    if (!a.xhat || !a.uhat || !a.model_par || !a.sigma || !a.costs) return ISLS_ERR_ARG;
    if (a.model_par_sb < 0 || a.cost_par_sb < 0 || a.Qtab_sb < 0 || a.ztab_sb < 0 || a.sigma_sb < 0 || a.stat_sb < 0) return ISLS_ERR_ARG;
    if (!(a.temperature > 0.0) || !(a.temperature < __builtin_huge_val())) return ISLS_ERR_ARG;
    const bool ucost = is_user_cost(a.cost_model), umodel = is_user_model(a.model);
    if (a.cost_model == ISLS_COST_VIA && (!a.Qtab || !a.ztab || !a.seq)) return ISLS_ERR_ARG;
    if (ucost && !a.cost_par) return ISLS_ERR_ARG;
    if (!dims_supported(a.n, a.m)) return ISLS_ERR_UNSUPPORTED;
    if (!ucost && a.cost_model != ISLS_COST_VIA && (a.cost_model != ISLS_COST_PHUBER || a.model != ISLS_MODEL_TASSA || !a.cost_par))
        return ISLS_ERR_UNSUPPORTED;
    if (ucost) {
        const int rc = urtc::check_table(a.cost_model, a.N, a.ztab, a.ztab_sb, a.nvia);
        if (rc != ISLS_OK) return rc;
    }
    if (umodel) {                                              // a table model: [par | N rows] behind model_par
        const int rc = urtc::check_model_table(a.model, a.N, a.model_par, a.model_par_sb);
        if (rc != ISLS_OK) return rc;
    }
    const int64_t chunks = ((int64_t)a.S + kWave - 1) / kWave;
    if ((int64_t)a.B * chunks > 0x7fffffff) return ISLS_ERR_UNSUPPORTED;
    if (a.phase < 0 || a.phase > 2) return ISLS_ERR_ARG;
    if (a.B == 0) return ISLS_OK;

    SampleP<T> p;
    p.B = a.B; p.N = a.N; p.S = a.S; p.chunks = (int)chunks;
    p.cost_model = a.cost_model;
    p.par = (const T *)a.model_par; p.par_sb = a.model_par_sb;
    p.xhat = (T *)a.xhat; p.uhat = (T *)a.uhat;
    p.Qtab = (const T *)a.Qtab; p.ztab = (const T *)a.ztab; p.Qtab_sb = a.Qtab_sb; p.ztab_sb = a.ztab_sb;
    p.seq = a.seq; p.u_std = (T)a.u_std;
    p.cpar = (const T *)a.cost_par; p.cpar_sb = ucost ? a.cost_par_sb : 0;
    p.sigma = (const T *)a.sigma; p.sigma_sb = a.sigma_sb;
    p.u_lo = (const T *)a.u_lo; p.u_hi = (const T *)a.u_hi;
    p.temperature = (T)a.temperature;
    p.seed = a.seed; p.problem0 = (unsigned int)a.problem0; p.problem_ids = a.problem_ids;
    p.active = a.active;
    p.costs = (T *)a.costs;
    p.cost_before = (T *)a.cost_before; p.cost_after = (T *)a.cost_after; p.cost_best = (T *)a.cost_best; p.ess = (T *)a.ess;
    p.took_best = a.took_best; p.stat_sb = a.stat_sb;

    const size_t ubytes = (size_t)a.N * (a.m + (fb ? a.n : 0)) * sizeof(T);   // closed loop: x_new [N][n] behind u_new
    const SampleFbP<T> q = {p, K, K_sb};
    if (umodel || ucost) {
        // a user model keeps its parameters in registers; a built-in model under a user cost brings its LDS words
        const int mdlw = umodel ? 0 : family_lds_words(a.n, a.m, a.model);
        if (mdlw < 0) return ISLS_ERR_UNSUPPORTED;
        const size_t smem2 = smp_mdl_words(mdlw) * sizeof(T) + ubytes;
        if (smem2 > kSmpMaxLds) return ISLS_ERR_UNSUPPORTED;
        return launch_sample_user<T>(p, a.model, ucost ? a.cost_model : urtc::kNone, a.n, a.m, mdlw * sizeof(T), smem2, a.phase, s,
                                     fb ? K : nullptr, K_sb);
    }
#define FAMILY(NX_, NU_, MODEL_)                                                                                              \
    if (a.n == NX_ && a.m == NU_ && a.model == MODEL_) {                                                                      \
        constexpr int MDLW = Model<T, NX_, NU_, MODEL_>::LDS_WORDS;                                                           \
        const size_t smem2 = smp_mdl_words(MDLW) * sizeof(T) + ubytes;                                                        \
        if (smem2 > kSmpMaxLds) return ISLS_ERR_UNSUPPORTED;                                                                  \
        if (a.phase != 2 && !fb)                                                                                              \
            hipLaunchKernelGGL((sample_cost_kernel<T, NX_, NU_, MODEL_>), dim3((unsigned)(a.B * chunks)), dim3(kWave),        \
                               MDLW * sizeof(T), s, p);                                                                       \
        if (a.phase != 2 && fb)                                                                                               \
            hipLaunchKernelGGL((sample_cost_fb_kernel<T, NX_, NU_, MODEL_>), dim3((unsigned)(a.B * chunks)), dim3(kWave),     \
                               MDLW * sizeof(T), s, q);                                                                       \
        if (check_launch() != ISLS_OK) return ISLS_ERR_LAUNCH;                                                                \
        if (a.phase == 1) return ISLS_OK;                                                                                     \
        if (fb)                                                                                                               \
            hipLaunchKernelGGL((sample_update_fb_kernel<T, NX_, NU_, MODEL_>), dim3((unsigned)a.B), dim3(kWave), smem2, s, q);\
        else                                                                                                                  \
            hipLaunchKernelGGL((sample_update_kernel<T, NX_, NU_, MODEL_>), dim3((unsigned)a.B), dim3(kWave), smem2, s, p);   \
        return check_launch();                                                                                                \
    }
    ISLS_FOR_EACH_FAMILY(FAMILY)
#undef FAMILY
    return ISLS_ERR_UNSUPPORTED;
}

template <typename T>
int launch_sample_nominal(const isls_sample_args &a, hipStream_t s)
{
    return launch_sample_round<T>(a, false, nullptr, 0, s);
}
template int launch_sample_nominal<double>(const isls_sample_args &, hipStream_t);
template int launch_sample_nominal<float>(const isls_sample_args &, hipStream_t);

template <typename T>
int launch_sample_nominal_fb(const isls_sample_args &a, const void *K, int64_t K_sb, hipStream_t s)
{
    return launch_sample_round<T>(a, true, (const T *)K, K_sb, s);
}
template int launch_sample_nominal_fb<double>(const isls_sample_args &, const void *, int64_t, hipStream_t);
template int launch_sample_nominal_fb<float>(const isls_sample_args &, const void *, int64_t, hipStream_t);

}  // namespace isls
