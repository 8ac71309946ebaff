// monte_carlo.hip -- isls_mc_closed_loop_*: argument checks, launch plan and dispatch of the Monte-Carlo closed loop (kernel
// template: monte_carlo.hpp).  The built-in (n, m, model) families of families.def run at their own dimensions, every other dense
// LTI pair with n <= 16, m <= 8 runs the instantiation with run-time dimensions, a user model goes to user_model.hip.
#include "monte_carlo.hpp"

namespace isls {

constexpr int kMcMaxN = 16, kMcMaxM = 8;
constexpr size_t kMcLdsBytes = 64 * 1024;

// elements of the caller's scratch: form 1 keeps dx of every (sample, step) in a sample-fastest layout, one block of
// [N n][lanes] per workgroup of 64 or 128 lanes
int64_t mc_work_elems(int32_t P, int32_t M, int32_t N, int32_t n, int32_t m, int32_t K_form)
{
    if (P < 0 || M < 0 || N < 1 || n < 1 || n > kMcMaxN || m < 1 || m > kMcMaxM || K_form != 1) return 0;
    return (int64_t)P * (((int64_t)M + 127) / 128 * 128) * N * n;
}

template <typename T>
int launch_mc_closed_loop(const isls_mc_loop_args &a, hipStream_t s)
{
    if (a.P < 0 || a.M < 0 || a.N < 1 || a.n < 1 || a.n > kMcMaxN || a.m < 1 || a.m > kMcMaxM) return ISLS_ERR_ARG;
    if (a.K_form != 0 && a.K_form != 1) return ISLS_ERR_ARG;
    if (!a.model_par || !a.K || !a.k) return ISLS_ERR_ARG;
    if ((a.x0s != nullptr) == (a.x0 != nullptr)) return ISLS_ERR_ARG;          // one source of initial states
    if (a.x0s && a.x0_std) return ISLS_ERR_ARG;
    if (a.w && a.noise_std) return ISLS_ERR_ARG;                                // at most one source of noise
    if (a.par_sb < 0 || a.K_sb < 0 || a.k_sb < 0 || a.xhat_sb < 0 || a.uhat_sb < 0 || a.x0_sb < 0) return ISLS_ERR_ARG;
    if (a.K_form == 1 && (!a.work || a.work_elems < mc_work_elems(a.P, a.M, a.N, a.n, a.m, 1))) return ISLS_ERR_ARG;
    if (a.P == 0 || a.M == 0) return ISLS_OK;

    McP<T> p;
    p.P = a.P; p.M = a.M; p.N = a.N; p.n = a.n; p.m = a.m;
    p.form = a.K_form;
    p.nw = (a.w || a.noise_std) ? 1 : 0;
    p.par = (const T *)a.model_par; p.par_sb = a.par_sb;
    p.K = (const T *)a.K; p.k = (const T *)a.k; p.K_sb = a.K_sb; p.k_sb = a.k_sb;
    p.xhat = (const T *)a.xhat; p.uhat = (const T *)a.uhat; p.xhat_sb = a.xhat_sb; p.uhat_sb = a.uhat_sb;
    p.x0s = (const T *)a.x0s; p.x0 = (const T *)a.x0; p.x0_std = (const T *)a.x0_std; p.x0_sb = a.x0_sb;
    p.w = (const T *)a.w; p.noise_std = (const T *)a.noise_std;
    p.seed = a.seed; p.problem0 = (unsigned int)a.problem0; p.sample0 = (unsigned int)a.sample0;
    p.u_lo = View<T>(a.u_lo); p.u_hi = View<T>(a.u_hi); p.x_lo = View<T>(a.x_lo); p.x_hi = View<T>(a.x_hi);
    p.viol_u = a.viol_u; p.viol_x = a.viol_x; p.viol_any = a.viol_any;
    p.u_min = (T *)a.u_min; p.u_max = (T *)a.u_max; p.x_min = (T *)a.x_min; p.x_max = (T *)a.x_max;
    p.x_log = (T *)a.x_log; p.u_log = (T *)a.u_log; p.w_out = (T *)a.w_out; p.x0_out = (T *)a.x0_out;
    p.work = (T *)a.work;

    const bool user = is_user_model(a.model);
    int mdlw = -1;
    bool rt = false;
    if (user) {
        mdlw = 0;
    } else {
#define FAMILY(NX_, NU_, MODEL_) \
    if (a.n == NX_ && a.m == NU_ && a.model == MODEL_) mdlw = McModel<T, NX_, NU_, MODEL_>::LDS_WORDS;
        ISLS_FOR_EACH_FAMILY(FAMILY)
#undef FAMILY
        if (mdlw < 0 && a.model == ISLS_MODEL_LTI) {
            rt = true;
            mdlw = McModel<T, kMcMaxN, kMcMaxM, kMcModelRt>::LDS_WORDS;
        }
        if (mdlw < 0) return ISLS_ERR_UNSUPPORTED;
    }
    // the plan: tiles of kMcTile steps, halved while the stage of 64 lanes does not fit; 128 lanes where their stage fits too
    int tt = kMcTile, lanes = 64;
    while (tt > 1 && mc_plan(a.n, a.m, tt, p.nw, p.form, 64, mdlw).words * sizeof(T) > kMcLdsBytes) tt /= 2;
    if (mc_plan(a.n, a.m, tt, p.nw, p.form, 128, mdlw).words * sizeof(T) <= kMcLdsBytes && a.M > 64) lanes = 128;
    const size_t smem = mc_plan(a.n, a.m, tt, p.nw, p.form, lanes, mdlw).words * sizeof(T);
    if (smem > kMcLdsBytes) return ISLS_ERR_UNSUPPORTED;
    p.tt = tt;
    p.tiles = (a.M + lanes - 1) / lanes;
    const int64_t grid = (int64_t)a.P * p.tiles;
    if (grid > 0x7fffffff) return ISLS_ERR_UNSUPPORTED;

    if (user) return launch_mc_closed_loop_user<T>(p, a.model, (int)grid, lanes, smem, s);
    if (rt) {
        hipLaunchKernelGGL((mc_closed_loop_kernel<T, kMcMaxN, kMcMaxM, kMcModelRt>), dim3((unsigned)grid), dim3(lanes), smem, s, p);
        return check_launch();
    }
#define FAMILY(NX_, NU_, MODEL_)                                                                                              \
    if (a.n == NX_ && a.m == NU_ && a.model == MODEL_) {                                                                      \
        hipLaunchKernelGGL((mc_closed_loop_kernel<T, NX_, NU_, MODEL_>), dim3((unsigned)grid), dim3(lanes), smem, s, p);      \
        return check_launch();                                                                                                \
    }
    ISLS_FOR_EACH_FAMILY(FAMILY)
#undef FAMILY
    return ISLS_ERR_UNSUPPORTED;
}
template int launch_mc_closed_loop<double>(const isls_mc_loop_args &, hipStream_t);
template int launch_mc_closed_loop<float>(const isls_mc_loop_args &, hipStream_t);

}  // namespace isls
