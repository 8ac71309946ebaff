// mpc.hip -- isls_mpc_step_*: argument checks and dispatch of the receding-horizon control step (kernel template: mpc.hpp).  The
// built-in (n, m, model) families of families.def run at their own dimensions, every other dense LTI pair with n <= 16, m <= 8
// runs the instantiation with run-time dimensions, a user model goes to user_model.hip.
#include "mpc.hpp"

namespace isls {

constexpr int kMpcMaxN = 16, kMpcMaxM = 8;

template <typename T>
int launch_mpc_step(const isls_mpc_step_args &a, hipStream_t s)
{
    if (a.B < 0 || a.N < 1 || a.n < 1 || a.n > kMpcMaxN || a.m < 1 || a.m > kMpcMaxM) return ISLS_ERR_ARG;
    if (!a.xhat || !a.uhat || !a.model_par) return ISLS_ERR_ARG;
    if (a.par_sb < 0 || a.plant_sb < 0 || a.tab_sb < 0 || a.tab_next_sb < 0 || a.x_meas_sb < 0 || a.u_out_sb < 0 || a.x_next_sb < 0)
        return ISLS_ERR_ARG;
    if (a.tab && (a.W < 1 || a.W > kMpcMaxTab)) return ISLS_ERR_ARG;
    if (a.w && a.noise_std) return ISLS_ERR_ARG;               // at most one source of disturbance
    if (a.B == 0) return ISLS_OK;

    MpcP<T> p;
    p.B = a.B; p.N = a.N; p.n = a.n; p.m = a.m; p.W = a.tab ? a.W : 0;
    p.par = (const T *)a.model_par; p.par_sb = a.par_sb;
    p.plant = a.plant_par ? (const T *)a.plant_par : p.par;
    p.plant_sb = a.plant_par ? a.plant_sb : a.par_sb;
    p.xhat = (T *)a.xhat; p.uhat = (T *)a.uhat; p.K = (T *)a.K; p.zx = (T *)a.zx; p.zu = (T *)a.zu;
    p.tab = (T *)a.tab; p.tab_sb = a.tab_sb;
    p.tab_next = a.tab ? (const T *)a.tab_next : nullptr; p.tab_next_sb = a.tab_next_sb;
    p.u_lo = (const T *)a.u_lo; p.u_hi = (const T *)a.u_hi; p.w = (const T *)a.w; p.noise_std = (const T *)a.noise_std;
    p.seed = a.seed; p.problem0 = (unsigned int)a.problem0; p.step = (unsigned int)a.step;
    p.x_meas = (T *)a.x_meas_out; p.u_out = (T *)a.u_out; p.x_next = (T *)a.x_next_out;
    p.x_meas_sb = a.x_meas_sb; p.u_out_sb = a.u_out_sb; p.x_next_sb = a.x_next_sb;

    constexpr int TPW = kWave / kMpcLanes;
    const int64_t grid = ((int64_t)a.B + TPW - 1) / TPW;
    if (grid > 0x7fffffff) return ISLS_ERR_UNSUPPORTED;
    if (is_user_model(a.model)) {
        if (!dims_supported(a.n, a.m)) return ISLS_ERR_UNSUPPORTED;
        size_t smem = 0;
#define ISLS_MPC_DIMS_(NX_, NU_) if (a.n == NX_ && a.m == NU_) smem = TPW * MpcLayout<NX_, NU_>::slot_words(0) * sizeof(T);
        ISLS_FOR_EACH_DIMS(ISLS_MPC_DIMS_)
#undef ISLS_MPC_DIMS_
        return launch_mpc_step_user<T>(p, a.model, (int)grid, smem, s);
    }
#define FAMILY(NX_, NU_, MODEL_)                                                                                              \
    if (a.n == NX_ && a.m == NU_ && a.model == MODEL_) {                                                                      \
        const size_t smem = TPW * MpcLayout<NX_, NU_>::slot_words(McModel<T, NX_, NU_, MODEL_>::LDS_WORDS) * sizeof(T);       \
        hipLaunchKernelGGL((mpc_step_kernel<T, NX_, NU_, MODEL_>), dim3((unsigned)grid), dim3(kWave), smem, s, p);            \
        return check_launch();                                                                                                \
    }
    ISLS_FOR_EACH_FAMILY(FAMILY)
#undef FAMILY
    if (a.model == ISLS_MODEL_LTI) {
        const size_t smem = TPW * MpcLayout<kMpcMaxN, kMpcMaxM>::slot_words(McModel<T, kMpcMaxN, kMpcMaxM, kMcModelRt>::LDS_WORDS) * sizeof(T);
        hipLaunchKernelGGL((mpc_step_kernel<T, kMpcMaxN, kMpcMaxM, kMcModelRt>), dim3((unsigned)grid), dim3(kWave), smem, s, p);
        return check_launch();
    }
    return ISLS_ERR_UNSUPPORTED;
}
template int launch_mpc_step<double>(const isls_mpc_step_args &, hipStream_t);
template int launch_mpc_step<float>(const isls_mpc_step_args &, hipStream_t);

}  // namespace isls
