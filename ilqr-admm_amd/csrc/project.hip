// project.hip -- isls_project_rows_*: row-wise projections / project_set_convex for P problems x R rows
// (isls/projections.py; device code in projections.hpp).  One workgroup per problem, one thread per row; the
// reference stops all rows of a call together, so every inner iteration ends with a workgroup-wide max.
#include "projections.hpp"

namespace isls {

template <typename T>
struct ProjP {
    int P, R, nsets, max_iter, algorithm;
    T rho, threshold;
    int kind[kMaxSets], dim[kMaxSets];
    const T *A[kMaxSets], *b[kMaxSets], *par[kMaxSets];
    int64_t A_sp[kMaxSets], b_sp[kMaxSets], par_sp[kMaxSets];
    const T *y_in;
    T *y_out;
    int64_t in_sp, in_sr, out_sp, out_sr;
    int32_t *iters;
    const int32_t *active;
    const int32_t *row_mask;
};

// BLOCK = largest workgroup the instance is launched with: up to 256 threads (R <= 256, the usual case: rows = time
// steps or N*m) a wave may use the whole register file; 1024-thread workgroups are capped at 128 VGPRs.
// ROWS = some set of the stage carries ISLS_SET_ROW_PAR / ISLS_SET_ROW_B (p.kind[s] keeps the flag bits): every thread reads
// its own row's block of `par` / `b` (project_rows_moving_kernel).  The shared form (project_rows_kernel) stays an instance of
// its own: there the set operands are uniform over the wavefront (scalar loads, addresses in SGPRs); per-lane addresses for
// everybody would make them vector loads and cost registers in a kernel that sits at its VGPR caps.  One body for both
// (project_rows_body.inc), a kernel name each: the shared form keeps its symbol and its code.
template <typename T, int D, int BLOCK>
__global__ __launch_bounds__(BLOCK, (BLOCK <= 256 ? 2 : 1)) void project_rows_kernel(ProjP<T> p)
{
    constexpr bool ROWS = false;
#include "project_rows_body.inc"
}

template <typename T, int D, int BLOCK>
__global__ __launch_bounds__(BLOCK, (BLOCK <= 256 ? 2 : 1)) void project_rows_moving_kernel(ProjP<T> p)
{
    constexpr bool ROWS = true;
#include "project_rows_body.inc"
}

template <typename T>
int launch_project(const isls_project_args &a, hipStream_t s)
{
    if (a.P < 0 || a.R < 1 || a.R > 1024 || a.d < 1 || a.d > kMaxRowDim || a.nsets < 1 || a.nsets > kMaxSets) return ISLS_ERR_ARG;
    if (!a.y_in || !a.y_out) return ISLS_ERR_ARG;
    if (a.algorithm < ISLS_PROJ_ALG_ADMM || a.algorithm > ISLS_PROJ_ALG_SOC) return ISLS_ERR_UNSUPPORTED;
    const bool dyk = a.algorithm == ISLS_PROJ_ALG_DYKSTRA;
    const bool direct = a.algorithm == ISLS_PROJ_ALG_ADMM && a.nsets == 1 && a.sets[0].A == nullptr;
    bool rows = false;                                         // a per-row table in this stage: the ROWS instance
    for (int i = 0; i < a.nsets; ++i) {
        const isls_cset &c = a.sets[i];
        const int kind = c.kind & ~ISLS_SET_ROW_FLAGS;
        if (kind < ISLS_SET_BOX || kind > ISLS_SET_MULTILINEAR) return ISLS_ERR_UNSUPPORTED;
        if (c.dim < 1 || c.dim > kMaxSetDim) return ISLS_ERR_ARG;
        if (!direct && !dyk && (!c.A || !c.b)) return ISLS_ERR_ARG;
        if (kind != ISLS_SET_SOC_UNIT && !c.par) return ISLS_ERR_ARG;
        if ((direct || dyk) && c.dim != a.d) return ISLS_ERR_ARG;      // the set acts on the row itself
        if ((c.kind & ISLS_SET_ROW_PAR) && kind == ISLS_SET_SOC_UNIT) return ISLS_ERR_ARG;   // no parameters to move
        if ((c.kind & ISLS_SET_ROW_B) && (direct || dyk)) return ISLS_ERR_ARG;               // b is not used there
        rows = rows || (c.kind & ISLS_SET_ROW_FLAGS) != 0;
    }
    if (a.algorithm == ISLS_PROJ_ALG_SOC && (a.nsets != 1 || (a.sets[0].kind & ~ISLS_SET_ROW_FLAGS) != ISLS_SET_SOC_UNIT))
        return ISLS_ERR_ARG;
    if (!direct && a.max_iter < 1) return ISLS_ERR_ARG;
    if (!direct && !dyk && !(a.rho > 0)) return ISLS_ERR_ARG;
    if (a.P == 0) return ISLS_OK;
    ProjP<T> p = {};
    p.P = a.P; p.R = a.R; p.nsets = a.nsets; p.max_iter = a.max_iter; p.algorithm = a.algorithm;
    p.rho = (T)a.rho; p.threshold = (T)a.threshold;
    for (int i = 0; i < kMaxSets; ++i) {
        const bool on = i < a.nsets;
        p.kind[i] = on ? a.sets[i].kind : 0;
        p.dim[i] = on ? a.sets[i].dim : 0;
        p.A[i] = on ? (const T *)a.sets[i].A : nullptr;
        p.b[i] = on ? (const T *)a.sets[i].b : nullptr;
        p.par[i] = on ? (const T *)a.sets[i].par : nullptr;
        p.A_sp[i] = on ? a.sets[i].A_sp : 0; p.b_sp[i] = on ? a.sets[i].b_sp : 0; p.par_sp[i] = on ? a.sets[i].par_sp : 0;
    }
    p.y_in = (const T *)a.y_in; p.y_out = (T *)a.y_out;
    p.in_sp = a.in_sp; p.in_sr = a.in_sr; p.out_sp = a.out_sp; p.out_sr = a.out_sr;
    p.iters = a.iters; p.active = a.active; p.row_mask = a.row_mask;
    const int threads = ((a.R + 63) / 64) * 64;
#define CALL_(K_, D_)                                                                                         \
    if (threads <= 256) hipLaunchKernelGGL((K_<T, D_, 256>), dim3(a.P), dim3(threads), 0, s, p);              \
    else if (threads <= 512) hipLaunchKernelGGL((K_<T, D_, 512>), dim3(a.P), dim3(threads), 0, s, p); /* 256 VGPRs: no spills at fp64 */ \
    else hipLaunchKernelGGL((K_<T, D_, 1024>), dim3(a.P), dim3(threads), 0, s, p)
#define CALL(D_)                                                                                              \
    if (rows) { CALL_(project_rows_moving_kernel, D_); } else { CALL_(project_rows_kernel, D_); }
    switch (a.d) {
        case 1: CALL(1); break;
        case 2: CALL(2); break;
        case 3: CALL(3); break;
        default: CALL(4); break;
    }
#undef CALL
#undef CALL_
    int rc = check_launch();
    if (rc == ISLS_OK && a.next) {                             // next stage, in place on this stage's output
        isls_project_args nx = *a.next;
        nx.P = a.P; nx.R = a.R; nx.d = a.d;
        nx.y_in = a.y_out; nx.y_out = a.y_out;
        nx.in_sp = nx.out_sp = a.out_sp; nx.in_sr = nx.out_sr = a.out_sr;
        nx.iters = nullptr; nx.active = a.active;
        rc = launch_project<T>(nx, s);
    }
    return rc;
}
template int launch_project<double>(const isls_project_args &, hipStream_t);
template int launch_project<float>(const isls_project_args &, hipStream_t);

}  // namespace isls
