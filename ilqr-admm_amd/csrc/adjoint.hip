// adjoint.hip -- the costate sweep of the nominal's cost on gfx950 (isls_adjoint_sweep_*; formulae in include/isls_hip.h):
//     lam_{N-1} = c0x_{N-1} ;  lam_t = c0x_t + A_t' lam_{t+1} ;  gu_t = c0u_t + B_t' lam_{t+1} (t <= N-2) ;  gu_{N-1} = c0u_{N-1} ;  gx0 = lam_0
//
// Sequential in t and bound by the stream of A_t, B_t (n (n + m) words per step and trajectory against as many multiply-adds), so
// the kernel takes the layout of the feed-forward pass (riccati_ff.hip), cut down to what this recursion needs:
//   * one 64-lane wavefront per workgroup, TPW = 64 / (n + m) slots of G = n + m lanes, slot = trajectory;
//   * lane i of a slot owns COLUMN i of [A_t B_t]: x-lane i ends a step with lam_t[i], u-lane r with gu_t[r].  The lane reads its
//     column itself, word k from row k: one load instruction takes row k of A_t and row k of B_t of every slot, n + m contiguous
//     words per slot, and the n instructions of a step consume every byte of the step's two blocks.  Nothing is staged through
//     LDS and no lane strides alone through a trajectory's blocks;
//   * every lane keeps a ring of D steps of its column and its gradient entry in flight in registers; the loads are
//     unconditional (steps past the start are clamped, idle lanes shadow the block's first trajectory);
//   * the one hand-off of a step is lam_{t+1}: the x-lanes publish it in the slot's n words of LDS (slot_sync, no s_barrier).
#include "entry.hpp"
#include "isls_common.hpp"

namespace isls {

constexpr int kAdjDepth = 4;                                 // steps of operands in flight per lane

template <typename T>
struct AdjP {
    int B, N, n, m;
    View<T> A, Bm;
    const T *c0x, *c0u;
    T *lam, *gu, *gx0;
    const int32_t *active;
};

template <typename T, int NX, int NU, int D>
__global__ __launch_bounds__(64) void adjoint_sweep_kernel(AdjP<T> p)
{
    constexpr int G = NX + NU, TPW = kWave / G, SLOT = NX + 1;
    __shared__ T lds[(TPW + 1) * SLOT];                        // + one dump slot for the lanes beyond the last slot
    const int lane = threadIdx.x, s = lane / G, i = lane - s * G, N = p.N;
    const int b0 = blockIdx.x * TPW, b = b0 + s;
    const bool inslot = s < TPW, inbatch = inslot && b < p.B;
    const bool valid = inbatch && (p.active == nullptr || p.active[b] != 0);
    const int bl = inbatch ? b : b0;                           // idle lanes shadow the block's first trajectory (loads only)
    const bool xl = i < NX;
    const int iu = xl ? 0 : i - NX;
    T *rec = lds + (inslot ? s : TPW) * SLOT;

    // the lane's column: word k at pcol[t * cst + k * crow]; its gradient entry at pc0[t * c0st]
    const T *pcol = xl ? p.A.at(bl, 0) + i : p.Bm.at(bl, 0) + iu;
    const int64_t cst = xl ? p.A.st : p.Bm.st;
    const int crow = xl ? NX : NU;
    const int c0st = xl ? NX : NU;
    const T *pc0 = xl ? p.c0x + (int64_t)bl * N * NX + i : p.c0u + (int64_t)bl * N * NU + iu;
    T *pout = xl ? p.lam + (int64_t)bl * N * NX + i : p.gu + (int64_t)bl * N * NU + iu;

    struct Stage {
        T col[NX], c0;
    };
    auto fetch = [&](int t, Stage &g) {
        const T *c = pcol + (int64_t)t * cst;
#pragma unroll
        for (int k = 0; k < NX; ++k) g.col[k] = c[k * crow];
        g.c0 = pc0[(int64_t)t * c0st];
    };

    // terminal step: lam_{N-1} = c0x, gu_{N-1} = c0u
    T cur = pc0[(int64_t)(N - 1) * c0st];
    if (valid) pout[(int64_t)(N - 1) * c0st] = cur;
    if (xl) rec[i] = cur;
    slot_sync();

    Stage ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(N - 2 - d > 0 ? N - 2 - d : 0, ring[d]);

    // groups of D steps with the ring index a compile-time constant; the last group is padded with dead steps (t < 0: loads
    // clamped, nothing stored, lam left alone)
    for (int tb = N - 2; tb >= 0; tb -= D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = tb - d;
            const bool live = t >= 0;
            Stage &g = ring[d];
            T acc = T(0);
#pragma unroll
            for (int k = 0; k < NX; ++k) acc += g.col[k] * rec[k];
            const T val = g.c0 + acc;
            fetch(t - D > 0 ? t - D : 0, g);                   // refill (clamped, unconditional)
            slot_sync();                                       // every lane has read lam_{t+1}
            cur = live ? val : cur;
            if (xl) rec[i] = cur;
            if (valid && live) pout[(int64_t)t * c0st] = cur;
            slot_sync();
        }
    }
    if (valid && xl && p.gx0) p.gx0[(int64_t)b * NX + i] = cur;
}

// Any (n <= 16, m <= 8) without an instantiation above (dims_generic): the same slots and columns with run-time dimensions; the
// column words are consumed as they arrive (no register ring: its depth would be a run-time index).
template <typename T>
__global__ __launch_bounds__(64) void adjoint_sweep_generic_kernel(AdjP<T> p)
{
    constexpr int MAXN = 16;
    __shared__ T lds[(kWave / 2 + 1) * (MAXN + 1)];
    const int NX = p.n, NU = p.m, G = NX + NU, TPW = kWave / G, SLOT = NX + 1;
    const int lane = threadIdx.x, s = lane / G, i = lane - s * G, N = p.N;
    const int b0 = blockIdx.x * TPW, b = b0 + s;
    const bool inslot = s < TPW, inbatch = inslot && b < p.B;
    const bool valid = inbatch && (p.active == nullptr || p.active[b] != 0);
    const int bl = inbatch ? b : b0;
    const bool xl = i < NX;
    const int iu = xl ? 0 : i - NX;
    T *rec = lds + (inslot ? s : TPW) * SLOT;
    const T *pcol = xl ? p.A.at(bl, 0) + i : p.Bm.at(bl, 0) + iu;
    const int64_t cst = xl ? p.A.st : p.Bm.st;
    const int crow = xl ? NX : NU, c0st = crow;
    const T *pc0 = xl ? p.c0x + (int64_t)bl * N * NX + i : p.c0u + (int64_t)bl * N * NU + iu;
    T *pout = xl ? p.lam + (int64_t)bl * N * NX + i : p.gu + (int64_t)bl * N * NU + iu;

    T cur = pc0[(int64_t)(N - 1) * c0st];
    if (valid) pout[(int64_t)(N - 1) * c0st] = cur;
    if (xl) rec[i] = cur;
    slot_sync();
    for (int t = N - 2; t >= 0; --t) {
        const T *c = pcol + (int64_t)t * cst;
        T acc = T(0);
        for (int k = 0; k < NX; ++k) acc += c[k * crow] * rec[k];
        cur = pc0[(int64_t)t * c0st] + acc;
        slot_sync();
        if (xl) rec[i] = cur;
        if (valid) pout[(int64_t)t * c0st] = cur;
        slot_sync();
    }
    if (valid && xl && p.gx0) p.gx0[(int64_t)b * NX + i] = cur;
}

template <typename T>
int launch_adjoint(const isls_adjoint_args &a, hipStream_t s)
{
    if (a.B < 0 || a.N < 1 || !a.A.p || !a.Bm.p || !a.c0x || !a.c0u || !a.lam || !a.gu) return ISLS_ERR_ARG;
    if (a.A.sb < 0 || a.A.st < 0 || a.Bm.sb < 0 || a.Bm.st < 0) return ISLS_ERR_ARG;
    if (!dims_supported(a.n, a.m) && !dims_generic(a.n, a.m)) return ISLS_ERR_UNSUPPORTED;
    if (a.B == 0) return ISLS_OK;
    AdjP<T> p;
    p.B = a.B; p.N = a.N; p.n = a.n; p.m = a.m;
    p.A = View<T>(a.A); p.Bm = View<T>(a.Bm);
    p.c0x = (const T *)a.c0x; p.c0u = (const T *)a.c0u;
    p.lam = (T *)a.lam; p.gu = (T *)a.gu; p.gx0 = (T *)a.gx0; p.active = a.active;
    if (!dims_supported(a.n, a.m)) {
        const int tpw = kWave / (a.n + a.m);
        hipLaunchKernelGGL((adjoint_sweep_generic_kernel<T>), dim3((a.B + tpw - 1) / tpw), dim3(64), 0, s, p);
        return check_launch();
    }
#define CALL(NX_, NU_)                                                                                                     \
    {                                                                                                                      \
        constexpr int tpw = kWave / (NX_ + NU_);                                                                           \
        hipLaunchKernelGGL((adjoint_sweep_kernel<T, NX_, NU_, kAdjDepth>), dim3((a.B + tpw - 1) / tpw), dim3(64), 0, s, p); \
    }
    ISLS_DISPATCH_DIMS(a.n, a.m, CALL)
#undef CALL
    return check_launch();
}

}  // namespace isls

using namespace isls;

ISLS_ENTRY(adjoint_sweep, isls_adjoint_args, launch_adjoint, false)
