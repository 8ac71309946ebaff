// user_cost.hpp -- the device side of a user-written cost function (isls.costs.Custom), compiled at run time by hiprtc for gfx950
// (user_cost.hip builds the program).  The program text is
//     #include "user_cost_ad.hpp"
//     [namespace isls_user { <a user model's step<S, P>> }   #define ISLS_USER_NPAR <P>]      -- with a models.Custom
//     namespace isls_user_cost { <the user's stage<S, P>> }
//     #define ISLS_USER_COST_NPAR <P>
//     [#define ISLS_USER_COST_NTAB <W>]                                                       -- a cost with a per-step table
//     #include "user_cost.hpp"
// and its name expressions instantiate, for one (cost, model, dtype): every (JM, OCC) variant of rollout_kernel that the launch
// plan of a built-in model of the same dimensions can pick -- the built-ins' template as it is, with RoCost<..., true> below as
// its stage cost --, user_expand_kernel and user_cost_value_kernel.
// With ISLS_USER_COST_NTAB the user's stage takes the W words of step t as `const P *row` behind `par` (plain P: nothing is
// differentiated with respect to them); a source of the other form than its registration says does not compile.
// With ISLS_USER_COST_NCON = K > 0 the source also defines
//     template <typename S, typename P> __device__ void constraint(const S *x, const S *u, const P *par, [const P *row,] int t, int N, S *g);
// K path constraints g_i(x, u) <= 0.  ISLS_USER_COST_NTAB is then the width of the library's row, [user row (W) | lambda_0 ..
// lambda_{K-1} | mu] = W + K + 1 words (the user's functions take `row` only where W > 0), user_stage is the augmented Lagrangian
// of the stage (PHR form, below) and the program holds user_constraint_update_kernel, the multiplier and penalty update.
#pragma once

#ifndef ISLS_USER_COST_NPAR
#error "ISLS_USER_COST_NPAR: the parameter count of the user cost"
#endif

#ifndef ISLS_USER_COST_NTAB
#define ISLS_USER_COST_NTAB 0
#endif

#ifndef ISLS_USER_COST_NCON
#define ISLS_USER_COST_NCON 0
#endif

// words of the row that are the user's own (what `stage` and `constraint` see behind `row`)
#if ISLS_USER_COST_NCON > 0
#define ISLS_USER_COST_NROW (ISLS_USER_COST_NTAB - ISLS_USER_COST_NCON - 1)
#else
#define ISLS_USER_COST_NROW ISLS_USER_COST_NTAB
#endif

#ifdef ISLS_USER_NPAR
#include "user_model.hpp"
#else
#include "rollout_kernel.hpp"
#endif
#include "sampling.hpp"
#include "user_cost_ad.hpp"

namespace isls {

constexpr int kUserCostParWords = ISLS_USER_COST_NPAR > 0 ? ISLS_USER_COST_NPAR : 1;

template <typename T>
__device__ __forceinline__ void user_cost_par(const T *p, T (&par)[kUserCostParWords])
{
#pragma unroll
    for (int i = 0; i < kUserCostParWords; ++i) par[i] = i < ISLS_USER_COST_NPAR ? p[i] : T(0);
}

// the user's stage in the form its registration names: with the row of step t, or without
template <typename S, typename T>
__device__ __forceinline__ S user_plain_stage(const S *x, const S *u, const T *par, const T *row, int t, int N)
{
#if ISLS_USER_COST_NROW > 0
    return ::isls_user_cost::stage<S, T>(x, u, par, row, t, N);
#else
    return ::isls_user_cost::stage<S, T>(x, u, par, t, N);
#endif
}

#if ISLS_USER_COST_NCON > 0
// ... and the user's constraint, likewise
template <typename S, typename T>
__device__ __forceinline__ void user_constraint(const S *x, const S *u, const T *par, const T *row, int t, int N, S *g)
{
#if ISLS_USER_COST_NROW > 0
    ::isls_user_cost::constraint<S, T>(x, u, par, row, t, N, g);
#else
    ::isls_user_cost::constraint<S, T>(x, u, par, t, N, g);
#endif
}
#endif

// What every kernel of the program costs a step with.  With constraints: the augmented Lagrangian of the stage in the
// Powell-Hestenes-Rockafellar form, lambda_i = row[W + i], mu = row[W + K]:
//     h_i = lambda_i + mu g_i > 0 :  c += lambda_i g_i + mu / 2 g_i^2 ;   else :  c -= lambda_i^2 / (2 mu)   (0 where mu = 0)
// continuous with a continuous gradient, and exactly `stage` at lambda = 0, mu = 0.  The branch is taken on the value part of h
// (the AD contract's comparisons); only g carries derivatives, the row is plain T.
template <typename S, typename T>
__device__ __forceinline__ S user_stage(const S *x, const S *u, const T *par, const T *row, int t, int N)
{
#if ISLS_USER_COST_NCON > 0
    S c = user_plain_stage<S, T>(x, u, par, row, t, N);
    S g[ISLS_USER_COST_NCON];
    user_constraint<S, T>(x, u, par, row, t, N, g);
    const T mu = row[ISLS_USER_COST_NROW + ISLS_USER_COST_NCON];
#pragma unroll
    for (int i = 0; i < ISLS_USER_COST_NCON; ++i) {
        const T lam = row[ISLS_USER_COST_NROW + i];
        const S h = lam + mu * g[i];
        if (h > T(0)) c += lam * g[i] + (T(0.5) * mu) * (g[i] * g[i]);
        else c -= S(mu > T(0) ? lam * lam / (T(2) * mu) : T(0));
    }
    return c;
#else
    return user_plain_stage<S, T>(x, u, par, row, t, N);
#endif
}

// the stage cost of the line search: parameters in registers (no LDS words, so the launch plan is the built-ins'); the row of a
// table cost comes from the step's side record in LDS (rollout_kernel.hpp)
template <typename T, int NX, int NU>
struct RoCost<T, NX, NU, true> {
    static constexpr int NTAB = ISLS_USER_COST_NTAB;
    T par[kUserCostParWords];
    __device__ __forceinline__ void load(const T *p) { user_cost_par(p, par); }
    __device__ __forceinline__ T stage(const T (&x)[NX], const T (&u)[NU], const T *row, int t, int N) const
    {
        return user_stage<T, T>(x, u, par, row, t, N);
    }
};

// (Arguments of user_expand_kernel: UserExpP, rollout_kernel.hpp.)
// Gradient and Hessian of the stage cost along the nominal (isls_expand_args layout: Cxx [B,N,n,n], Cuu [B,N,m,m], Cux [B,N,m,n],
// c0x [B,N,n], c0u [B,N,m]; Cxx += 2 Qr, Cuu += 2 Rr).  One lane per (step, pair i <= j of [x; u]): it evaluates stage() on a
// hyper-dual number seeded with (e_i, e_j) and holds H_ij; the diagonal pairs also hold the gradient.  (All K (K + 1) / 2 second
// derivatives in one lane would be a dual state of (K + 1)(K + 2) / 2 words per scalar: 91 at n = 9, m = 3.)
// A workgroup takes S steps of one trajectory and walks their S * NP work items in sweeps of 64: up to 64 pairs (n + m <= 10)
// S = 64 / NP steps fit one sweep; (9, 3) has 78 pairs, and S = 4 steps there make 312 items = 5 sweeps with 8 idle lane slots
// (one step per workgroup would be 2 sweeps with 50 idle slots, i.e. 8 sweeps for the same four steps).
// The entries meet in LDS as full symmetric blocks and leave as contiguous runs, one per output array.
template <typename T, int NX, int NU>
__global__ __launch_bounds__(64) void user_expand_kernel(UserExpP<T> p)
{
    constexpr int K = NX + NU, NP = K * (K + 1) / 2, S = NP <= kWave ? kWave / NP : 4;
    __shared__ T tXX[S * NX * NX], tUU[S * NU * NU], tUX[S * NU * NX], tg[S * K];
    const int b = blockIdx.x / p.nbt, t0 = (blockIdx.x - b * p.nbt) * S;
    if (p.active && p.active[b] == 0) return;                 // uniform: the trajectory's arrays are left as they are
    const int N = p.N;
    const int64_t bN = (int64_t)b * N;
    T par[kUserCostParWords];
    user_cost_par(p.par + (int64_t)b * p.par_sb, par);
    const T *const tab = ISLS_USER_COST_NTAB > 0 ? p.tab + (int64_t)b * p.tab_sb : nullptr;   // row t: a plain global read
    using D = ad::Dual2<T>;
#pragma unroll 1
    for (int w = threadIdx.x; w < S * NP; w += kWave) {
        const int ts = w / NP, q = w - ts * NP, t = t0 + ts;
        if (t >= N) continue;
        // pair q -> (i, j), i <= j: row i of the upper triangle starts at i K - i (i - 1) / 2
        int i = 0;
#pragma unroll
        for (int r = 1; r < K; ++r) i += q >= r * K - r * (r - 1) / 2 ? 1 : 0;
        const int j = i + (q - (i * K - i * (i - 1) / 2));
        D x[NX], u[NU];
#pragma unroll
        for (int e = 0; e < NX; ++e) x[e] = D(p.xhat ? p.xhat[(bN + t) * NX + e] : T(0), e == i ? T(1) : T(0), e == j ? T(1) : T(0), T(0));
#pragma unroll
        for (int e = 0; e < NU; ++e)
            u[e] = D(p.uhat ? p.uhat[(bN + t) * NU + e] : T(0), NX + e == i ? T(1) : T(0), NX + e == j ? T(1) : T(0), T(0));
        const D c = user_stage<D, T>(x, u, par, tab + (int64_t)t * ISLS_USER_COST_NTAB, t, N);
        if (i == j) tg[ts * K + i] = c.a;
        if (j < NX) {                                          // i <= j < NX
            const T *Q = p.Qr.p ? p.Qr.at(b, t) : nullptr;
            tXX[(ts * NX + i) * NX + j] = c.ab + (Q ? T(2) * Q[i * NX + j] : T(0));
            if (i != j) tXX[(ts * NX + j) * NX + i] = c.ab + (Q ? T(2) * Q[j * NX + i] : T(0));
        } else if (i >= NX) {
            const int iu = i - NX, ju = j - NX;
            const T *R = p.Rr.p ? p.Rr.at(b, t) : nullptr;
            tUU[(ts * NU + iu) * NU + ju] = c.ab + (R ? T(2) * R[iu * NU + ju] : T(0));
            if (i != j) tUU[(ts * NU + ju) * NU + iu] = c.ab + (R ? T(2) * R[ju * NU + iu] : T(0));
        } else {                                               // i < NX <= j: H_ux[j - NX, i]
            tUX[(ts * NU + (j - NX)) * NX + i] = c.ab;
        }
    }
    __syncthreads();
    const int ns = N - t0 < S ? N - t0 : S;
    if (p.Cxx) {
        T *o = p.Cxx + (bN + t0) * NX * NX;
        for (int e = threadIdx.x; e < ns * NX * NX; e += kWave) o[e] = tXX[e];
    }
    if (p.Cuu) {
        T *o = p.Cuu + (bN + t0) * NU * NU;
        for (int e = threadIdx.x; e < ns * NU * NU; e += kWave) o[e] = tUU[e];
    }
    if (p.Cux) {
        T *o = p.Cux + (bN + t0) * NU * NX;
        for (int e = threadIdx.x; e < ns * NU * NX; e += kWave) o[e] = tUX[e];
    }
    for (int e = threadIdx.x; e < ns * K; e += kWave) {
        const int ts = e / K, i = e - ts * K;
        if (i < NX) p.c0x[(bN + t0 + ts) * NX + i] = tg[e];
        else p.c0u[(bN + t0 + ts) * NU + (i - NX)] = tg[e];
    }
}

// cost[r] = sum_t stage(x[r,t], u[r,t], par, t, N) for R trajectories, one lane each, summed in the order of the line search
// (isls_user_cost_value_*, and the nominal cost of an expansion); par [P] shared (par_sb = 0) or one row per trajectory; tab: the
// table of a cost that has one, [N][NTAB] shared (tab_sb = 0) or per trajectory
template <typename T, int NX, int NU>
__global__ __launch_bounds__(64) void user_cost_value_kernel(int R, int N, const T *par, int64_t par_sb, const T *x, const T *u, T *cost,
                                                             const int32_t *active, const T *tab, int64_t tab_sb)
{
    const int r = blockIdx.x * kWave + threadIdx.x;
    if (r >= R || (active && active[r] == 0)) return;
    RoCost<T, NX, NU, true> c;
    c.load(par + (int64_t)r * par_sb);
    const T *const trow = ISLS_USER_COST_NTAB > 0 ? tab + (int64_t)r * tab_sb : nullptr;
    T sum = T(0);
    for (int t = 0; t < N; ++t) {
        T xr[NX], ur[NU];
#pragma unroll
        for (int i = 0; i < NX; ++i) xr[i] = x ? x[((int64_t)r * N + t) * NX + i] : T(0);
#pragma unroll
        for (int i = 0; i < NU; ++i) ur[i] = u ? u[((int64_t)r * N + t) * NU + i] : T(0);
        sum += c.stage(xr, ur, trow + (int64_t)t * ISLS_USER_COST_NTAB, t, N);
    }
    cost[r] = sum;
}

#if ISLS_USER_COST_NCON > 0
// The multiplier and penalty update of the augmented Lagrangian (isls_user_constraint_update_*; arguments: UserConP,
// rollout_kernel.hpp).  One wavefront per trajectory, lanes stride over the steps.  Per step, in plain T: g = constraint(xhat_t,
// uhat_t), v_t = max_i max(0, g_i) (a NaN in g: +inf, and its lambda_i stays), g_out[b, t, :] = g where given, and with `update`
// lambda_i <- max(0, lambda_i + mu g_i) with the mu the trajectory came with.  Then viol[b] = max_t v_t by a wave reduction; with
// `update` and viol[b] > eta viol_prev[b] the lanes write mu <- min(phi mu, mu_max) into the last word of all N rows; viol_prev[b]
// <- viol[b].  No LDS, no atomics; a trajectory with active[b] == 0 is left untouched, viol and viol_prev included.
template <typename T, int NX, int NU>
__global__ __launch_bounds__(64) void user_constraint_update_kernel(UserConP<T> p)
{
    constexpr int K = ISLS_USER_COST_NCON, W = ISLS_USER_COST_NTAB, W0 = ISLS_USER_COST_NROW;
    const int b = blockIdx.x, N = p.N;
    if (b >= p.B || (p.active && p.active[b] == 0)) return;    // uniform
    T par[kUserCostParWords];
    user_cost_par(p.par + (int64_t)b * p.par_sb, par);
    T *const tab = p.tab + (int64_t)b * p.tab_sb;
    const int64_t bN = (int64_t)b * N;
    const T mu = tab[W0 + K];                                  // row 0's: every row of a trajectory holds the same mu
    T v = T(0);
#pragma unroll 1
    for (int t = threadIdx.x; t < N; t += kWave) {
        T x[NX], u[NU], g[K];
#pragma unroll
        for (int e = 0; e < NX; ++e) x[e] = p.xhat[(bN + t) * NX + e];
#pragma unroll
        for (int e = 0; e < NU; ++e) u[e] = p.uhat[(bN + t) * NU + e];
        T *const row = tab + (int64_t)t * W;
        user_constraint<T, T>(x, u, par, row, t, N, g);
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const T gi = g[i];
            if (gi != gi) {
                v = (T)__builtin_huge_val();
            } else {
                v = gi > v ? gi : v;
                if (p.update) {
                    const T nl = row[W0 + i] + mu * gi;
                    row[W0 + i] = nl > T(0) ? nl : T(0);
                }
            }
            if (p.g_out) p.g_out[(bN + t) * K + i] = gi;
        }
    }
    v = wave_max(v);
    if (p.update && v > p.eta * p.viol_prev[b]) {
        const T phimu = p.phi * mu, nm = phimu < p.mu_max ? phimu : p.mu_max;
#pragma unroll 1
        for (int t = threadIdx.x; t < N; t += kWave) tab[(int64_t)t * W + W0 + K] = nm;
    }
    if (threadIdx.x == 0) {
        p.viol[b] = v;
        p.viol_prev[b] = v;
    }
}
#endif

}  // namespace isls
