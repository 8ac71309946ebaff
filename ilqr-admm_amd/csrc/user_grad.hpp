// user_grad.hpp -- the parameter and table directions of the nominal's cost for a user-written model or cost
// (isls_user_{model,cost}_grad_*; user_rtc.hip builds the program, user_grad.hip launches it).  The program text is that of the
// source's own program with this header in the place of user_model.hpp / user_cost.hpp, and its one name expression is
// user_model_grad_kernel or user_cost_grad_kernel.  It is a program of its own because it instantiates the source with
// S = P = ad::Dual<T, 1>: x, u are constants and ONE word d of [par | row] carries the derivative, so what the source does with
// `par` and `row` must keep to the S contract of user_model_ad.hpp too.  The source's other programs take P = T as before.
//
// One wavefront per (trajectory, direction d); the lanes stride over the steps.  A table direction writes its value per step; a
// parameter direction sums its lane's steps in order and the wave reduces (wave_sum: a fixed butterfly, no atomics).
#pragma once

#if !defined(__HIPCC_RTC__)
#include "isls_common.hpp"                                   // the host side (user_grad.hip): the argument block only
#elif defined(ISLS_USER_COST_NPAR)
#include "user_cost.hpp"
#else
#include "user_model.hpp"
#endif

namespace isls {

template <typename T>
struct UserGradP {
    int B, N;
    int d0, nd;                    // the directions of this launch: d0 .. d0 + nd - 1 of [par (P) | row (W)]
    const T *par;
    int64_t par_sb;
    const T *tab;                  // the cost's table (a model's rows lie behind its parameters)
    int64_t tab_sb;
    const T *xhat, *uhat;
    const T *lam;                  // [B,N,n] (model)
    T *g_par, *g_tab;              // [B,P], [B,N,W]
    const int32_t *active;
};

#ifdef __HIPCC_RTC__
// v = the cnt words at src (zero beyond) as constants, but word d - first with derivative 1
template <typename T, int NW>
__device__ __forceinline__ void grad_seed(ad::Dual<T, 1> (&v)[NW], const T *src, int cnt, int first, int d)
{
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        v[i] = ad::Dual<T, 1>(i < cnt ? src[i] : T(0));
        v[i].d[0] = first + i == d && i < cnt ? T(1) : T(0);
    }
}

#ifndef ISLS_USER_COST_NPAR
template <typename T, int NX, int NU>
__global__ __launch_bounds__(64) void user_model_grad_kernel(UserGradP<T> p)
{
    constexpr int P = ISLS_USER_NPAR, W = ISLS_USER_MODEL_NTAB, WW = W > 0 ? W : 1;
    using D = ad::Dual<T, 1>;
    const int b = blockIdx.x / p.nd, d = p.d0 + (blockIdx.x - b * p.nd), N = p.N;
    if (p.active && p.active[b] == 0) return;                 // uniform
    const int64_t bN = (int64_t)b * N;
    const T *pp = p.par + (int64_t)b * p.par_sb;
    D par[kUserParWords];
    grad_seed<T, kUserParWords>(par, pp, P, 0, d);
    T acc = T(0);
#pragma unroll 1
    for (int t = threadIdx.x; t < N; t += kWave) {
        T g = T(0);                                            // step N-1 steps nothing: its row's derivative is exactly 0
        if (t < N - 1) {
            D x[NX], u[NU], xn[NX], row[WW];
#pragma unroll
            for (int i = 0; i < NX; ++i) x[i] = D(p.xhat[(bN + t) * NX + i]);
#pragma unroll
            for (int i = 0; i < NU; ++i) u[i] = D(p.uhat[(bN + t) * NU + i]);
            grad_seed<T, WW>(row, pp + P + (int64_t)t * W, W, P, d);
            user_step<D, D>(x, u, par, row, xn);
#pragma unroll
            for (int i = 0; i < NX; ++i) g += p.lam[(bN + t + 1) * NX + i] * xn[i].d[0];
        }
        if (d >= P) p.g_tab[(bN + t) * W + (d - P)] = g;
        else acc += g;
    }
    if (d < P) {
        acc = wave_sum(acc);
        if (threadIdx.x == 0) p.g_par[(int64_t)b * P + d] = acc;
    }
}
#else
template <typename T, int NX, int NU>
__global__ __launch_bounds__(64) void user_cost_grad_kernel(UserGradP<T> p)
{
    // NTAB: the words of a row as the table holds them (with constraints: the multipliers and mu behind the user's W = NROW)
    constexpr int P = ISLS_USER_COST_NPAR, NTAB = ISLS_USER_COST_NTAB, W = ISLS_USER_COST_NROW, WW = NTAB > 0 ? NTAB : 1;
    using D = ad::Dual<T, 1>;
    const int b = blockIdx.x / p.nd, d = p.d0 + (blockIdx.x - b * p.nd), N = p.N;
    if (p.active && p.active[b] == 0) return;                 // uniform
    const int64_t bN = (int64_t)b * N;
    D par[kUserCostParWords];
    grad_seed<T, kUserCostParWords>(par, p.par + (int64_t)b * p.par_sb, P, 0, d);
    const T *const tab = NTAB > 0 ? p.tab + (int64_t)b * p.tab_sb : nullptr;
    T acc = T(0);
#pragma unroll 1
    for (int t = threadIdx.x; t < N; t += kWave) {
        D x[NX], u[NU], row[WW];
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = D(p.xhat[(bN + t) * NX + i]);
#pragma unroll
        for (int i = 0; i < NU; ++i) u[i] = D(p.uhat[(bN + t) * NU + i]);
        grad_seed<T, WW>(row, tab + (int64_t)t * NTAB, NTAB, P, d);   // d < P + W: a multiplier or mu is never seeded
        const T g = user_stage<D, D>(x, u, par, row, t, N).d[0];
        if (d >= P) p.g_tab[(bN + t) * W + (d - P)] = g;
        else acc += g;
    }
    if (d < P) {
        acc = wave_sum(acc);
        if (threadIdx.x == 0) p.g_par[(int64_t)b * P + d] = acc;
    }
}
#endif
#endif  // __HIPCC_RTC__

}  // namespace isls
