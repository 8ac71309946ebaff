// user_model.hpp -- the device side of a user-written forward model (isls.models.Custom), compiled at run time by hiprtc for
// gfx950 (user_model.hip builds the program).  The program text is
//     #include "user_model_ad.hpp"
//     namespace isls_user { <the user's step<S, P>> }
//     #define ISLS_USER_NPAR <P>
//     [#define ISLS_USER_MODEL_NTAB <W>]                                                      -- a model with a per-step table
//     #include "user_model.hpp"
// and its name expressions instantiate, for one (n, m, dtype): every (JM, OCC) variant of rollout_kernel that the launch plan
// of a built-in model of the same dimensions can pick, user_linearize_kernel, dense_closed_loop_kernel, user_step_kernel and
// mc_closed_loop_kernel (monte_carlo.hpp) and mpc_step_kernel (mpc.hpp).
// The rollout kernel is the built-ins' template as it is: only Model<T, NX, NU, ISLS_MODEL_USER> below is new.
// With ISLS_USER_MODEL_NTAB the user's step takes the W words of step t as `const P *row` behind `par` (plain P: nothing is
// differentiated with respect to them); a source of the other form than its registration says does not compile.  The table lies
// behind the parameters in the buffer the launch names as the model's: [par (P) | row 0 | ... | row N-1] (isls_hip.h).
#pragma once

#include "monte_carlo.hpp"
#include "mpc.hpp"
#include "rollout_kernel.hpp"
#include "sampling.hpp"
#include "user_model_ad.hpp"

#ifndef ISLS_USER_NPAR
#error "ISLS_USER_NPAR: the parameter count of the user model"
#endif

#ifndef ISLS_USER_MODEL_NTAB
#define ISLS_USER_MODEL_NTAB 0
#endif

namespace isls {

constexpr int kUserParWords = ISLS_USER_NPAR > 0 ? ISLS_USER_NPAR : 1;

// the user's step in the form its registration names: with the row of step t, or without
template <typename S, typename T>
__device__ __forceinline__ void user_step(const S *x, const S *u, const T *par, const T *row, S *xn)
{
#if ISLS_USER_MODEL_NTAB > 0
    ::isls_user::step<S, T>(x, u, par, row, xn);
#else
    ::isls_user::step<S, T>(x, u, par, xn);
#endif
}

// the user's parameters live in registers, like the nonlinear built-ins' (no LDS words: the same launch plan as theirs).  A table
// model keeps the address of row 0 (behind the parameters): step() is the step with that row -- the plant of isls_mpc_step --,
// step_row() the step with the row the kernel hands it (model_step_row / model_step_at, rollout_kernel.hpp)
template <typename T, int NX, int NU>
struct Model<T, NX, NU, ISLS_MODEL_USER> {
    static constexpr int LDS_WORDS = 0;
    T par[kUserParWords];
    const T *rows;
    __device__ __forceinline__ void load(const T *p, T *, int, int)
    {
#pragma unroll
        for (int i = 0; i < kUserParWords; ++i) par[i] = i < ISLS_USER_NPAR ? p[i] : T(0);
        rows = p + ISLS_USER_NPAR;
    }
    __device__ __forceinline__ void step(const T (&x)[NX], const T (&u)[NU], T (&xn)[NX]) const
    {
        user_step<T, T>(x, u, par, rows, xn);
    }
    __device__ __forceinline__ void step_row(const T (&x)[NX], const T (&u)[NU], const T *row, T (&xn)[NX]) const
    {
        user_step<T, T>(x, u, par, row, xn);
    }
};

// A_t, B_t of the user model along the nominal (isls_linearize_args layout: A [B,N,n,n], Bm [B,N,n,m]).  One lane per (step,
// input direction): lane j of a step evaluates step() on Dual<T, 1> seeded with e_j and holds column j of [A_t B_t].
// (Dual<T, n+m> in one lane per step would carry (n+m+1)(2n+m) words of dual state: 273 doubles at n = 9, m = 3, past the
// register file.)  The columns meet in LDS, and the wavefront writes its S = 64 / (n+m) steps out as two contiguous runs.
// (Arguments: UserLinP, rollout_kernel.hpp.)
template <typename T, int NX, int NU>
__global__ __launch_bounds__(64) void user_linearize_kernel(UserLinP<T> p)
{
    constexpr int K = NX + NU, S = kWave / K;
    __shared__ T tA[S * NX * NX], tB[S * NX * NU];
    const int b = blockIdx.x / p.nbt, t0 = (blockIdx.x - b * p.nbt) * S;
    if (p.active && p.active[b] == 0) return;                 // uniform: the trajectory's A, Bm are left as they are
    const int N = p.N, ts = threadIdx.x / K, j = threadIdx.x - ts * K, t = t0 + ts;
    const int64_t bN = (int64_t)b * N;
    if (ts < S && t < N) {
        using D = ad::Dual<T, 1>;
        const T *pp = p.par + (int64_t)b * p.par_sb;
        T par[kUserParWords];
#pragma unroll
        for (int i = 0; i < kUserParWords; ++i) par[i] = i < ISLS_USER_NPAR ? pp[i] : T(0);
        D x[NX], u[NU], xn[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            x[i] = D(p.xhat[(bN + t) * NX + i]);
            x[i].d[0] = i == j ? T(1) : T(0);
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            u[i] = D(p.uhat[(bN + t) * NU + i]);
            u[i].d[0] = NX + i == j ? T(1) : T(0);
        }
        user_step<D, T>(x, u, par, pp + ISLS_USER_NPAR + (int64_t)t * ISLS_USER_MODEL_NTAB, xn);   // row t: a plain global read
        if (j < NX) {
#pragma unroll
            for (int i = 0; i < NX; ++i) tA[(ts * NX + i) * NX + j] = xn[i].d[0];
        } else {
#pragma unroll
            for (int i = 0; i < NX; ++i) tB[(ts * NX + i) * NU + (j - NX)] = xn[i].d[0];
        }
    }
    __syncthreads();
    const int ns = N - t0 < S ? N - t0 : S;
    T *A = p.A + (bN + t0) * NX * NX, *Bm = p.Bm + (bN + t0) * NX * NU;
    for (int e = threadIdx.x; e < ns * NX * NX; e += kWave) A[e] = tA[e];
    for (int e = threadIdx.x; e < ns * NX * NU; e += kWave) Bm[e] = tB[e];
}

// xn[r] = f(x[r], u[r]) row by row (Custom.__call__); par [P] shared (par_sb = 0) or one row per state row
template <typename T, int NX, int NU>
__global__ __launch_bounds__(64) void user_step_kernel(int R, const T *par, int64_t par_sb, const T *x, const T *u, T *xn)
{
    const int r = blockIdx.x * kWave + threadIdx.x;
    if (r >= R) return;
    Model<T, NX, NU, ISLS_MODEL_USER> mdl;
    mdl.load(par + (int64_t)r * par_sb, nullptr, 0, 1);
    T xr[NX], ur[NU], yr[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xr[i] = x[(int64_t)r * NX + i];
#pragma unroll
    for (int i = 0; i < NU; ++i) ur[i] = u[(int64_t)r * NU + i];
    mdl.step(xr, ur, yr);
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[(int64_t)r * NX + i] = yr[i];
}

// The same for a table model (isls_user_model_step_tab_*; the last name expression of such a model's program): the state rows
// come in runs of `run` rows per parameter block [par | rows] (par_sb per run), and row r steps with table row tix[r], or
// (tix == NULL) with its place r % run in its run.
template <typename T, int NX, int NU>
__global__ __launch_bounds__(64) void user_step_tab_kernel(int R, const T *par, int64_t par_sb, const T *x, const T *u, T *xn, int run,
                                                           const int32_t *tix)
{
    const int r = blockIdx.x * kWave + threadIdx.x;
    if (r >= R) return;
    Model<T, NX, NU, ISLS_MODEL_USER> mdl;
    mdl.load(par + (int64_t)(r / run) * par_sb, nullptr, 0, 1);
    const int t = tix ? tix[r] : r % run;
    T xr[NX], ur[NU], yr[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xr[i] = x[(int64_t)r * NX + i];
#pragma unroll
    for (int i = 0; i < NU; ++i) ur[i] = u[(int64_t)r * NU + i];
    model_step_at<ISLS_MODEL_USER>(mdl, xr, ur, t, yr);
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[(int64_t)r * NX + i] = yr[i];
}

}  // namespace isls
