// monte_carlo.hpp -- Monte-Carlo validation of a batch of controllers (isls_mc_closed_loop_*): M noisy closed loops of every
// problem through its forward model and its own controller, statistics per problem, trajectories on request (kernel template;
// launched by monte_carlo.hip for the built-in models and by user_model.hip from a user model's run-time compiled module).
//
// Reference semantics: get_trajectory_sls (isls/isls_base.py:28-42, isls/sls_base.py:91-105), get_trajectory_dp / _batch
// (isls/sls_base.py:61-89): the control first, then the step, then the noise: x_{i+1} = f(x_i, u_i) + w_i.
//
// Mapping: lane = sample; a workgroup (64 or 128 lanes) holds samples of ONE problem and walks the horizon in tiles of TT steps.
//   per tile   : the nominal, k (form 0: the gains K_t too) and explicit noise of the tile's steps are fetched cooperatively in
//                contiguous runs into LDS and read back as broadcasts; every lane records x_t, u_t, w_t in its row of the LDS
//                stage.  Behind the tile's last step the stage leaves in runs of TT * n words per sample ([.,M,N,n] rows are
//                contiguous over the steps of a sample), and the statistics are taken FROM THE STAGE: one thread per (step,
//                coordinate) sweeps the samples' column, counts the bound violations, takes min / max and issues one atomic per
//                workgroup, step and coordinate.  They are therefore the statistics of the values written, bit for bit.
//   form 1     : (gather) dx_j = x_j - xhat_j goes to the caller's scratch `work` in a sample-fastest layout
//                [workgroup][N n][lanes]: a history read is one coalesced line per wavefront.  The rows of K of step i are staged
//                in double-buffered LDS chunks of kMcChunk entries by the whole workgroup; a lane never fetches K for itself.
//                Summation order of every u_i as in the reference: j ascending from 0, then + k_i, then + uhat_i.
//   lanes past M repeat the problem's last sample (same loads, same arithmetic) and are left out of the stores and statistics.
// The multiply-adds of u_i are explicit fma in both forms: a stage-local controller and its block-diagonal dense embedding give
// the same bits (a zero entry of K leaves the accumulator as it is).
#pragma once

#include "philox.hpp"
#include "rollout_kernel.hpp"

namespace isls {

constexpr int kMcTile = 8;         // steps per tile (halved by the launcher while a 64-lane stage does not fit: McPlan)
constexpr int kMcChunk = 128;      // entries of a row of K per LDS chunk (form 1)
constexpr int kMcModelRt = 98;     // template id: dense LTI pair with run-time dimensions n <= 16, m <= 8

template <typename T>
struct McP {
    int P, M, N, n, m;
    int tiles;                     // workgroups per problem
    int tt;                        // steps per tile
    int form;                      // 0: K [.,N,m,n]; 1: K [., N m, N n]
    int nw;                        // 1: the stage has a noise block (explicit w, drawn noise)
    const T *par;
    int64_t par_sb;
    const T *K, *k;
    int64_t K_sb, k_sb;
    const T *xhat, *uhat;          // nullable: 0
    int64_t xhat_sb, uhat_sb;
    const T *x0s, *x0, *x0_std;    // x0s [P,M,n], or x0 (+ x0_sb) and the nullable x0_std [n]
    int64_t x0_sb;
    const T *w, *noise_std;        // at most one
    unsigned long long seed;
    unsigned int problem0, sample0;
    View<T> u_lo, u_hi, x_lo, x_hi;
    int32_t *viol_u, *viol_x, *viol_any;
    T *u_min, *u_max, *x_min, *x_max;
    T *x_log, *u_log, *w_out, *x0_out;
    T *work;
};

// LDS plan of a launch, in words of T (host and device evaluate the same function)
struct McPlan {
    int sw;                        // words of a lane's stage row (odd: rows start in different banks)
    int o_nomx, o_nomu, o_k, o_K, o_kbuf, o_std, o_mdl, o_flag, words;
};
__host__ __device__ inline McPlan mc_plan(int n, int m, int tt, int nw, int form, int lanes, int mdlw)
{
    McPlan q;
    q.sw = (tt * (n + m + (nw ? n : 0))) | 1;
    int o = lanes * q.sw;
    q.o_nomx = o; o += tt * n;
    q.o_nomu = o; o += tt * m;
    q.o_k = o; o += tt * m;
    q.o_K = o; o += form == 0 ? tt * m * n : 0;
    q.o_kbuf = o; o += form == 1 ? 2 * m * kMcChunk : 0;
    q.o_std = o; o += 2 * n;
    q.o_mdl = o; o += mdlw + 1;
    q.o_flag = o; o += lanes;      // one word of T per lane, used as int32 (sizeof(T) >= 4)
    q.words = o;
    return q;
}

__device__ __forceinline__ double mc_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float mc_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// std * z and mean + std * z in fp64, rounded once to T, never contracted: an explicit replay of the values written to w_out /
// x0_out then takes the same bits through the same additions
template <typename T>
__device__ __forceinline__ T mc_scale(T sd, double z)
{
#pragma clang fp contract(off)
    const double v = (double)sd * z;
    return (T)v;
}
template <typename T>
__device__ __forceinline__ T mc_shift_scale(T mean, T sd, double z)
{
#pragma clang fp contract(off)
    const double v = (double)sd * z;
    const double s = (double)mean + v;
    return (T)s;
}
template <typename T>
__device__ __forceinline__ T mc_add(T a, T b)
{
#pragma clang fp contract(off)
    return a + b;
}

// the dense LTI pair at run-time dimensions: [A (n x n) | B (n x m)] as the caller lays them out, in LDS
template <typename T, int NX, int NU>
struct McLtiRt {
    const T *ab;
    int n, m;
    __device__ __forceinline__ void load(const T *par, T *lds, int c, int G)
    {
        for (int e = c; e < n * (n + m); e += G) lds[e] = par[e];
        ab = lds;
    }
    __device__ __forceinline__ void step(const T (&x)[NX], const T (&u)[NU], T (&xn)[NX]) const
    {
        const T *Bm = ab + n * n;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            T s = T(0), r = T(0);
            if (i < n) {
#pragma unroll
                for (int j = 0; j < NX; ++j)
                    if (j < n) s += ab[i * n + j] * x[j];
#pragma unroll
                for (int j = 0; j < NU; ++j)
                    if (j < m) r += Bm[i * m + j] * u[j];
            }
            xn[i] = s + r;
        }
    }
};

template <typename T, int NX, int NU, int MODEL>
struct McModel {
    using type = Model<T, NX, NU, MODEL>;
    static constexpr int LDS_WORDS = type::LDS_WORDS;
};
template <typename T, int NX, int NU>
struct McModel<T, NX, NU, kMcModelRt> {
    using type = McLtiRt<T, NX, NU>;
    static constexpr int LDS_WORDS = NX * (NX + NU);
};

template <typename T, int NX, int NU, int MODEL>
__global__ __launch_bounds__(128) void mc_closed_loop_kernel(McP<T> p)
{
    extern __shared__ __align__(16) unsigned char mc_smem[];
    constexpr bool RT = MODEL == kMcModelRt;
    T *lds = reinterpret_cast<T *>(mc_smem);
    const int n = RT ? p.n : NX, m = RT ? p.m : NU;
    const int N = p.N, TT = p.tt, lanes = blockDim.x, tid = threadIdx.x;
    const McPlan q = mc_plan(n, m, TT, p.nw, p.form, lanes, McModel<T, NX, NU, MODEL>::LDS_WORDS);
    const int pb = blockIdx.x / p.tiles, tile = blockIdx.x - pb * p.tiles;
    const int s_first = tile * lanes;
    const int nvalid = p.M - s_first < lanes ? p.M - s_first : lanes;
    const bool valid = tid < nvalid;
    const int s = s_first + (valid ? tid : nvalid - 1);        // lanes past M repeat the last sample
    const int64_t ps = (int64_t)pb * p.M + s;

    T *row = lds + tid * q.sw;
    const T *wrow = lds + (valid ? tid : nvalid - 1) * q.sw;    // explicit noise: the lanes past M read the last sample's
    const int OU = TT * n, OW = TT * (n + m);
    T *nomx = lds + q.o_nomx, *nomu = lds + q.o_nomu, *kk = lds + q.o_k, *Kt = lds + q.o_K, *kbuf = lds + q.o_kbuf;
    T *sdx = lds + q.o_std, *sdw = sdx + n;
    int32_t *flag = reinterpret_cast<int32_t *>(lds + q.o_flag);

    typename McModel<T, NX, NU, MODEL>::type mdl;
    if constexpr (RT) { mdl.n = n; mdl.m = m; }
    mdl.load(p.par + (int64_t)pb * p.par_sb, lds + q.o_mdl, tid, lanes);
    for (int e = tid; e < n; e += lanes) {
        sdx[e] = p.x0_std ? p.x0_std[e] : T(0);
        sdw[e] = p.noise_std ? p.noise_std[e] : T(0);
    }
    flag[tid] = 0;
    __syncthreads();

    const unsigned int c_sample = p.sample0 + (unsigned int)s, c_problem = p.problem0 + (unsigned int)pb;
    T x[NX], u[NU], xn[NX];
    // ---- initial state -------------------------------------------------------------------------------------------------------
    if (p.x0s) {
#pragma unroll
        for (int j = 0; j < NX; ++j) x[j] = j < n ? p.x0s[ps * n + j] : T(0);
    } else {
        const T *mean = p.x0 + (int64_t)pb * p.x0_sb;
#pragma unroll
        for (int g = 0; g < (NX + 3) / 4; ++g) {
            double z[4] = {0.0, 0.0, 0.0, 0.0};
            if (p.x0_std && 4 * g < n) philox::normal4(p.seed, c_sample, c_problem, 0xffffffffu, (unsigned int)g, z);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * g + e < NX) x[4 * g + e] = 4 * g + e < n ? mc_shift_scale(mean[4 * g + e], sdx[4 * g + e], z[e]) : T(0);
        }
    }
    if (p.x0_out && valid) {
#pragma unroll
        for (int j = 0; j < NX; ++j)
            if (j < n) p.x0_out[ps * n + j] = x[j];
    }

    const T *Kp = p.K + (int64_t)pb * p.K_sb, *kp = p.k + (int64_t)pb * p.k_sb;
    const int64_t Nn = (int64_t)N * n;
    T *hist = p.form == 1 ? p.work + (int64_t)blockIdx.x * Nn * lanes + tid : nullptr;

    int par = 0;                                              // K chunk buffer in use (form 1)
    for (int i0 = 0; i0 < N; i0 += TT) {
        const int cnt = N - i0 < TT ? N - i0 : TT;
        // ---- the tile's operands: contiguous runs, once per workgroup ----------------------------------------------------------
        for (int e = tid; e < cnt * n; e += lanes) nomx[e] = p.xhat ? p.xhat[(int64_t)pb * p.xhat_sb + (int64_t)i0 * n + e] : T(0);
        for (int e = tid; e < cnt * m; e += lanes) {
            nomu[e] = p.uhat ? p.uhat[(int64_t)pb * p.uhat_sb + (int64_t)i0 * m + e] : T(0);
            kk[e] = kp[(int64_t)i0 * m + e];
        }
        if (p.form == 0)
            for (int e = tid; e < cnt * m * n; e += lanes) Kt[e] = Kp[(int64_t)i0 * m * n + e];
        if (p.w) {
            const int run = cnt * n;
            for (int e = tid; e < nvalid * run; e += lanes) {
                const int sl = e / run, o = e - sl * run;
                lds[sl * q.sw + OW + o] = p.w[(((int64_t)pb * p.M + s_first + sl) * N + i0) * n + o];
            }
        }
        __syncthreads();

        for (int t = 0; t < cnt; ++t) {
            const int i = i0 + t;
            T dx[NX], acc[NU];
#pragma unroll
            for (int j = 0; j < NX; ++j) {
                dx[j] = T(0);
                if (j < n) {
                    dx[j] = x[j] - nomx[t * n + j];
                    row[t * n + j] = x[j];
                }
            }
#pragma unroll
            for (int r = 0; r < NU; ++r) acc[r] = T(0);
            if (p.form == 0) {
#pragma unroll
                for (int r = 0; r < NU; ++r)
                    if (r < m) {
#pragma unroll
                        for (int j = 0; j < NX; ++j)
                            if (j < n) acc[r] = mc_fma(dx[j], Kt[(t * m + r) * n + j], acc[r]);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < NX; ++j)
                    if (j < n) hist[((int64_t)i * n + j) * lanes] = dx[j];
                const int J = (i + 1) * n;
                const T *Krow = Kp + (int64_t)i * m * Nn;
                for (int j0 = 0; j0 < J; j0 += kMcChunk, par ^= 1) {   // `par` runs on over the steps: the buffers alternate
                    T *kb = kbuf + par * m * kMcChunk;
                    for (int e = tid; e < m * kMcChunk; e += lanes) {
                        const int r = e / kMcChunk, c = e - r * kMcChunk;
                        const int jj = j0 + c < J ? j0 + c : J - 1;
                        kb[e] = Krow[(int64_t)r * Nn + jj];
                    }
                    __syncthreads();
                    const int cn = J - j0 < kMcChunk ? J - j0 : kMcChunk;
                    const T *h = hist + (int64_t)j0 * lanes;
#pragma unroll 4
                    for (int c = 0; c < cn; ++c) {
                        const T hv = h[(int64_t)c * lanes];
#pragma unroll
                        for (int r = 0; r < NU; ++r)
                            if (r < m) acc[r] = mc_fma(hv, kb[r * kMcChunk + c], acc[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < NU; ++r) {
                u[r] = T(0);
                if (r < m) {
                    u[r] = mc_add(mc_add(acc[r], kk[t * m + r]), nomu[t * m + r]);
                    row[OU + t * m + r] = u[r];
                }
            }
            mdl.step(x, u, xn);
            if (p.nw) {
                if (p.w) {
#pragma unroll
                    for (int j = 0; j < NX; ++j) x[j] = j < n ? mc_add(xn[j], wrow[OW + t * n + j]) : T(0);
                } else {
#pragma unroll
                    for (int g = 0; g < (NX + 3) / 4; ++g) {
                        double z[4] = {0.0, 0.0, 0.0, 0.0};
                        if (4 * g < n) philox::normal4(p.seed, c_sample, c_problem, (unsigned int)i, (unsigned int)g, z);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int j = 4 * g + e;
                            if (j < NX) {
                                x[j] = T(0);
                                if (j < n) {
                                    const T wv = mc_scale(sdw[j], z[e]);
                                    row[OW + t * n + j] = wv;
                                    x[j] = mc_add(xn[j], wv);
                                }
                            }
                        }
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < NX; ++j) x[j] = xn[j];
            }
        }
        __syncthreads();

        // ---- the tile leaves: runs of cnt * n (cnt * m) words per sample -------------------------------------------------------
        const int64_t prow = (int64_t)pb * p.M + s_first;
        if (p.x_log) {
            const int run = cnt * n;
            for (int e = tid; e < nvalid * run; e += lanes) {
                const int sl = e / run, o = e - sl * run;
                p.x_log[((prow + sl) * N + i0) * n + o] = lds[sl * q.sw + o];
            }
        }
        if (p.u_log) {
            const int run = cnt * m;
            for (int e = tid; e < nvalid * run; e += lanes) {
                const int sl = e / run, o = e - sl * run;
                p.u_log[((prow + sl) * N + i0) * m + o] = lds[sl * q.sw + OU + o];
            }
        }
        if (p.w_out && p.nw) {
            const int run = cnt * n;
            for (int e = tid; e < nvalid * run; e += lanes) {
                const int sl = e / run, o = e - sl * run;
                p.w_out[((prow + sl) * N + i0) * n + o] = lds[sl * q.sw + OW + o];
            }
        }
        // ---- statistics of the stage: one thread per (step, coordinate) --------------------------------------------------------
        const bool st_x = p.viol_x || p.x_min || p.x_max || (p.viol_any && (p.x_lo.p || p.x_hi.p));
        const bool st_u = p.viol_u || p.u_min || p.u_max || (p.viol_any && (p.u_lo.p || p.u_hi.p));
        const int items_x = st_x ? cnt * n : 0, items = items_x + (st_u ? cnt * m : 0);
        for (int it = tid; it < items; it += lanes) {
            const bool isx = it < items_x;
            const int qi = isx ? it : it - items_x, d = isx ? n : m;
            const int tt = qi / d, c = qi - tt * d, off = isx ? qi : OU + qi, i = i0 + tt;
            const View<T> &vlo = isx ? p.x_lo : p.u_lo, &vhi = isx ? p.x_hi : p.u_hi;
            const T inf = (T)__builtin_huge_val();
            const T lo = vlo.p ? vlo.at(pb, i)[c] : -inf, hi = vhi.p ? vhi.at(pb, i)[c] : inf;
            T mn = inf, mx = -inf;
            int nv = 0;
            for (int sl = 0; sl < nvalid; ++sl) {
                const T v = lds[sl * q.sw + off];
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
                if (v < lo || v > hi) {
                    ++nv;
                    flag[sl] = 1;                                // several threads may store here at once: all store 1
                }
            }
            const int64_t o = ((int64_t)pb * N + i) * d + c;
            int32_t *viol = isx ? p.viol_x : p.viol_u;
            T *pmn = isx ? p.x_min : p.u_min, *pmx = isx ? p.x_max : p.u_max;
            if (viol && nv) atomicAdd(viol + o, nv);
            if (pmn) atomicMin(pmn + o, mn);
            if (pmx) atomicMax(pmx + o, mx);
        }
        __syncthreads();                                         // the stage is free for the next tile
    }
    __syncthreads();
    if (p.viol_any) {
        const unsigned long long bal = __ballot(valid && flag[tid] != 0);
        if ((tid & (kWave - 1)) == 0 && bal) atomicAdd(p.viol_any + pb, (int32_t)__popcll(bal));
    }
}

#ifndef __HIPCC_RTC__
// the Monte-Carlo closed loop of a user model (user_model.hip), from the model's own module
template <typename T>
int launch_mc_closed_loop_user(const McP<T> &p, int model, int grid, int lanes, size_t smem, hipStream_t s);
#endif

}  // namespace isls
