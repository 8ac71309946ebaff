// controller.hip -- the SLS controller K = PHI_U Phi_x^-1, k = (I - K Su) du of a batch of problems without dense transfer
// matrices or an inverse (replaces SLS.controller, isls/sls.py:235-242).
//
// Phi_x = Sw + Su PHI_U is UNIT block lower triangular when PHI_U is causal (block lower triangular), so K is block lower
// triangular and follows from two recursions:
//   column block s of Phi_x:  X_s[s] = I,  X_s[l+1] = A_l X_s[l] + B_l PHI_U[l, s]             (l = s .. N-2)
//   row block t of K:         K[t, s] = PHI_U[t, s] - sum_{l = s+1..t} K[t, l] X_s[l]           (s = t, t-1, .., 0)
//   feed-forward:             xd_0 = 0, xd_{t+1} = A_t xd_t + B_t du_t,  k_t = du_t - sum_{l <= t} K[t, l] xd_l
// Phase 1 (ctl_columns_kernel) runs the column recursions, one lane per (problem, column of Phi_x) plus one lane per problem
// for xd, into the caller's workspace.  Phase 2 (ctl_rows_kernel) is one workgroup per problem, one lane per row of K: the
// back-substitution descends over s for all rows at once, so the blocks X_s[s+1 .. N-1] it reads are staged in LDS once per
// s and read by every lane as broadcasts.  Rows are independent; a lane reads back the entries of its own K row that it wrote
// for larger s.  The same pass writes the zero blocks above the diagonal, computes k and flags a PHI_U that is not causal.
//
// Workspace of one problem (caller's dtype): the N(N-1)/2 blocks X_s[l], l > s, column block after column block
// (column s starts at block s(N-1) - s(s-1)/2, block (l, s) is entry l - s - 1 of it, each n x n row-major), then xd [N, n].
#include <algorithm>

#include "isls_common.hpp"

namespace isls {

namespace {

constexpr int kCtlColThreads = 256;
constexpr int kCtlRowThreads = 512;
constexpr int kCtlLdsBytes = 32768;      // X blocks staged per chunk of phase 2: 50 at n = 9, 113 at n = 6 (fp64)

__host__ __device__ inline int64_t ctl_col_off(int64_t s, int64_t N) { return s * (N - 1) - s * (s - 1) / 2; }

__host__ __device__ inline int64_t ctl_work_per_problem(int64_t N, int64_t n) { return N * (N - 1) / 2 * n * n + N * n; }

template <typename T>
struct CtlP {
    int B, N, m;
    View<T> A, Bm;
    const T *__restrict__ PHI;
    const T *__restrict__ du;
    T *K, *k, *work;
    int32_t *flags;
};

template <typename T, int NX>
__global__ __launch_bounds__(kCtlColThreads) void ctl_columns_kernel(CtlP<T> p)
{
    const int N = p.N, m = p.m;
    const int64_t cols = (int64_t)N * NX + 1;                   // N n columns of Phi_x, then xd
    const int64_t idx = (int64_t)blockIdx.x * kCtlColThreads + threadIdx.x;
    if (idx >= (int64_t)p.B * cols) return;
    const int b = (int)(idx / cols);
    const int c = (int)(idx - (int64_t)b * cols);
    const bool is_xd = c == N * NX;
    const int s = is_xd ? 0 : c / NX, j = is_xd ? 0 : c - s * NX;
    const int64_t ldp = (int64_t)N * NX;
    // input column of the recursion: column c of PHI_U (row stride N n) or du (stride 1), element l m + r at u[(l m + r) us]
    const int64_t us = is_xd ? 1 : ldp;
    const T *u = is_xd ? p.du + (int64_t)b * N * m : p.PHI + (int64_t)b * N * m * ldp + c;
    T *w = p.work + (int64_t)b * ctl_work_per_problem(N, NX);
    T *xd = w + (int64_t)N * (N - 1) / 2 * NX * NX;
    T *blk = w + ctl_col_off(s, N) * NX * NX + j;               // column j of block (s + 1, s)
    T x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = (!is_xd && i == j) ? T(1) : T(0);
    if (is_xd) {
#pragma unroll
        for (int i = 0; i < NX; ++i) xd[i] = T(0);
    }
    for (int l = s; l < N - 1; ++l) {
        const T *Al = p.A.at(b, l), *Bl = p.Bm.at(b, l);
        const T *ul = u + (int64_t)l * m * us;
        T xn[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            T acc = T(0);
#pragma unroll
            for (int q = 0; q < NX; ++q) acc += Al[i * NX + q] * x[q];
            xn[i] = acc;
        }
        for (int r = 0; r < m; ++r) {
            const T ur = ul[(int64_t)r * us];
#pragma unroll
            for (int i = 0; i < NX; ++i) xn[i] += Bl[i * m + r] * ur;
        }
        if (is_xd) {
#pragma unroll
            for (int i = 0; i < NX; ++i) xd[(int64_t)(l + 1) * NX + i] = xn[i];
        } else {
            T *o = blk + (int64_t)(l - s) * NX * NX;
#pragma unroll
            for (int i = 0; i < NX; ++i) o[i * NX] = xn[i];
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = xn[i];
    }
}

template <typename T, int NX>
__global__ __launch_bounds__(kCtlRowThreads) void ctl_rows_kernel(CtlP<T> p, int lc)
{
    extern __shared__ __align__(16) unsigned char ctl_smem[];
    T *xs = reinterpret_cast<T *>(ctl_smem);                    // lc staged blocks X_s[l]
    const int b = blockIdx.x;
    const int N = p.N, m = p.m, R = N * m;
    const int64_t ldp = (int64_t)N * NX;
    const T *w = p.work + (int64_t)b * ctl_work_per_problem(N, NX);
    const T *xd = w + (int64_t)N * (N - 1) / 2 * NX * NX;
    int flag = 0;
    for (int r0 = 0; r0 < R; r0 += blockDim.x) {                // passes over the rows (one when N m <= 512)
        const int row = r0 + threadIdx.x;
        const bool live = row < R;
        const int t = live ? row / m : -1;
        const T *ph = p.PHI + ((int64_t)b * R + (live ? row : 0)) * ldp;
        T *kr = p.K + ((int64_t)b * R + (live ? row : 0)) * ldp;
        for (int s = N - 1; s >= 0; --s) {
            T acc[NX];
#pragma unroll
            for (int j = 0; j < NX; ++j) acc[j] = T(0);
            const int nb = N - 1 - s;                           // blocks l = s+1 .. N-1 of column s
            const T *cs = w + ctl_col_off(s, N) * NX * NX;
            for (int l0 = 0; l0 < nb; l0 += lc) {
                const int cnt = min(lc, nb - l0);
                __syncthreads();                                // the previous chunk has been read
                for (int e = threadIdx.x; e < cnt * NX * NX; e += blockDim.x) xs[e] = cs[(int64_t)l0 * NX * NX + e];
                __syncthreads();
                const int qn = min(cnt, t - s - l0);            // l = s + 1 + l0 + q <= t
                for (int q = 0; q < qn; ++q) {
                    const T *kl = kr + (int64_t)(s + 1 + l0 + q) * NX;
                    const T *X = xs + q * NX * NX;
                    T kv[NX];
#pragma unroll
                    for (int i = 0; i < NX; ++i) kv[i] = kl[i];
#pragma unroll
                    for (int i = 0; i < NX; ++i) {
#pragma unroll
                        for (int j = 0; j < NX; ++j) acc[j] += kv[i] * X[i * NX + j];
                    }
                }
            }
            if (live) {
                T *ko = kr + (int64_t)s * NX;
                const T *po = ph + (int64_t)s * NX;
                if (t >= s) {
#pragma unroll
                    for (int j = 0; j < NX; ++j) ko[j] = po[j] - acc[j];
                } else {                                        // above the block diagonal: K is 0, PHI_U must be 0
#pragma unroll
                    for (int j = 0; j < NX; ++j) {
                        flag |= po[j] != T(0);
                        ko[j] = T(0);
                    }
                }
            }
        }
        if (live) {
            T acc = T(0);
            for (int l = 0; l <= t; ++l) {
#pragma unroll
                for (int i = 0; i < NX; ++i) acc += kr[(int64_t)l * NX + i] * xd[(int64_t)l * NX + i];
            }
            p.k[(int64_t)b * R + row] = p.du[(int64_t)b * R + row] - acc;
        }
    }
    flag = __syncthreads_or(flag);
    if (threadIdx.x == 0) p.flags[b] = flag ? ISLS_CTL_NOT_CAUSAL : 0;
}

template <typename T, int NX>
int launch_nx(const CtlP<T> &p, hipStream_t s)
{
    const int64_t lanes = (int64_t)p.B * ((int64_t)p.N * NX + 1);
    const int64_t g1 = (lanes + kCtlColThreads - 1) / kCtlColThreads;
    if (g1 > INT32_MAX) return ISLS_ERR_ARG;
    hipLaunchKernelGGL((ctl_columns_kernel<T, NX>), dim3((unsigned)g1), dim3(kCtlColThreads), 0, s, p);
    if (check_launch() != ISLS_OK) return ISLS_ERR_LAUNCH;
    const int R = p.N * p.m;
    const int threads = R >= kCtlRowThreads ? kCtlRowThreads : (R + kWave - 1) / kWave * kWave;
    const int per = (int)(kCtlLdsBytes / (NX * NX * sizeof(T)));
    const int lc = std::max(1, std::min(per, p.N - 1));
    hipLaunchKernelGGL((ctl_rows_kernel<T, NX>), dim3(p.B), dim3(threads), sizeof(T) * lc * NX * NX, s, p, lc);
    return check_launch();
}

}  // namespace

int64_t sls_controller_work_elems(int32_t B, int32_t N, int32_t n)
{
    if (B < 0 || N < 1 || n < 1) return 0;
    return (int64_t)B * ctl_work_per_problem(N, n);
}

template <typename T>
int launch_sls_controller(const isls_sls_controller_args &a, hipStream_t s)
{
    if (a.B < 0 || a.N < 1 || a.n < 1 || a.m < 1 || !a.A.p || !a.Bm.p || !a.PHI_U || !a.du || !a.K || !a.k || !a.flags || !a.work)
        return ISLS_ERR_ARG;
    if (a.n > 16 || a.m > 8) return ISLS_ERR_UNSUPPORTED;
    if ((int64_t)a.N * a.m > INT32_MAX / 2 || (int64_t)a.N * a.n > INT32_MAX / 2) return ISLS_ERR_ARG;
    if (a.B == 0) return ISLS_OK;
    CtlP<T> p;
    p.B = a.B; p.N = a.N; p.m = a.m;
    p.A = View<T>(a.A); p.Bm = View<T>(a.Bm);
    p.PHI = (const T *)a.PHI_U; p.du = (const T *)a.du;
    p.K = (T *)a.K; p.k = (T *)a.k; p.work = (T *)a.work; p.flags = a.flags;
    switch (a.n) {
#define CTL_CASE(NX_) \
    case NX_: return launch_nx<T, NX_>(p, s);
        CTL_CASE(1) CTL_CASE(2) CTL_CASE(3) CTL_CASE(4) CTL_CASE(5) CTL_CASE(6) CTL_CASE(7) CTL_CASE(8)
        CTL_CASE(9) CTL_CASE(10) CTL_CASE(11) CTL_CASE(12) CTL_CASE(13) CTL_CASE(14) CTL_CASE(15) CTL_CASE(16)
#undef CTL_CASE
        default: return ISLS_ERR_UNSUPPORTED;
    }
}
template int launch_sls_controller<double>(const isls_sls_controller_args &, hipStream_t);
template int launch_sls_controller<float>(const isls_sls_controller_args &, hipStream_t);

}  // namespace isls
