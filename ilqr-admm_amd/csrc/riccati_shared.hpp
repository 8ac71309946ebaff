// riccati_shared.hpp -- what the Riccati gain pass (riccati_gain_kernel.hpp) and the feed-forward passes on its records and arrays
// (riccati_ff.hip, riccati_ffrec.hip, ff_segments.hip) compute alike, written once.  Register arithmetic only: which words are
// read in which batch, the hand-offs and where the stores of a step go stay with each kernel (the one read of global memory here
// is the mask, in the K-piece plan ahead of a kernel's step loop).
#pragma once
#include "isls_common.hpp"

namespace isls {

// ---- k = -Quu^-1 qu from the cached factor -----------------------------------------------------------------------------------
// mode (a kernel's template argument or its run-time p.mode): ISLS_SOLVE_CHOL -- two triangular solves with the strict upper
// part U of the factor and its reciprocal pivots rd; ISLS_SOLVE_INV -- a product with inv = Quu^-1.  FX: every multiply-add one
// fused operation (ff_mad; the twin recursion below).  PLUS_ZERO: the negation is 0 - x, so that qu = +0 gives k = +0 (the
// one-hand-off pass emits k[N-1] = 0 this way).
template <int NU, bool FX = false, bool PLUS_ZERO = false, typename T>
__device__ __forceinline__ void k_from_factor(int mode, const T (&U)[NU][NU], const T (&rd)[NU], const T (&inv)[NU][NU], const T (&qu)[NU],
                                              T (&kt)[NU])
{
    T x[NU];
    if (mode == ISLS_SOLVE_CHOL) {
        chol_solve_mad<NU, FX>(U, rd, qu, x);
    } else {
#pragma unroll
        for (int r = 0; r < NU; ++r) {
            T acc = T(0);
#pragma unroll
            for (int c = 0; c < NU; ++c) acc = ff_mad<FX>(inv[r][c], qu[c], acc);
            x[r] = acc;
        }
    }
#pragma unroll
    for (int r = 0; r < NU; ++r) kt[r] = PLUS_ZERO ? T(0) - x[r] : -x[r];
}
// ... from the m x m block as the records and the fac array hold it: U with rd on its diagonal, or Quu^-1
template <int NU, bool FX = false, bool PLUS_ZERO = false, typename T>
__device__ __forceinline__ void k_from_factor(int mode, const T (&fac)[NU][NU], const T (&qu)[NU], T (&kt)[NU])
{
    T rd[NU];
#pragma unroll
    for (int r = 0; r < NU; ++r) rd[r] = fac[r][r];
    k_from_factor<NU, FX, PLUS_ZERO>(mode, fac, rd, fac, qu, kt);   // (the solves never read U's diagonal)
}

// ---- the v / k recursion of the first feed-forward pass ------------------------------------------------------------------------
//     c_i = c0_i + sum_j (2 row)_j d_j      qu_r = cu_r + sum_k [A B][k, n + r] v_k
//     v_i = (cx_i + sum_k Phi[k, i] v_k) + sum_r K[r, i] cu_r,      Phi[:, i] = A[:, i] + B K[:, i]
// Every sum starts from zero and takes its terms in index order; FX as for ff_mad.  The structured gain pass (FF, LIN = 1) and the
// stand-in pass on the kept table (riccati_ffrec2_kernel, FU) both evaluate these with FX = true on the double integrator's
// column below, so the k of a call is the same bit for bit whichever of them ran.
template <int N, bool FX, typename T>
__device__ __forceinline__ T ff_dot(const T (&a)[N], const T (&b)[N])
{
    T acc = T(0);
#pragma unroll
    for (int j = 0; j < N; ++j) acc = ff_mad<FX>(a[j], b[j], acc);
    return acc;
}
template <int N, bool FX, typename T>
__device__ __forceinline__ T ff_cost_grad(T c0, const T (&row2)[N], const T (&d)[N]) { return c0 + ff_dot<N, FX>(row2, d); }
template <int NX, bool FX, typename T>
__device__ __forceinline__ T ff_qu(T ci, const T (&col)[NX], const T (&v)[NX]) { return ci + ff_dot<NX, FX>(col, v); }
template <int NX, int NU, bool FX, typename T>
__device__ __forceinline__ T ff_vi(T ci, const T (&phc)[NX], const T (&v)[NX], const T (&Kc)[NU], const T (&cu)[NU])
{
    const T acc = ff_dot<NX, FX>(phc, v), kcu = ff_dot<NU, FX>(Kc, cu);
    return (ci + acc) + kcu;
}
// The double integrator, [A B] = [I aI b0 I; 0 I b1 I] (n = 2 d, m = d): column i of it has at most two entries, c1 at row r1 and c2
// at row r2 >= r1 -- x-lane i < d: e_i; x-lane i >= d: a e_{i-d} + e_i; u-lane r: b0 e_r + b1 e_{d+r} -- and colc is the column with
// its exact zeros.
template <int NX, int NU, typename T>
__device__ __forceinline__ void di_column(bool xl, int i, int iu, T a, T b0, T b1, T &c1, int &r1, T &c2, int &r2, T (&colc)[NX])
{
    if (xl && i < NU) { c1 = T(1); r1 = i; c2 = T(0); r2 = i; }
    else if (xl) { c1 = a; r1 = i - NU; c2 = T(1); r2 = i; }
    else { c1 = b0; r1 = iu; c2 = b1; r2 = NU + iu; }
#pragma unroll
    for (int k = 0; k < NX; ++k) colc[k] = (k == r1) ? c1 : ((k == r2) ? c2 : T(0));
}
// Phi[k, i] = A[k, i] + (row k of B) . K[:, i]: that row has one entry
template <int NU, typename T>
__device__ __forceinline__ T di_phi(int k, T a_ki, T b0, T b1, const T (&Kc)[NU]) { return ff_mad<true>(k < NU ? b0 : b1, Kc[k % NU], a_ki); }

// ---- the K blocks' way out of a wavefront's slots --------------------------------------------------------------------------------
// Lane-linear plan: piece e = lane + 64 j of the TPW slots' K blocks, KU pieces of PW words to a block of KW words.  kso: where the
// piece is in LDS (slot stride `stride`, the block at k_off of a slot); kgo: its word in the K array at t = 0.  Pieces of slots
// without a trajectory go where the shadowed trajectory's (bsh) go -- same words; lanes past the last piece repeat piece 0 of the
// shadowed slot ssh.
template <int JK, int KU, int PW, int KW, int JA>
__device__ __forceinline__ void k_piece_plan(int lane, int bx, int TPW, int stride, int k_off, int ssh, int bsh, int B, const int32_t *active, int N,
                                             int (&kso)[JA], int64_t (&kgo)[JA])
{
#pragma unroll
    for (int j = 0; j < JK; ++j) {
        const int e = lane + kWave * j, in = e < TPW * KU;
        const int sl = in ? e / KU : ssh, pc = in ? e - (e / KU) * KU : 0;
        const int bk = bx * TPW + sl;
        const bool ok = bk < B && (active == nullptr || active[bk] != 0);
        kso[j] = sl * stride + k_off + pc * PW;
        kgo[j] = (int64_t)(ok ? bk : bsh) * N * KW + pc * PW;
    }
}

}  // namespace isls
