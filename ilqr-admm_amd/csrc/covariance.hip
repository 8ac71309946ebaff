// covariance.hip -- isls_cov_closed_loop_*: mean and covariance of the linearised closed loop of a batch of stage-local
// controllers (formulas and conventions: include/isls_hip.h).  The reference has no covariance code: it samples
// (get_trajectory_sls with noise) or, in its SLS form, constrains phi_u S0 phi_u'; this is the DP-form counterpart.
//
// An n x n forward recursion per trajectory, sequential in t and bound by latency, on the execution model of isls_common.hpp:
//   * one 64-lane wavefront per workgroup, TPW = 64 / n slots of G = n lanes, slot = trajectory (10 per wavefront at n = 6);
//   * lane i owns row i of Sig, row i of Phi = A + B K and d_i; the first m lanes of a slot also own row i of K Sig (the other
//     lanes evaluate row m-1 again and throw it away: no divergence);
//   * A_t, B_t, K_t, k_t, W_t are fetched cooperatively (lane i takes the elements i, i + n, ...) and unconditionally into a
//     register ring cov_depth() steps ahead, staged into the slot's LDS record and read back as broadcasts / own rows; xhat_t,
//     uhat_t and the bounds ride in the same ring entry, one word per lane;
//   * hand-offs use slot_sync(); three per step: (a) operands, Sig, d  ->  (b) Phi, K Sig K'  ->  (c) S = Phi Sig Phi' + W;
//   * a slot past P or an inactive one runs the recursion on trajectory min(b, P-1) and stores nothing; the lanes behind the last
//     slot work on a dump record; a wavefront without a single active trajectory returns at once;
//   * an absent k, W, xhat, uhat, dx0 is loaded from a valid dummy address (K or S0) and multiplied by a 0/1 mask where it is used;
//   * x_cov and u_cov leave lane-linearly from the symmetrised LDS images (n and ceil(m m / n) stores of n-word / m m-word runs
//     per slot and step); the vectors are n- / m-word runs per slot as the lanes hold them.
//
// Summation order (every multiply-add one fma through ff_mad, every sum ascending in its inner index, starting from 0 unless
// said otherwise; tests/cov_reference.py restates it):
//   Phi_ij  = A_ij, then + B_ir K_rj              r = 0..m-1
//   M_ij    = sum_k Phi_ik Sig_kj                 k = 0..n-1         (M = Phi Sig)
//   S_ij    = sum_k M_ik Phi_jk                   k = 0..n-1, then + mw W_ij as the last fused operation
//   Sig'_ij = 0.5 (S_ij + S_ji)
//   KS_rj   = sum_k K_rk Sig_kj                   k = 0..n-1
//   SU_rc   = sum_j KS_rj K_cj                    j = 0..n-1 ;  Su_rc = 0.5 (SU_rc + SU_cr)
//   ubar_r  = uhat_r + a,  a = mk k_r, then + K_rj d_j          j = 0..n-1
//   d'_i    = sum_j Phi_ij d_j                    j = 0..n-1, then + B_ir (mk k_r)   r = 0..m-1
//   xbar_i  = mx xhat_i + d_i (one fused operation)
// The diagonals: 0.5 (S_ii + S_ii) == S_ii exactly, so x_var / u_var are read from the unsymmetrised images.
#include "covariance.hpp"

namespace isls {

// Steps of operands in flight per lane: 4, or 2 where four ring entries (2n + 2m + 7 words each) would pass ~900 bytes per lane
// -- (9, 3) in double, whose ring of 4 alone took 496 of the 512 registers and spilled.  One wavefront per SIMD either way.
template <typename T>
constexpr int cov_depth(int n, int m) { return sizeof(T) * (2 * n + 2 * m + 7) * 4 > 900 ? 2 : 4; }

template <typename T>
struct CovP {
    int P, N;
    View<T> A, Bm, W, u_lo, u_hi, x_lo, x_hi;  // (absent W / bounds: S0 with strides 0)
    const T *K, *k, *xhat, *uhat, *dx0, *S0;
    int64_t K_sb, k_sb, xhat_sb, uhat_sb, dx0_sb, S0_sb;
    int64_t k_st, xhat_st, uhat_st;            // time strides (0 for a dummy)
    T mk, mw, mx, mu, md;                      // 0/1: k, W, xhat, uhat, dx0 present
    int has;                                   // bounds present: 1 u_lo, 2 u_hi, 4 x_lo, 8 x_hi
    const int32_t *active;
    T *x_mean, *u_mean, *x_var, *u_var, *x_cov, *u_cov, *p_u, *p_x;
};

__device__ __forceinline__ double cov_erfc(double x) { return erfc(x); }
__device__ __forceinline__ float cov_erfc(float x) { return erfcf(x); }

// Gaussian probability of lying outside [lo, hi]; var <= 0: the indicator of the mean lying outside
template <typename T>
__device__ __forceinline__ T prob_outside(T mu, T var, T lo, T hi, bool has_lo, bool has_hi)
{
    const T sd = sqrt(var > T(0) ? var : T(0));
    const bool point = !(sd > T(0));
    const T den = (point ? T(1) : sd) * T(1.4142135623730951);
    const T pl = T(0.5) * cov_erfc((mu - lo) / den), ph = T(0.5) * cov_erfc((hi - mu) / den);
    const T p = (has_lo ? pl : T(0)) + (has_hi ? ph : T(0));
    const T ind = ((has_lo && mu < lo) || (has_hi && mu > hi)) ? T(1) : T(0);
    return point ? ind : p;
}

// FULL: x_cov / u_cov are written; PROB: a bound is given and p_x / p_u are written
template <typename T, int NX, int NU, int D, bool FULL, bool PROB>
__global__ __launch_bounds__(64) void cov_closed_loop_kernel(CovP<T> p)
{
    static_assert(NU <= NX && NX <= kWave, "the first m lanes of a slot own the rows of K Sig");
    constexpr int G = NX, TPW = kWave / G;
    constexpr int JU = (NU * NU + G - 1) / G;
    // slot record (elements): A[NX][NX] | B[NX][NU] | K[NU][NX] | k[NU] | W[NX][NX] | Sig[NX][NX] | Phi[NX][NX] | S[NX][NX] |
    //                         SU[NU][NU] | Su[NU][NU] | d[NX] | dump
    constexpr int A_OFF = 0, B_OFF = A_OFF + NX * NX, K_OFF = B_OFF + NX * NU, KV_OFF = K_OFF + NU * NX, W_OFF = KV_OFF + NU,
                  SIG_OFF = W_OFF + NX * NX, PHI_OFF = SIG_OFF + NX * NX, S_OFF = PHI_OFF + NX * NX, SU_OFF = S_OFF + NX * NX,
                  SUS_OFF = SU_OFF + NU * NU, DV_OFF = SUS_OFF + NU * NU, DUMP_OFF = DV_OFF + NX;
    constexpr int SLOT = ((DUMP_OFF + 1) | 1);
    __shared__ T lds[(TPW + 1) * SLOT];                        // + one dump slot for the lanes behind the last slot

    const int lane = threadIdx.x;
    const int s = lane / G, i = lane - s * G;
    const bool inslot = s < TPW;
    const int b = blockIdx.x * TPW + (inslot ? s : 0);
    const bool valid = inslot && b < p.P && (p.active == nullptr || p.active[b] != 0);
    if (__builtin_amdgcn_ballot_w64(valid) == 0) return;       // (uniform) nothing to write from this wavefront
    const int bs = b < p.P ? b : p.P - 1;                      // the trajectory whose operands this slot reads
    const int N = p.N;
    const bool ul = i < NU;
    const int r = ul ? i : NU - 1;                             // the row of K Sig this lane evaluates
    T *rec = lds + (inslot ? s : TPW) * SLOT;

    // ---- load plan: per-lane pointers at step 0, uniform time strides ---------------------------------------
    const T *pA = p.A.at(bs, 0) + i, *pB = p.Bm.at(bs, 0) + i, *pW = p.W.at(bs, 0) + i;
    const T *pK = p.K + (int64_t)bs * p.K_sb + i, *pk = p.k + (int64_t)bs * p.k_sb + r;
    const T *pxh = p.xhat + (int64_t)bs * p.xhat_sb + i, *puh = p.uhat + (int64_t)bs * p.uhat_sb + r;
    const T *pul = p.u_lo.at(bs, 0) + r, *puu = p.u_hi.at(bs, 0) + r, *pxl = p.x_lo.at(bs, 0) + i, *pxu = p.x_hi.at(bs, 0) + i;
    const int64_t stA = p.A.st, stB = p.Bm.st, stW = p.W.st, stk = p.k_st, stxh = p.xhat_st, stuh = p.uhat_st;
    const int64_t stul = p.u_lo.st, stuu = p.u_hi.st, stxl = p.x_lo.st, stxu = p.x_hi.st;
    const T mk = p.mk, mw = p.mw, mx = p.mx, mu = p.mu;
    const bool h_ul = (p.has & 1) != 0, h_uu = (p.has & 2) != 0, h_xl = (p.has & 4) != 0, h_xu = (p.has & 8) != 0;

    struct Stage {
        T ra[NX], rw[NX], rb[NU], rk[NU];
        T kv, xh, uh, ulo, uhi, xlo, xhi;
    };
    auto fetch = [&](int t, Stage &g) {                        // (t clamped by the caller; nothing is computed on the results here)
#pragma unroll
        for (int j = 0; j < NX; ++j) g.ra[j] = pA[(int64_t)t * stA + G * j];
#pragma unroll
        for (int j = 0; j < NU; ++j) g.rb[j] = pB[(int64_t)t * stB + G * j];
#pragma unroll
        for (int j = 0; j < NU; ++j) g.rk[j] = pK[(int64_t)t * (NU * NX) + G * j];
#pragma unroll
        for (int j = 0; j < NX; ++j) g.rw[j] = pW[(int64_t)t * stW + G * j];
        g.kv = pk[(int64_t)t * stk];
        g.xh = pxh[(int64_t)t * stxh];
        g.uh = puh[(int64_t)t * stuh];
        if constexpr (PROB) {
            g.ulo = pul[(int64_t)t * stul];
            g.uhi = puu[(int64_t)t * stuu];
            g.xlo = pxl[(int64_t)t * stxl];
            g.xhi = pxu[(int64_t)t * stxu];
        }
    };

    // ---- outputs: this lane's words of step 0 --------------------------------------------------------------
    const int64_t bt0 = (int64_t)(valid ? b : 0) * N;
    T *oxm = p.x_mean + bt0 * NX + i, *oxv = p.x_var + bt0 * NX + i, *opx = p.p_x + bt0 * NX + i;
    T *oum = p.u_mean + bt0 * NU + r, *ouv = p.u_var + bt0 * NU + r, *opu = p.p_u + bt0 * NU + r;
    T *oxc = p.x_cov + bt0 * (NX * NX) + i, *ouc = p.u_cov + bt0 * (NU * NU) + i;
    const bool w_xm = valid && p.x_mean != nullptr, w_xv = valid && p.x_var != nullptr, w_px = valid && p.p_x != nullptr;
    const bool w_um = valid && ul && p.u_mean != nullptr, w_uv = valid && ul && p.u_var != nullptr, w_pu = valid && ul && p.p_u != nullptr;
    const bool w_xc = valid && p.x_cov != nullptr, w_uc = valid && p.u_cov != nullptr;

    // ---- Sig_0 = (S0 + S0')/2, d_0 = dx0 ---------------------------------------------------------------------
    T sig[NX], d;
    {
        const T *s0 = p.S0 + (int64_t)bs * p.S0_sb;
#pragma unroll
        for (int j = 0; j < NX; ++j) sig[j] = T(0.5) * (s0[i * NX + j] + s0[j * NX + i]);
        d = p.md * p.dx0[(int64_t)bs * p.dx0_sb + i];
    }
    Stage ring[D];
#pragma unroll
    for (int q = 0; q < D; ++q) {
        fetch(q < N ? q : N - 1, ring[q]);
        __builtin_amdgcn_sched_barrier(0);                     // the ring's first loads in consumption order
    }

    // Groups of D steps with the ring index a compile-time constant; the last group is padded with dead steps (t >= N: loads
    // clamped, Sig and d untouched, nothing stored), so the body exists once.
    for (int tb = 0; tb < N; tb += D) {
#pragma unroll
        for (int q = 0; q < D; ++q) {
            const int t = tb + q;
            const bool live = t < N;
            Stage &g = ring[q];
            // (a) stage the operands of step t and publish Sig_t (row i) and d_i
#pragma unroll
            for (int j = 0; j < NX; ++j) { rec[A_OFF + i + G * j] = g.ra[j]; rec[W_OFF + i + G * j] = g.rw[j]; }
#pragma unroll
            for (int j = 0; j < NU; ++j) { rec[B_OFF + i + G * j] = g.rb[j]; rec[K_OFF + i + G * j] = g.rk[j]; }
            rec[ul ? KV_OFF + i : DUMP_OFF] = mk * g.kv;
#pragma unroll
            for (int j = 0; j < NX; ++j) rec[SIG_OFF + i * NX + j] = sig[j];
            rec[DV_OFF + i] = d;
            const T xh = g.xh, uh = g.uh;
            T ulo, uhi, xlo, xhi;
            if constexpr (PROB) { ulo = g.ulo; uhi = g.uhi; xlo = g.xlo; xhi = g.xhi; }
            slot_sync();
            fetch(t + D < N ? t + D : N - 1, g);               // refill (clamped, unconditional)

            // x outputs of step t: the mean, the variance (the image's diagonal) and, lane-linearly, the image itself
            const T xbar = ff_mad(mx, xh, d);
            const T xvar = rec[SIG_OFF + i * NX + i];
            const int64_t ot = (int64_t)t;
            if (w_xm && live) oxm[ot * NX] = xbar;
            if (w_xv && live) oxv[ot * NX] = xvar;
            if constexpr (PROB) {
                const T px = prob_outside(xbar, xvar, xlo, xhi, h_xl, h_xu);
                if (w_px && live) opx[ot * NX] = px;
            }
            if constexpr (FULL) {
                T img[NX];
#pragma unroll
                for (int j = 0; j < NX; ++j) img[j] = rec[SIG_OFF + i + G * j];
#pragma unroll
                for (int j = 0; j < NX; ++j)
                    if (w_xc && live) oxc[ot * (NX * NX) + G * j] = img[j];
            }

            // (b) Phi row i, M = Phi Sig row i, K Sig K' row r, the means
            T Kt[NU][NX], phi[NX], dv[NX], kvm[NU], Brow[NU];
#pragma unroll
            for (int c = 0; c < NU; ++c) {
#pragma unroll
                for (int j = 0; j < NX; ++j) Kt[c][j] = rec[K_OFF + c * NX + j];
                kvm[c] = rec[KV_OFF + c];
                Brow[c] = rec[B_OFF + i * NU + c];
            }
#pragma unroll
            for (int j = 0; j < NX; ++j) { phi[j] = rec[A_OFF + i * NX + j]; dv[j] = rec[DV_OFF + j]; }
#pragma unroll
            for (int j = 0; j < NX; ++j) {
#pragma unroll
                for (int c = 0; c < NU; ++c) phi[j] = ff_mad(Brow[c], Kt[c][j], phi[j]);
                rec[PHI_OFF + i * NX + j] = phi[j];
            }
            T M[NX], ks[NX];
#pragma unroll
            for (int j = 0; j < NX; ++j) { M[j] = T(0); ks[j] = T(0); }
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                const T krk = rec[K_OFF + r * NX + k];
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    const T skj = rec[SIG_OFF + k * NX + j];
                    M[j] = ff_mad(phi[k], skj, M[j]);
                    ks[j] = ff_mad(krk, skj, ks[j]);
                }
            }
            T su[NU];
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                su[c] = T(0);
#pragma unroll
                for (int j = 0; j < NX; ++j) su[c] = ff_mad(ks[j], Kt[c][j], su[c]);
                rec[ul ? SU_OFF + r * NU + c : DUMP_OFF] = su[c];
            }
            T ua = rec[KV_OFF + r], dn = T(0);
#pragma unroll
            for (int j = 0; j < NX; ++j) {
                ua = ff_mad(rec[K_OFF + r * NX + j], dv[j], ua);
                dn = ff_mad(phi[j], dv[j], dn);
            }
#pragma unroll
            for (int c = 0; c < NU; ++c) dn = ff_mad(Brow[c], kvm[c], dn);
            const T ubar = ff_mad(mu, uh, ua);
            slot_sync();

            // (c) S = M Phi' + W row i; the control covariance symmetrised
            T S[NX];
#pragma unroll
            for (int j = 0; j < NX; ++j) {
                T acc = T(0);
#pragma unroll
                for (int k = 0; k < NX; ++k) acc = ff_mad(M[k], rec[PHI_OFF + j * NX + k], acc);
                S[j] = ff_mad(mw, rec[W_OFF + i * NX + j], acc);
                rec[S_OFF + i * NX + j] = S[j];
            }
            const T uvar = rec[SU_OFF + r * NU + r];
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                const T sus = T(0.5) * (su[c] + rec[SU_OFF + c * NU + r]);
                rec[ul ? SUS_OFF + r * NU + c : DUMP_OFF] = sus;
            }
            if (w_um && live) oum[ot * NU] = ubar;
            if (w_uv && live) ouv[ot * NU] = uvar;
            if constexpr (PROB) {
                const T pu = prob_outside(ubar, uvar, ulo, uhi, h_ul, h_uu);
                if (w_pu && live) opu[ot * NU] = pu;
            }
            slot_sync();
#pragma unroll
            for (int j = 0; j < NX; ++j) {
                const T sn = T(0.5) * (S[j] + rec[S_OFF + j * NX + i]);
                sig[j] = live ? sn : sig[j];
            }
            d = live ? dn : d;
            if constexpr (FULL) {
#pragma unroll
                for (int j = 0; j < JU; ++j) {
                    const int e = i + G * j;
                    const T v = rec[SUS_OFF + (e < NU * NU ? e : NU * NU - 1)];
                    if (w_uc && live && e < NU * NU) ouc[ot * (NU * NU) + G * j] = v;
                }
            }
        }
    }
}

template <typename T>
int launch_cov_closed_loop(const isls_cov_args &a, hipStream_t s)
{
    if (a.P < 0 || a.N < 1 || !a.A.p || !a.Bm.p || !a.K || !a.S0) return ISLS_ERR_ARG;
    if (a.K_sb < 0 || a.k_sb < 0 || a.xhat_sb < 0 || a.uhat_sb < 0 || a.dx0_sb < 0 || a.S0_sb < 0) return ISLS_ERR_ARG;
    for (const isls_view *v : {&a.A, &a.Bm, &a.W, &a.u_lo, &a.u_hi, &a.x_lo, &a.x_hi})
        if (v->sb < 0 || v->st < 0) return ISLS_ERR_ARG;
    if (!dims_supported(a.n, a.m)) return ISLS_ERR_UNSUPPORTED;          // run-time dimensions: not served
    if (a.P == 0) return ISLS_OK;

    CovP<T> p;
    p.P = a.P; p.N = a.N;
    p.A = View<T>(a.A); p.Bm = View<T>(a.Bm);
    const T *const S0 = (const T *)a.S0, *const K = (const T *)a.K;
    isls_view dummy = {a.S0, 0, 0};                                       // n n words: a valid address for every absent view
    p.W = View<T>(a.W.p ? a.W : dummy);
    p.u_lo = View<T>(a.u_lo.p ? a.u_lo : dummy); p.u_hi = View<T>(a.u_hi.p ? a.u_hi : dummy);
    p.x_lo = View<T>(a.x_lo.p ? a.x_lo : dummy); p.x_hi = View<T>(a.x_hi.p ? a.x_hi : dummy);
    p.has = (a.u_lo.p ? 1 : 0) | (a.u_hi.p ? 2 : 0) | (a.x_lo.p ? 4 : 0) | (a.x_hi.p ? 8 : 0);
    p.K = K; p.K_sb = a.K_sb; p.S0 = S0; p.S0_sb = a.S0_sb;
    p.k = a.k ? (const T *)a.k : K;       p.k_sb = a.k ? a.k_sb : 0;          p.k_st = a.k ? a.m : 0;       p.mk = a.k ? T(1) : T(0);
    p.xhat = a.xhat ? (const T *)a.xhat : S0; p.xhat_sb = a.xhat ? a.xhat_sb : 0; p.xhat_st = a.xhat ? a.n : 0; p.mx = a.xhat ? T(1) : T(0);
    p.uhat = a.uhat ? (const T *)a.uhat : K;  p.uhat_sb = a.uhat ? a.uhat_sb : 0; p.uhat_st = a.uhat ? a.m : 0; p.mu = a.uhat ? T(1) : T(0);
    p.dx0 = a.dx0 ? (const T *)a.dx0 : S0;    p.dx0_sb = a.dx0 ? a.dx0_sb : 0;    p.md = a.dx0 ? T(1) : T(0);
    p.mw = a.W.p ? T(1) : T(0);
    p.active = a.active;
    p.x_mean = (T *)a.x_mean; p.u_mean = (T *)a.u_mean; p.x_var = (T *)a.x_var; p.u_var = (T *)a.u_var;
    p.x_cov = (T *)a.x_cov; p.u_cov = (T *)a.u_cov; p.p_u = (T *)a.p_u; p.p_x = (T *)a.p_x;
    const bool full = a.x_cov || a.u_cov, prob = a.p_u || a.p_x;

#define LAUNCH(NX_, NU_, FULL_, PROB_) \
    hipLaunchKernelGGL((cov_closed_loop_kernel<T, NX_, NU_, cov_depth<T>(NX_, NU_), FULL_, PROB_>), dim3(grid), dim3(kWave), 0, s, p)
#define CALL(NX_, NU_)                                                  \
    {                                                                   \
        const int tpw = kWave / NX_;                                    \
        const unsigned grid = (unsigned)((a.P + tpw - 1) / tpw);        \
        if (full && prob) LAUNCH(NX_, NU_, true, true);                 \
        else if (full) LAUNCH(NX_, NU_, true, false);                   \
        else if (prob) LAUNCH(NX_, NU_, false, true);                   \
        else LAUNCH(NX_, NU_, false, false);                            \
    }
    ISLS_DISPATCH_DIMS(a.n, a.m, CALL)
#undef CALL
#undef LAUNCH
    return check_launch();
}
template int launch_cov_closed_loop<double>(const isls_cov_args &, hipStream_t);
template int launch_cov_closed_loop<float>(const isls_cov_args &, hipStream_t);

}  // namespace isls
