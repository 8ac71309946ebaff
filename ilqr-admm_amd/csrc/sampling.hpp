// sampling.hpp -- one sampling round about the nominal of every problem of a batch (isls_sample_nominal_*): S open-loop rollouts
// per problem with controls drawn about uhat, their costs, and the path-integral update of the nominal with the fallback to the
// best sample (kernel templates; launched by sampling.hip for the built-in families and, for a user model and / or a user cost,
// from the run-time compiled module of the (model, cost) pair).  include/isls_hip.h states the formulas.
//
// The reference has no sampling code: it refines the nominal it is handed (isls/isls.py:336-374).  This is one round of model
// predictive path integral control (Williams et al., "Information theoretic MPC", ICRA 2017) with the cost of the problem itself.
//
// sample_cost_kernel    grid B x ceil(S / 64), one wavefront per workgroup, lane = sample.  The state, the control and the
//                       running cost of a sample live in registers for the whole horizon; uhat_t, sigma, the clip, the model's
//                       parameters, the via point or the table row of step t have wave-uniform addresses (every lane of the
//                       wavefront reads the same words); the normals come from Philox in the lane, ceil(m / 4) blocks per step;
//                       one store per lane, costs[b, s], NaN written as +inf.  Lanes s >= S repeat the arithmetic and store nothing.
// sample_update_kernel  one wavefront per problem.  Minimum and FIRST arg-min of costs[b, :] (a lane takes s = lane, lane + 64, ...
//                       ascending, then a fixed butterfly that prefers the smaller index on a tie), the weights and their sums the
//                       same way: bitwise repeatable, and independent of B and of the launch's other problems.  The weighted sum of
//                       the clipped draws is formed by REGENERATING them, kSmpTile steps per sweep over the samples (one weight per
//                       sample and sweep): the generator is counter-based, a [B, S, N, m] array of noise never exists.  u_new goes
//                       to LDS [N][m], is rolled out and costed (x_t overwrites xhat_t as it goes: only xhat_0 is an input); where
//                       its cost is not below the minimum the best sample's controls are regenerated into the same LDS rows and
//                       rolled out instead.  uhat leaves LDS in one contiguous sweep.
// The cost of a rollout is the line search's (rollout_kernel.hpp): the user's stage through RoCost<>, the line search's own code,
// in a program that carries a user cost; else the pseudo-Huber terms (ISLS_MODEL_TASSA) or the via-point terms, restated below
// (ro_phuber_* / ro_via_*) in the line search's order -- state terms step by step, control terms step by step, one addition
// of the two at the end.
#pragma once

#include "monte_carlo.hpp"

namespace isls {

constexpr int kSmpTile = 4;        // steps per sweep over the samples in the update (weights are formed once per sweep)

template <typename T>
struct SampleP {
    int B, N, S, chunks;           // chunks = ceil(S / 64): workgroups per problem of the cost kernel
    int cost_model;
    const T *par;
    int64_t par_sb;
    T *xhat, *uhat;                // [B,N,n], [B,N,m]: in / out
    const T *Qtab, *ztab;          // via-point tables; a user cost's table travels in ztab / ztab_sb (isls_rollout_args)
    int64_t Qtab_sb, ztab_sb;
    const int32_t *seq;
    T u_std;
    const T *cpar;                 // ISLS_COST_PHUBER [m + 4 n] shared; a user cost's [P] / [B,P]
    int64_t cpar_sb;
    const T *sigma;                // [m] / [B,m]
    int64_t sigma_sb;
    const T *u_lo, *u_hi;          // [m], each nullable
    T temperature;
    unsigned long long seed;
    unsigned int problem0;
    const int32_t *problem_ids;    // nullable: the draws' problem counter of problem b (else problem0 + b)
    const int32_t *active;
    T *costs;                      // [B,S]
    T *cost_before, *cost_after, *cost_best, *ess;   // per problem, element b at b * stat_sb (each nullable)
    int32_t *took_best;
    int64_t stat_sb;
};

template <typename T>
__device__ __forceinline__ T smp_sub(T a, T b)
{
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double smp_tiny(double) { return 2.2250738585072014e-308; }
__device__ __forceinline__ float smp_tiny(float) { return 1.17549435e-38f; }

// sigma, the clip and the counters of one problem's draws
template <typename T, int NU>
struct SampleDraw {
    T sig[NU], lo[NU], hi[NU];
    unsigned long long seed;
    unsigned int problem;
    __device__ __forceinline__ void load(const SampleP<T> &p, int b)
    {
        const T inf = (T)__builtin_huge_val();
        const T *sg = p.sigma + (int64_t)b * p.sigma_sb;
#pragma unroll
        for (int r = 0; r < NU; ++r) {
            sig[r] = sg[r];
            lo[r] = p.u_lo ? p.u_lo[r] : -inf;
            hi[r] = p.u_hi ? p.u_hi[r] : inf;
        }
        seed = p.seed;
        problem = p.problem_ids ? (unsigned int)p.problem_ids[b] : p.problem0 + (unsigned int)b;
    }
    // u = clip(uh + eps), e = u - uh with eps = sigma o z(seed, problem, sample, step) (sample 0: eps = 0); the product in fp64,
    // rounded once to T, sum and difference never contracted (monte_carlo.hpp's rule for drawn noise)
    __device__ __forceinline__ void controls(unsigned int sample, unsigned int step, const T (&uh)[NU], T (&u)[NU], T (&e)[NU]) const
    {
#pragma unroll
        for (int g = 0; g < (NU + 3) / 4; ++g) {
            double z[4];
            philox::normal4(seed, sample, problem, step, (unsigned int)g, z);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int r = 4 * g + h;
                if (r < NU) {
                    const T eps = sample == 0u ? T(0) : mc_scale(sig[r], z[h]);
                    T v = mc_add(uh[r], eps);
                    v = v < lo[r] ? lo[r] : v;
                    v = v > hi[r] ? hi[r] : v;
                    u[r] = v;
                    e[r] = smp_sub(v, uh[r]);
                }
            }
        }
    }
};

// ---- the stage terms of the built-in costs, as the step of the line search writes them (rollout_kernel.hpp, ISLS_RO_STEP): each adds
// its terms to the running sum it is handed, in that order, and returns it.  They are a second text of those terms: the line
// search keeps its own inside the step macro, and calling these from there changed the instruction text of 120 of its
// instantiations, so that kernel is left as it is and tests/test_sampling_gpu.py holds the two texts together.
// sum_j c_j ph(x_j, p_j), ph(x, p) = sqrt(x^2 + p^2) - p   (ISLS_COST_PHUBER: the running and the final state term)
template <typename T, int NX>
__device__ __forceinline__ T ro_phuber_x(const T (&x)[NX], const T (&c)[NX], const T (&p)[NX], T sum)
{
#pragma unroll
    for (int j = 0; j < NX; ++j) sum += c[j] * (sqrt(x[j] * x[j] + p[j] * p[j]) - p[j]);
    return sum;
}
// sum_r c_r u_r^2   (ISLS_COST_PHUBER)
template <typename T, int NU>
__device__ __forceinline__ T ro_phuber_u(const T (&u)[NU], const T (&c)[NU], T sum)
{
#pragma unroll
    for (int r = 0; r < NU; ++r) sum += c[r] * (u[r] * u[r]);
    return sum;
}
// (x - z)' Q (x - z)   (ISLS_COST_VIA: Q [NX][NX], z [NX] of the step's via point)
template <typename T, int NX>
__device__ __forceinline__ T ro_via_x(const T (&x)[NX], const T *Q, const T *z, T sum)
{
    T dq[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) dq[j] = x[j] - z[j];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        T acc = T(0);
#pragma unroll
        for (int j = 0; j < NX; ++j) acc += Q[i * NX + j] * dq[j];
        sum += dq[i] * acc;
    }
    return sum;
}
// u_std |u|^2   (ISLS_COST_VIA)
template <typename T, int NU>
__device__ __forceinline__ T ro_via_u(const T (&u)[NU], T ustd, T sum)
{
#pragma unroll
    for (int r = 0; r < NU; ++r) sum += u[r] * (ustd * u[r]);
    return sum;
}

// the running cost of one rollout: the line search's terms in the line search's order
template <typename T, int NX, int NU, int MODEL>
struct SampleCost {
    static constexpr bool UC = kRoUserCost;
    static constexpr bool kHasPH = !UC && MODEL == ISLS_MODEL_TASSA;
    static constexpr int NTAB = RoCost<T, NX, NU, UC>::NTAB;
    RoCost<T, NX, NU, UC> ucost;
    const T *Qtab, *ztab, *tab;
    const int32_t *seq;
    T ustd;
    bool phuber;
    T ph_cu[NU], ph_cx[NX], ph_px[NX], ph_cf[NX], ph_pf[NX];
    T cst, cu;
    __device__ __forceinline__ void load(const SampleP<T> &p, int b)
    {
        Qtab = p.Qtab + (int64_t)b * p.Qtab_sb;
        ztab = p.ztab + (int64_t)b * p.ztab_sb;
        tab = ztab;                                            // a user cost's table: rows read with plain global loads
        seq = p.seq;
        ustd = p.u_std;
        if constexpr (UC) ucost.load(p.cpar + (int64_t)b * p.cpar_sb);
        phuber = kHasPH && p.cost_model == ISLS_COST_PHUBER;
#pragma unroll
        for (int r = 0; r < NU; ++r) ph_cu[r] = phuber ? p.cpar[r] : T(0);
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            ph_cx[j] = phuber ? p.cpar[NU + j] : T(0);
            ph_px[j] = phuber ? p.cpar[NU + NX + j] : T(1);
            ph_cf[j] = phuber ? p.cpar[NU + 2 * NX + j] : T(0);
            ph_pf[j] = phuber ? p.cpar[NU + 3 * NX + j] : T(1);
        }
    }
    __device__ __forceinline__ void reset() { cst = T(0); cu = T(0); }
    __device__ __forceinline__ void add(const T (&x)[NX], const T (&u)[NU], int t, int N)
    {
        if constexpr (UC) {
            cst += ucost.stage(x, u, tab + (int64_t)t * NTAB, t, N);
        } else if (kHasPH && phuber) {
            cst = ro_phuber_x<T, NX>(x, ph_cx, ph_px, cst);
            if (t == N - 1) cst = ro_phuber_x<T, NX>(x, ph_cf, ph_pf, cst);
            cu = ro_phuber_u<T, NU>(u, ph_cu, cu);
        } else {                                               // every step, also where Q_t == 0 (no q_nonzero hint here: isls_hip.h)
            const int sq = seq[t];
            cst = ro_via_x<T, NX>(x, Qtab + (int64_t)sq * NX * NX, ztab + (int64_t)sq * NX, cst);
            cu = ro_via_u<T, NU>(u, ustd, cu);
        }
    }
    __device__ __forceinline__ T total() const { return cst + cu; }
};

// model words in LDS, padded to an even count (the rows of u behind them stay 16-byte aligned in double)
__host__ __device__ constexpr int smp_mdl_words(int mdlw) { return mdlw + (mdlw & 1); }

template <typename T, int NX, int NU, int MODEL>
__global__ __launch_bounds__(64) void sample_cost_kernel(SampleP<T> p)
{
    extern __shared__ __align__(16) unsigned char smp_smem[];
    const int lane = threadIdx.x, N = p.N;
    const int b = blockIdx.x / p.chunks, ch = blockIdx.x - b * p.chunks;
    if (p.active && p.active[b] == 0) return;                  // uniform
    const int s = ch * kWave + lane;
    Model<T, NX, NU, MODEL> mdl;
    mdl.load(p.par + (int64_t)b * p.par_sb, reinterpret_cast<T *>(smp_smem), lane, kWave);
    __syncthreads();
    SampleDraw<T, NU> draw;
    draw.load(p, b);
    SampleCost<T, NX, NU, MODEL> cost;
    cost.load(p, b);
    cost.reset();
    const T *xh = p.xhat + (int64_t)b * N * NX, *uhp = p.uhat + (int64_t)b * N * NU;
    T x[NX], xn[NX], u[NU], e[NU], uh[NU];
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = xh[j];
    for (int t = 0; t < N; ++t) {
#pragma unroll
        for (int r = 0; r < NU; ++r) uh[r] = uhp[(int64_t)t * NU + r];
        draw.controls((unsigned int)s, (unsigned int)t, uh, u, e);
        cost.add(x, u, t, N);
        if (t < N - 1) {
            model_step_at<MODEL>(mdl, x, u, t, xn);
#pragma unroll
            for (int j = 0; j < NX; ++j) x[j] = xn[j];
        }
    }
    const T c = cost.total();
    if (s < p.S) p.costs[(int64_t)b * p.S + s] = c != c ? (T)__builtin_huge_val() : c;
}

// the rollout of the controls in LDS from xhat_0, costed; lane 0 writes x_t over xhat_t for t >= 1
template <typename T, int NX, int NU, int MODEL>
__device__ __forceinline__ T smp_rollout(const Model<T, NX, NU, MODEL> &mdl, SampleCost<T, NX, NU, MODEL> &cost, const T *ubuf, T *xh, int N,
                                         int lane)
{
    T x[NX], xn[NX], u[NU];
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = xh[j];
    cost.reset();
    for (int t = 0; t < N; ++t) {
#pragma unroll
        for (int r = 0; r < NU; ++r) u[r] = ubuf[t * NU + r];
        if (lane == 0 && t > 0) {
#pragma unroll
            for (int j = 0; j < NX; ++j) xh[(int64_t)t * NX + j] = x[j];
        }
        cost.add(x, u, t, N);
        if (t < N - 1) {
            model_step_at<MODEL>(mdl, x, u, t, xn);
#pragma unroll
            for (int j = 0; j < NX; ++j) x[j] = xn[j];
        }
    }
    return cost.total();
}

template <typename T>
__device__ __forceinline__ T smp_weight(T c, T cmin, T lam)
{
    return exp(-(c - cmin) / lam);
}

template <typename T, int NX, int NU, int MODEL>
__global__ __launch_bounds__(64) void sample_update_kernel(SampleP<T> p)
{
    extern __shared__ __align__(16) unsigned char smp_smem[];
    constexpr int MDLW = smp_mdl_words(Model<T, NX, NU, MODEL>::LDS_WORDS), TT = kSmpTile;
    const int lane = threadIdx.x, N = p.N, S = p.S, b = blockIdx.x;
    if (p.active && p.active[b] == 0) return;                  // uniform: the trajectory and its statistics stay as they are
    T *ubuf = reinterpret_cast<T *>(smp_smem) + MDLW;          // [N][NU]
    const T *cs = p.costs + (int64_t)b * S;
    const T inf = (T)__builtin_huge_val();
    const int64_t so = (int64_t)b * p.stat_sb;

    // ---- minimum and first arg-min ---------------------------------------------------------------------------------------------
    T cmin = inf;
    int imin = 0x7fffffff;
    for (int s = lane; s < S; s += kWave) {
        const T c = cs[s];
        if (c < cmin) { cmin = c; imin = s; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T oc = __shfl_xor(cmin, o, kWave);
        const int oi = __shfl_xor(imin, o, kWave);
        if (oc < cmin || (oc == cmin && oi < imin)) { cmin = oc; imin = oi; }
    }
    const T c0 = cs[0];
    if (!(c0 < inf) || !(c0 > -inf)) {                         // the nominal's own rollout has no finite cost: nothing to start from
        if (lane == 0) {
            if (p.cost_before) p.cost_before[so] = c0;
            if (p.cost_after) p.cost_after[so] = c0;
            if (p.cost_best) p.cost_best[so] = cmin;
            if (p.ess) p.ess[so] = T(0);
            if (p.took_best) p.took_best[so] = 0;
        }
        return;
    }

    // ---- weights: w_s = exp(-(S_s - Smin) / (temperature max(Smin, tiny))), normalised ----------------------------------------------
    const T tiny = smp_tiny(T(0));
    const T lam = p.temperature * (cmin > tiny ? cmin : tiny);
    T wsum = T(0), w2 = T(0);                                  // ess = 1 / sum (w / wsum)^2 = wsum^2 / sum w^2: one pass
    for (int s = lane; s < S; s += kWave) {
        const T w = smp_weight(cs[s], cmin, lam);
        wsum += w;
        w2 += w * w;
    }
    wsum = wave_sum(wsum);
    w2 = wave_sum(w2);

    Model<T, NX, NU, MODEL> mdl;
    mdl.load(p.par + (int64_t)b * p.par_sb, reinterpret_cast<T *>(smp_smem), lane, kWave);
    SampleDraw<T, NU> draw;
    draw.load(p, b);
    SampleCost<T, NX, NU, MODEL> cost;
    cost.load(p, b);
    T *xh = p.xhat + (int64_t)b * N * NX, *uhp = p.uhat + (int64_t)b * N * NU;

    // ---- u_new_t = uhat_t + sum_s w_s (clip(uhat_t + eps_st) - uhat_t), the draws regenerated ------------------------------------
    for (int t0 = 0; t0 < N; t0 += TT) {
        T uh[TT][NU], acc[TT][NU];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            const int t = t0 + tt < N ? t0 + tt : N - 1;
#pragma unroll
            for (int r = 0; r < NU; ++r) {
                uh[tt][r] = uhp[(int64_t)t * NU + r];
                acc[tt][r] = T(0);
            }
        }
        for (int s = lane; s < S; s += kWave) {
            const T wn = smp_weight(cs[s], cmin, lam) / wsum;
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                if (t0 + tt < N) {                             // uniform
                    T u[NU], e[NU];
                    draw.controls((unsigned int)s, (unsigned int)(t0 + tt), uh[tt], u, e);
#pragma unroll
                    for (int r = 0; r < NU; ++r) acc[tt][r] += wn * e[r];
                }
            }
        }
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
            for (int r = 0; r < NU; ++r) {
                const T a = wave_sum(acc[tt][r]);
                if (lane == 0 && t0 + tt < N) ubuf[(t0 + tt) * NU + r] = mc_add(uh[tt][r], a);
            }
        }
    }
    __syncthreads();

    // ---- roll u_new out; where it does not beat the best sample, that sample's controls instead ---------------------------------
    const T cnew = smp_rollout<T, NX, NU, MODEL>(mdl, cost, ubuf, xh, N, lane);
    const bool take_best = !(cnew < cmin);
    if (take_best) {                                           // uniform
        __syncthreads();
        for (int t = lane; t < N; t += kWave) {
            T uh[NU], u[NU], e[NU];
#pragma unroll
            for (int r = 0; r < NU; ++r) uh[r] = uhp[(int64_t)t * NU + r];
            draw.controls((unsigned int)imin, (unsigned int)t, uh, u, e);
#pragma unroll
            for (int r = 0; r < NU; ++r) ubuf[t * NU + r] = u[r];
        }
        __syncthreads();
        smp_rollout<T, NX, NU, MODEL>(mdl, cost, ubuf, xh, N, lane);
    }
    __syncthreads();
    for (int e = lane; e < N * NU; e += kWave) uhp[e] = ubuf[e];
    if (lane == 0) {
        if (p.cost_before) p.cost_before[so] = c0;
        if (p.cost_after) p.cost_after[so] = take_best ? cmin : cnew;
        if (p.cost_best) p.cost_best[so] = cmin;
        if (p.ess) p.ess[so] = (wsum * wsum) / w2;
        if (p.took_best) p.took_best[so] = take_best ? 1 : 0;
    }
}

// ---- the closed-loop round (isls_sample_nominal_fb_*): every sample's control is uhat_t + G_t (x_t - xhat_t) + eps_t ------------------
// The same mapping, counters and cost code as above; what differs:
//   * xa_t = xhat[b,t] (NX words) and G_t = K[b,t] (NU NX words) are read per step at wave-uniform addresses, like uhat_t: the gain
//     table is never held in registers.
//   * the update sums the DRAWN noise, d_t = sum_s w_s eps[s,t] (the realised deviation of a closed-loop sample depends on its state
//     and could not be regenerated without its rollout; the draw can), kSmpTile steps per sweep as above.
//   * both rollouts of the update need the anchor xa_t while the new states are produced: the new states [N][NX] and controls [N][NU]
//     stay in LDS until the choice is made, xhat / uhat are read only until then and leave LDS in two contiguous sweeps.
// These are kernels of their own with an argument block of their own: the open-loop kernels and SampleP<> are as they were.
template <typename T>
struct SampleFbP {
    SampleP<T> p;
    const T *K;                    // [.,N,m,n]
    int64_t K_sb;                  // 0 (shared by the batch) or N m n
};

// eps = sigma o z(seed, problem, sample, step) (sample 0: eps = 0): the draw of SampleDraw<>::controls, unclipped
template <typename T, int NU>
__device__ __forceinline__ void smp_noise(const SampleDraw<T, NU> &draw, unsigned int sample, unsigned int step, T (&eps)[NU])
{
#pragma unroll
    for (int g = 0; g < (NU + 3) / 4; ++g) {
        double z[4];
        philox::normal4(draw.seed, sample, draw.problem, step, (unsigned int)g, z);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int r = 4 * g + h;
            if (r < NU) eps[r] = sample == 0u ? T(0) : mc_scale(draw.sig[r], z[h]);
        }
    }
}

// v = base + G (x - xa): the product summed over the state index ascending, then added to base
template <typename T, int NX, int NU>
__device__ __forceinline__ void smp_feedback(const T (&base)[NU], const T *G, const T *xa, const T (&x)[NX], T (&v)[NU])
{
    T dx[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) dx[j] = x[j] - xa[j];
#pragma unroll
    for (int r = 0; r < NU; ++r) {
        T acc = T(0);
#pragma unroll
        for (int j = 0; j < NX; ++j) acc += G[r * NX + j] * dx[j];
        v[r] = base[r] + acc;
    }
}

// u = clip(v + eps), the sum never contracted (the rule for drawn noise)
template <typename T, int NU>
__device__ __forceinline__ void smp_clip_add(const SampleDraw<T, NU> &draw, const T (&v)[NU], const T (&eps)[NU], T (&u)[NU])
{
#pragma unroll
    for (int r = 0; r < NU; ++r) {
        T w = mc_add(v[r], eps[r]);
        w = w < draw.lo[r] ? draw.lo[r] : w;
        w = w > draw.hi[r] ? draw.hi[r] : w;
        u[r] = w;
    }
}

template <typename T, int NX, int NU, int MODEL>
__global__ __launch_bounds__(64) void sample_cost_fb_kernel(SampleFbP<T> q)
{
    extern __shared__ __align__(16) unsigned char smp_smem[];
    const SampleP<T> &p = q.p;
    const int lane = threadIdx.x, N = p.N;
    const int b = blockIdx.x / p.chunks, ch = blockIdx.x - b * p.chunks;
    if (p.active && p.active[b] == 0) return;                  // uniform
    const int s = ch * kWave + lane;
    Model<T, NX, NU, MODEL> mdl;
    mdl.load(p.par + (int64_t)b * p.par_sb, reinterpret_cast<T *>(smp_smem), lane, kWave);
    __syncthreads();
    SampleDraw<T, NU> draw;
    draw.load(p, b);
    SampleCost<T, NX, NU, MODEL> cost;
    cost.load(p, b);
    cost.reset();
    const T *xh = p.xhat + (int64_t)b * N * NX, *uhp = p.uhat + (int64_t)b * N * NU;
    const T *G = q.K + (int64_t)b * q.K_sb;
    T x[NX], xn[NX], u[NU], v[NU], eps[NU], uh[NU];
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = xh[j];
    for (int t = 0; t < N; ++t) {
#pragma unroll
        for (int r = 0; r < NU; ++r) uh[r] = uhp[(int64_t)t * NU + r];
        smp_feedback<T, NX, NU>(uh, G + (int64_t)t * NU * NX, xh + (int64_t)t * NX, x, v);
        smp_noise<T, NU>(draw, (unsigned int)s, (unsigned int)t, eps);
        smp_clip_add<T, NU>(draw, v, eps, u);
        cost.add(x, u, t, N);
        if (t < N - 1) {
            model_step_at<MODEL>(mdl, x, u, t, xn);
#pragma unroll
            for (int j = 0; j < NX; ++j) x[j] = xn[j];
        }
    }
    const T c = cost.total();
    if (s < p.S) p.costs[(int64_t)b * p.S + s] = c != c ? (T)__builtin_huge_val() : c;
}

// One closed-loop rollout from xa_0, costed; lane 0 leaves x_t in xbuf[t] and the realised, clipped u_t in ubuf[t].  REPLAY: sample
// `sample` again, u_t = clip((ua_t + G_t (x_t - xa_t)) + eps_t) with the draws regenerated step by step (ubuf is written only);
// else the candidate, u_t = clip(v_t + G_t (x_t - xa_t)) with v_t read from ubuf[t] before u_t goes there.
template <typename T, int NX, int NU, int MODEL, bool REPLAY>
__device__ __forceinline__ T smp_rollout_fb(const Model<T, NX, NU, MODEL> &mdl, SampleCost<T, NX, NU, MODEL> &cost, const SampleDraw<T, NU> &draw,
                                            unsigned int sample, T *ubuf, T *xbuf, const T *xa, const T *ua, const T *G, int N, int lane)
{
    T x[NX], xn[NX], u[NU], v[NU], base[NU], eps[NU];
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = xa[j];
    cost.reset();
    for (int t = 0; t < N; ++t) {
#pragma unroll
        for (int r = 0; r < NU; ++r) base[r] = REPLAY ? ua[(int64_t)t * NU + r] : ubuf[t * NU + r];
        smp_feedback<T, NX, NU>(base, G + (int64_t)t * NU * NX, xa + (int64_t)t * NX, x, v);
        if constexpr (REPLAY) {
            smp_noise<T, NU>(draw, sample, (unsigned int)t, eps);
        } else {
#pragma unroll
            for (int r = 0; r < NU; ++r) eps[r] = T(0);
        }
        smp_clip_add<T, NU>(draw, v, eps, u);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < NU; ++r) ubuf[t * NU + r] = u[r];
#pragma unroll
            for (int j = 0; j < NX; ++j) xbuf[t * NX + j] = x[j];
        }
        cost.add(x, u, t, N);
        if (t < N - 1) {
            model_step_at<MODEL>(mdl, x, u, t, xn);
#pragma unroll
            for (int j = 0; j < NX; ++j) x[j] = xn[j];
        }
    }
    return cost.total();
}

template <typename T, int NX, int NU, int MODEL>
__global__ __launch_bounds__(64) void sample_update_fb_kernel(SampleFbP<T> q)
{
    extern __shared__ __align__(16) unsigned char smp_smem[];
    constexpr int MDLW = smp_mdl_words(Model<T, NX, NU, MODEL>::LDS_WORDS), TT = kSmpTile;
    const SampleP<T> &p = q.p;
    const int lane = threadIdx.x, N = p.N, S = p.S, b = blockIdx.x;
    if (p.active && p.active[b] == 0) return;                  // uniform: the trajectory and its statistics stay as they are
    T *ubuf = reinterpret_cast<T *>(smp_smem) + MDLW;          // [N][NU]
    T *xbuf = ubuf + N * NU;                                   // [N][NX]
    const T *cs = p.costs + (int64_t)b * S;
    const T inf = (T)__builtin_huge_val();
    const int64_t so = (int64_t)b * p.stat_sb;

    // ---- minimum and first arg-min (as sample_update_kernel) -----------------------------------------------------------------------
    T cmin = inf;
    int imin = 0x7fffffff;
    for (int s = lane; s < S; s += kWave) {
        const T c = cs[s];
        if (c < cmin) { cmin = c; imin = s; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T oc = __shfl_xor(cmin, o, kWave);
        const int oi = __shfl_xor(imin, o, kWave);
        if (oc < cmin || (oc == cmin && oi < imin)) { cmin = oc; imin = oi; }
    }
    const T c0 = cs[0];
    if (!(c0 < inf) || !(c0 > -inf)) {                         // the nominal's own rollout has no finite cost: nothing to start from
        if (lane == 0) {
            if (p.cost_before) p.cost_before[so] = c0;
            if (p.cost_after) p.cost_after[so] = c0;
            if (p.cost_best) p.cost_best[so] = cmin;
            if (p.ess) p.ess[so] = T(0);
            if (p.took_best) p.took_best[so] = 0;
        }
        return;
    }

    // ---- weights (as sample_update_kernel) -------------------------------------------------------------------------------------------
    const T tiny = smp_tiny(T(0));
    const T lam = p.temperature * (cmin > tiny ? cmin : tiny);
    T wsum = T(0), w2 = T(0);
    for (int s = lane; s < S; s += kWave) {
        const T w = smp_weight(cs[s], cmin, lam);
        wsum += w;
        w2 += w * w;
    }
    wsum = wave_sum(wsum);
    w2 = wave_sum(w2);

    Model<T, NX, NU, MODEL> mdl;
    mdl.load(p.par + (int64_t)b * p.par_sb, reinterpret_cast<T *>(smp_smem), lane, kWave);
    SampleDraw<T, NU> draw;
    draw.load(p, b);
    SampleCost<T, NX, NU, MODEL> cost;
    cost.load(p, b);
    T *xh = p.xhat + (int64_t)b * N * NX, *uhp = p.uhat + (int64_t)b * N * NU;
    const T *G = q.K + (int64_t)b * q.K_sb;

    // ---- v_t = uhat_t + sum_s w_s eps_st, the draws regenerated ---------------------------------------------------------------------
    for (int t0 = 0; t0 < N; t0 += TT) {
        T acc[TT][NU];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
            for (int r = 0; r < NU; ++r) acc[tt][r] = T(0);
        }
        for (int s = lane; s < S; s += kWave) {
            const T wn = smp_weight(cs[s], cmin, lam) / wsum;
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                if (t0 + tt < N) {                             // uniform
                    T eps[NU];
                    smp_noise<T, NU>(draw, (unsigned int)s, (unsigned int)(t0 + tt), eps);
#pragma unroll
                    for (int r = 0; r < NU; ++r) acc[tt][r] += wn * eps[r];
                }
            }
        }
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
#pragma unroll
            for (int r = 0; r < NU; ++r) {
                const T a = wave_sum(acc[tt][r]);
                if (lane == 0 && t0 + tt < N) ubuf[(t0 + tt) * NU + r] = mc_add(uhp[(int64_t)(t0 + tt) * NU + r], a);
            }
        }
    }
    __syncthreads();

    // ---- the candidate in closed loop; where it does not beat the best sample, that sample again -------------------------------------
    const T cnew = smp_rollout_fb<T, NX, NU, MODEL, false>(mdl, cost, draw, 0u, ubuf, xbuf, xh, uhp, G, N, lane);
    const bool take_best = !(cnew < cmin);
    if (take_best) {                                           // uniform
        __syncthreads();
        smp_rollout_fb<T, NX, NU, MODEL, true>(mdl, cost, draw, (unsigned int)imin, ubuf, xbuf, xh, uhp, G, N, lane);
    }
    __syncthreads();
    for (int e = lane; e < N * NU; e += kWave) uhp[e] = ubuf[e];
    for (int e = NX + lane; e < N * NX; e += kWave) xh[e] = xbuf[e];   // xhat_0 is never written
    if (lane == 0) {
        if (p.cost_before) p.cost_before[so] = c0;
        if (p.cost_after) p.cost_after[so] = take_best ? cmin : cnew;
        if (p.cost_best) p.cost_best[so] = cmin;
        if (p.ess) p.ess[so] = (wsum * wsum) / w2;
        if (p.took_best) p.took_best[so] = take_best ? 1 : 0;
    }
}

#ifndef __HIPCC_RTC__
// the two launches of a user model and / or a user cost (user_rtc.hip), from the module of the (model, cost) pair; K: the closed-loop
// pair of kernels with these gains (nullptr: the open-loop pair)
template <typename T>
int launch_sample_user(const SampleP<T> &p, int model, int cost, int n, int m, size_t smem_cost, size_t smem_update, int phase,
                       hipStream_t s, const T *K = nullptr, int64_t K_sb = 0);
#endif

}  // namespace isls
