// mpc.hpp -- one control step of a receding-horizon loop for the whole batch (isls_mpc_step_*): the first control of every plan
// goes through the plant, the plan (nominal, gains, ADMM targets, cost table) moves up by one step IN PLACE with its last row
// held, and the plan is rolled out again from the measured state (kernel template; launched by mpc.hip for the built-in models
// and by user_model.hip from a user model's run-time compiled module).
//
// Reference semantics: the nominal_values setter (isls/isls_base.py:80-85: a new nominal replaces the old one) and the order of
// a closed-loop step (isls/isls_base.py:59-75: the control first, then the step, then the noise), as in monte_carlo.hpp.
//
// Mapping: one 64-lane wavefront per workgroup, cut into four slots of kMpcLanes = 16 lanes; a slot owns one trajectory and
// walks its horizon once, t ascending.
//   ownership  : lane c of the slot owns words c, c + 16, ... of EVERY row of every array of the plan.  The owner of word e reads
//                (t+1, e) and writes (t, e), and nobody else ever touches either: the in-place shift needs no barrier and no second
//                buffer -- a word is read (program order of one lane) before the step that overwrites it.  A step's words of
//                K, xhat, uhat are adjacent over the slot's lanes: one contiguous run per array and step.
//   prefetch   : the rows of D steps ahead are in flight in a register ring (D = 4; 2 at the run-time dimensions, whose rows of K
//                are eight words per lane), fetched unconditionally with the row index clamped to N-1 -- the pass is one dependent
//                chain of N model steps per trajectory and is bound by the latency of these loads, not by their bytes.
//   per step   : the copies (K, zx, zu, the table) leave straight from the ring; K~_t, x~_t, u~_t go to the slot's LDS record
//                and come back as broadcasts; every lane of the slot forms u_t and steps the model redundantly (the state lives
//                in registers), lane 0 drops x_t, u_t into the record's out words and the owners write them to row t.
//   the table  : a shared table (tab_sb == 0) is moved by the slot of the launch's trajectory 0 alone.
// u_t = (sum_j K~_t[r][j] (x_t - x~_t)[j]) + u~_t with explicit fma, j ascending from 0, as in monte_carlo.hpp.
#pragma once

#include "monte_carlo.hpp"

namespace isls {

constexpr int kMpcLanes = 16;      // lanes per trajectory
constexpr int kMpcMaxTab = 16;     // words per row of the cost table at most (ISLS_USER_MAX_TAB)

template <typename T>
struct MpcP {
    int B, N, n, m, W;
    const T *par, *plant;
    int64_t par_sb, plant_sb;
    T *xhat, *uhat, *K, *zx, *zu, *tab;
    int64_t tab_sb;
    const T *tab_next;
    int64_t tab_next_sb;
    const T *u_lo, *u_hi, *w, *noise_std;
    unsigned long long seed;
    unsigned int problem0, step;
    T *x_meas, *u_out, *x_next;
    int64_t x_meas_sb, u_out_sb, x_next_sb;
};

template <int NX, int NU>
struct MpcLayout {
    static constexpr int GL = kMpcLanes, TPW = kWave / kMpcLanes;
    static constexpr int CK = (NU * NX + GL - 1) / GL, CX = (NX + GL - 1) / GL, CU = (NU + GL - 1) / GL,
                         CT = (kMpcMaxTab + GL - 1) / GL;      // words per lane of a row of K, x, u, the table
    static constexpr int D = NX * NU > 32 ? 2 : 4;             // rows in flight per lane
    static constexpr int REC = NU * NX + NX + NU, OUT = NX + NU;
    // slot (words): plant model | solver model | record K~ x~ u~ | out x u
    __host__ __device__ static constexpr int mdl_words(int mdlw) { return mdlw + (mdlw & 1); }
    __host__ __device__ static constexpr int slot_words(int mdlw) { return 2 * mdl_words(mdlw) + REC + OUT; }
};

// the words a lane owns of the rows one step reads: row t+1 of the plan (row N-1 held), the table's next row
template <typename T, int NX, int NU>
struct MpcRow {
    using LY = MpcLayout<NX, NU>;
    T K[LY::CK], x[LY::CX], u[LY::CU], zx[LY::CX], zu[LY::CU], tb[LY::CT];
};

// the trajectory's arrays (row 0) and what this slot moves
template <typename T>
struct MpcSrc {
    T *K, *x, *u, *zx, *zu, *tab;
    const T *tnext;
    int N, n, m, mn, W, c;
};

// the rows step `ts` reads; beyond the horizon the fetch repeats the last step's (unconditional, always inside the arrays)
template <typename T, int NX, int NU>
__device__ __forceinline__ void mpc_fetch(MpcRow<T, NX, NU> &o, const MpcSrc<T> &s, int ts)
{
    using LY = MpcLayout<NX, NU>;
    const int r = ts + 1 < s.N ? ts + 1 : s.N - 1;
    if (s.K) {
        const T *q = s.K + (int64_t)r * s.mn;
#pragma unroll
        for (int j = 0; j < LY::CK; ++j) o.K[j] = q[s.c + LY::GL * j < s.mn ? s.c + LY::GL * j : 0];
    }
    {
        const T *qx = s.x + (int64_t)r * s.n, *qu = s.u + (int64_t)r * s.m;
#pragma unroll
        for (int j = 0; j < LY::CX; ++j) o.x[j] = qx[s.c + LY::GL * j < s.n ? s.c + LY::GL * j : 0];
#pragma unroll
        for (int j = 0; j < LY::CU; ++j) o.u[j] = qu[s.c + LY::GL * j < s.m ? s.c + LY::GL * j : 0];
    }
    if (s.zx) {
        const T *q = s.zx + (int64_t)r * s.n;
#pragma unroll
        for (int j = 0; j < LY::CX; ++j) o.zx[j] = q[s.c + LY::GL * j < s.n ? s.c + LY::GL * j : 0];
    }
    if (s.zu) {
        const T *q = s.zu + (int64_t)r * s.m;
#pragma unroll
        for (int j = 0; j < LY::CU; ++j) o.zu[j] = q[s.c + LY::GL * j < s.m ? s.c + LY::GL * j : 0];
    }
    if (s.tab) {                                               // the last row takes the caller's next row where there is one
        const T *q = (ts >= s.N - 1 && s.tnext) ? s.tnext : s.tab + (int64_t)r * s.W;
#pragma unroll
        for (int j = 0; j < LY::CT; ++j) o.tb[j] = q[s.c + LY::GL * j < s.W ? s.c + LY::GL * j : 0];
    }
}

template <typename T, int NX, int NU, int MODEL>
__global__ __launch_bounds__(64) void mpc_step_kernel(MpcP<T> p)
{
    extern __shared__ __align__(16) unsigned char mpc_smem[];
    using LY = MpcLayout<NX, NU>;
    using Mdl = typename McModel<T, NX, NU, MODEL>::type;
    constexpr bool RT = MODEL == kMcModelRt;
    constexpr int GL = LY::GL, D = LY::D, MDLW = LY::mdl_words(McModel<T, NX, NU, MODEL>::LDS_WORDS);
    const int n = RT ? p.n : NX, m = RT ? p.m : NU, mn = m * n, N = p.N;
    const int sl = threadIdx.x / GL, c = threadIdx.x - sl * GL;
    const int b = blockIdx.x * LY::TPW + sl;
    const bool valid = b < p.B;
    const int bb = valid ? b : blockIdx.x * LY::TPW;          // idle slots shadow the block's first trajectory (loads only)
    T *slot = reinterpret_cast<T *>(mpc_smem) + sl * LY::slot_words(McModel<T, NX, NU, MODEL>::LDS_WORDS);
    T *rec = slot + 2 * MDLW, *out = rec + LY::REC;
    T *const rK = rec, *const rx = rec + mn, *const ru = rx + n;

    Mdl plant, mdl;
    if constexpr (RT) { plant.n = mdl.n = n; plant.m = mdl.m = m; }
    plant.load(p.plant + (int64_t)bb * p.plant_sb, slot, c, GL);
    mdl.load(p.par + (int64_t)bb * p.par_sb, slot + MDLW, c, GL);
    slot_sync();

    const int64_t bN = (int64_t)bb * N;
    MpcSrc<T> s;
    s.N = N; s.n = n; s.m = m; s.mn = mn; s.W = p.W; s.c = c;
    s.x = p.xhat + bN * n; s.u = p.uhat + bN * m;
    s.K = p.K ? p.K + bN * mn : nullptr;
    s.zx = p.zx ? p.zx + bN * n : nullptr;
    s.zu = p.zu ? p.zu + bN * m : nullptr;
    // the table: a trajectory's own, or the shared one in the hands of the launch's first trajectory
    const bool tab_mine = p.tab != nullptr && (p.tab_sb != 0 || b == 0);
    s.tab = tab_mine ? p.tab + (int64_t)bb * p.tab_sb : nullptr;
    s.tnext = p.tab_next ? p.tab_next + (int64_t)bb * p.tab_next_sb : nullptr;

    // ---- the first control through the plant: x+ = f(x_m, clip(u_0); plant) + w ---------------------------------------------
    T x[NX], u[NU], xn[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = j < n ? s.x[j] : T(0);
#pragma unroll
    for (int r = 0; r < NU; ++r) {
        u[r] = T(0);
        if (r < m) {
            T v = s.u[r];
            if (p.u_lo) { const T lo = p.u_lo[r]; v = v < lo ? lo : v; }
            if (p.u_hi) { const T hi = p.u_hi[r]; v = v > hi ? hi : v; }
            u[r] = v;
        }
    }
    plant.step(x, u, xn);
    if (c == 0 && valid) {
        if (p.x_meas) {
#pragma unroll
            for (int j = 0; j < NX; ++j)
                if (j < n) p.x_meas[(int64_t)b * p.x_meas_sb + j] = x[j];
        }
        if (p.u_out) {
#pragma unroll
            for (int r = 0; r < NU; ++r)
                if (r < m) p.u_out[(int64_t)b * p.u_out_sb + r] = u[r];
        }
    }
    if (p.w) {
#pragma unroll
        for (int j = 0; j < NX; ++j) x[j] = j < n ? mc_add(xn[j], p.w[(int64_t)bb * n + j]) : T(0);
    } else if (p.noise_std) {
#pragma unroll
        for (int g = 0; g < (NX + 3) / 4; ++g) {
            double z[4] = {0.0, 0.0, 0.0, 0.0};
            if (4 * g < n) philox::normal4(p.seed, 0u, p.problem0 + (unsigned int)bb, p.step, (unsigned int)g, z);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * g + e;
                if (j < NX) x[j] = j < n ? mc_add(xn[j], mc_scale(p.noise_std[j], z[e])) : T(0);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NX; ++j) x[j] = j < n ? xn[j] : T(0);
    }
    if (c == 0 && valid && p.x_next) {
#pragma unroll
        for (int j = 0; j < NX; ++j)
            if (j < n) p.x_next[(int64_t)b * p.x_next_sb + j] = x[j];
    }

    // ---- shift and re-roll: one pass, t ascending ------------------------------------------------------------------------------
    MpcRow<T, NX, NU> ring[D] = {};
#pragma unroll
    for (int d = 0; d < D; ++d) {
        mpc_fetch<T, NX, NU>(ring[d], s, d);
        __builtin_amdgcn_sched_barrier(0);                      // issue order = consumption order
    }
    const bool hasK = s.K != nullptr;
    for (int t0 = 0; t0 < N; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = t0 + d;
            if (t < N) {                                        // uniform
                const MpcRow<T, NX, NU> cur = ring[d];
                mpc_fetch<T, NX, NU>(ring[d], s, t + D);
                // the copies leave as they are; K~_t, x~_t, u~_t go to the record
#pragma unroll
                for (int j = 0; j < LY::CK; ++j) {
                    const int e = c + GL * j;
                    if (hasK && e < mn) {
                        rK[e] = cur.K[j];
                        if (valid) s.K[(int64_t)t * mn + e] = cur.K[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < LY::CX; ++j) {
                    const int e = c + GL * j;
                    if (e < n) {
                        rx[e] = cur.x[j];
                        if (valid && s.zx) s.zx[(int64_t)t * n + e] = cur.zx[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < LY::CU; ++j) {
                    const int e = c + GL * j;
                    if (e < m) {
                        ru[e] = cur.u[j];
                        if (valid && s.zu) s.zu[(int64_t)t * m + e] = cur.zu[j];
                    }
                }
                if (s.tab && valid) {
#pragma unroll
                    for (int j = 0; j < LY::CT; ++j)
                        if (c + GL * j < s.W) s.tab[(int64_t)t * s.W + c + GL * j] = cur.tb[j];
                }
                slot_sync();                                    // the record of step t is the slot's
                T dx[NX];
#pragma unroll
                for (int j = 0; j < NX; ++j) dx[j] = j < n ? x[j] - rx[j] : T(0);
#pragma unroll
                for (int r = 0; r < NU; ++r) {
                    u[r] = T(0);
                    if (r < m) {
                        u[r] = ru[r];
                        if (hasK) {
                            T acc = T(0);
#pragma unroll
                            for (int j = 0; j < NX; ++j)
                                if (j < n) acc = mc_fma(dx[j], rK[r * n + j], acc);
                            u[r] = mc_add(acc, ru[r]);
                        }
                    }
                }
                if (c == 0) {
#pragma unroll
                    for (int j = 0; j < NX; ++j)
                        if (j < n) out[j] = x[j];
#pragma unroll
                    for (int r = 0; r < NU; ++r)
                        if (r < m) out[n + r] = u[r];
                }
                slot_sync();                                    // x_t, u_t are the slot's: the owners write row t
                if (valid) {
#pragma unroll
                    for (int j = 0; j < LY::CX; ++j)
                        if (c + GL * j < n) s.x[(int64_t)t * n + c + GL * j] = out[c + GL * j];
#pragma unroll
                    for (int j = 0; j < LY::CU; ++j)
                        if (c + GL * j < m) s.u[(int64_t)t * m + c + GL * j] = out[n + c + GL * j];
                }
                if (t < N - 1) {
                    model_step_at<MODEL>(mdl, x, u, t, xn);   // (a table model: row t of the window, a global read)
#pragma unroll
                    for (int j = 0; j < NX; ++j) x[j] = j < n ? xn[j] : T(0);
                }
                slot_sync();                                    // the record and its out words are free for step t + 1
            }
        }
    }
}

#ifndef __HIPCC_RTC__
// the control step of a user model (user_model.hip), from the model's own module
template <typename T>
int launch_mpc_step_user(const MpcP<T> &p, int model, int grid, size_t smem, hipStream_t s);
#endif

}  // namespace isls
