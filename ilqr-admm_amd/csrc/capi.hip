// capi.hip -- extern "C" surface of libisls_hip.so (declared in include/isls_hip.h) and the
// stream-ordered driver of one outer DP-form iLQR-ADMM iteration.
#include <new>
#include <vector>

#include "isls_common.hpp"
#include "covariance.hpp"
#include "entry.hpp"
#include "gain_memo.hpp"

namespace isls {

// ---- optional per-kernel-family timing with HIP events on the launch stream -----------------------
// (bench.py reads these: average launch duration of the dominant kernel for the roofline line).  The context is
// caller-owned (isls_timing_create / isls_timing_destroy) and reaches the driver through isls_outer_args.timing: the
// library itself keeps no state.  One context belongs to one host thread / stream at a time.
struct Timing {
    bool paused = false;           // events are recorded only while !paused (bench.py samples every k-th step)
    static constexpr int kKinds = 5;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[kKinds];
    size_t used[kKinds] = {0, 0, 0, 0, 0};
};

struct ScopedTimer {
    hipStream_t s;
    hipEvent_t stop = nullptr;
    ScopedTimer(Timing *tm, int kind, hipStream_t s_) : s(s_)
    {
        if (!tm || tm->paused) return;
        auto &pool = tm->ev[kind];
        size_t &u = tm->used[kind];
        if (u == pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess) return;
            if (hipEventCreate(&b) != hipSuccess) { hipEventDestroy(a); return; }
            pool.emplace_back(a, b);
        }
        hipEventRecord(pool[u].first, s);
        stop = pool[u].second;
        ++u;
    }
    ~ScopedTimer()
    {
        if (stop) hipEventRecord(stop, s);
    }
};

template <typename T>
static int outer_iteration(const isls_outer_args &a, hipStream_t s)
{
    const isls_admm_args &ad = a.admm;
    Timing *const tmg = static_cast<Timing *>(a.timing);
    int rc = ISLS_OK;
    if (!a.begin_done &&
        (rc = launch_outer_begin<T>(ad.B, ad.N, ad.n, ad.m, ad.active, a.outer_active, ad.lx, ad.lu, ad.res_prev, ad.iters, s)) != ISLS_OK)
        return rc;
    bool ff_done = false;                                      // the gain pass ran the first feed-forward pass as well
    // the gain pass writes the records in the layout its hint selects and the feed-forward passes read them in theirs
    if (a.J > 0 && !lin_hints_agree(a.gain, a.ff)) return ISLS_ERR_ARG;
    if (a.ff.lin_on && ff_seg_enabled(a.ff.seg)) return ISLS_ERR_UNSUPPORTED;   // the segment operators need the dense records
    // One set of records for the whole batch (isls_gain_args.rec in include/isls_hip.h): the declared strides and hints say that
    // every trajectory has the same A, B, Cxx, Cuu, Cux, this call's gain pass writes the records its own feed-forward passes and
    // line searches read, the recursion is sequential, and all four blocks speak of the same batch and mask.  Then K_t and fac_t
    // are the same for every trajectory: the gain pass writes them once, and the other passes read that one table (which stays
    // in the caches) instead of a copy per trajectory.  The K array is still written for every trajectory.
    const bool shared = a.J > 0 && !a.skip_gain && gain_inputs_shared(a.gain) && dims_supported(a.gain.n, a.gain.m) &&
                        a.ff.rec == a.gain.rec && a.ff.lin_on && a.ff.lin_model == a.gain.lin_model && a.ff.lin_par_sb == 0 &&
                        !ff_seg_enabled(a.ff.seg) && a.ff.B == a.gain.B && a.ff.N == a.gain.N && a.ff.n == a.gain.n &&
                        a.ff.m == a.gain.m && a.ff.active == a.gain.active && a.ff._pad <= 1 && a.ro.B == a.gain.B &&
                        a.ro.N == a.gain.N && a.ro.n == a.gain.n && a.ro.m == a.gain.m && a.ro.K == a.gain.K &&
                        a.ro.active == a.gain.active;
    // The shared table is kept across calls, valid by content (gain_memo.hpp).  Three launches, stream-ordered:
    //   check     compares the recursion's inputs with the entry's snapshot (and brings the snapshot up to them);
    //   gain      stands down on a match; otherwise its block 0 writes the records into the entry's table and marks it filled;
    //   stand-in  on a match only: the first feed-forward pass the gain launch would have run, which also writes the K array
    //             from the table's records it stages (a call whose first pass does not ride on the gain launch has no stand-in:
    //             a K broadcast launch takes its place).
    // Which of them do the work is decided on the device alone.  Every reader takes the entry's table.  A hit used to be five
    // launches (check, gain, commit, stand-in, K broadcast): the commit launch did nothing on a hit and cost 4.7 us, the
    // broadcast 11.8 us behind the stand-in pass's 42.0 us (B = 4096, N = 100, fp64; DESIGN section 5 has the figures since).
    GainMemoRef memo;
    // (an empty batch launches nothing, the gain pass included: no check counted, no entry touched)
    const bool memo_on = shared && a.gain.B > 0 && gain_memo_acquire<T>(a.gain, s, memo);
    const void *const shared_rec = memo_on ? memo.table : (shared ? a.gain.rec : nullptr);
    isls_ff_args ff_sh = a.ff;
    if (memo_on) ff_sh.rec = memo.table;
    if (!a.skip_gain) {
        {
            ScopedTimer tm(tmg, 0, s);
            if (memo_on && (rc = launch_gain_memo_check<T>(a.gain, memo, s)) != ISLS_OK) return rc;
            // The gain pass with the recursion inside holds 370-400 registers: one wavefront per SIMD.  While its wavefronts fit
            // the chip's SIMDs that costs nothing; beyond (B > 7168 at n = 6, m = 3 on 256 CUs) the surplus runs as a second round
            // and the launch doubles (123 -> 251 us from B = 4096 to 8192), where the pass without the recursion (<= 256 registers,
            // two wavefronts per SIMD) and a feed-forward launch of its own take 148 + 82 us.
            static const int64_t simds = [] {
                int dev = 0; hipDeviceProp_t pr;
                if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) return (int64_t)1024;
                return (int64_t)pr.multiProcessorCount * 4;
            }();
            const int lanes = a.gain.n + a.gain.m;
            const int64_t waves = lanes > 0 && lanes <= kWave ? (a.gain.B + kWave / lanes - 1) / (kWave / lanes) : 0;
            const bool fuse_now = a.J > 0 && waves <= simds;
            if ((rc = launch_gain<T>(a.gain, s, fuse_now ? &a.ff : nullptr, &ff_done, false, shared, memo_on ? memo.hdr : nullptr,
                                      memo_on ? memo.table : nullptr)) != ISLS_OK)
                return rc;
            if (memo_on) {                                     // (one timed family with the gain launch it stands in for)
                // the pass that rode on the gain launch, and the K array, where that launch stood down
                if (ff_done) rc = launch_ff<T>(ff_sh, s, true, memo.hdr + kMemoMatch, a.gain.K);
                else rc = launch_gain_memo_broadcast<T>(a.gain, memo, s);
                if (rc != ISLS_OK) return rc;
            }
        }
        if (ff_seg_enabled(a.ff.seg)) {                        // operators of the time-parallel feed-forward pass
            const isls_ff_args &f = a.ff;
            isls_ff_prepare_args pr = {};
            pr.B = f.B; pr.N = f.N; pr.n = f.n; pr.m = f.m; pr.solve_mode = f.solve_mode;
            pr.A = f.A; pr.Bm = f.Bm; pr.K = f.K; pr.Quu = f.Quu; pr.fac = f.fac; pr.Qux = f.Qux;
            pr.active = f.active; pr.seg = f.seg; pr.rec = f.rec;
            ScopedTimer tm(tmg, 4, s);
            if ((rc = launch_ff_prepare<T>(pr, s)) != ISLS_OK) return rc;
        }
    }
    // element-wise ADMM updates ride on the winner replay of the rollout (one launch and one pass over x, u less)
    const bool fuse = rollout_can_fuse_admm(a.ro, a.admm);
    bool fused = false;
    for (int j = 0; j < a.J; ++j) {
        if (!(j == 0 && ff_done)) {
            ScopedTimer tm(tmg, 1, s);
            if ((rc = launch_ff<T>(memo_on ? ff_sh : a.ff, s, shared)) != ISLS_OK) return rc;
        }
        {
            ScopedTimer tm(tmg, 2, s);
            if ((rc = launch_rollout<T>(a.ro, s, fuse ? &a.admm : nullptr, &fused, j == a.J - 1 || a.log != nullptr, shared_rec)) != ISLS_OK) return rc;
        }
        if (!fused) {
            ScopedTimer tm(tmg, 3, s);
            if ((rc = launch_admm<T>(a.admm, s)) != ISLS_OK) return rc;
        }
        if (a.log) {
            if (hipMemcpyAsync((T *)a.log + (size_t)j * ad.B * 2, ad.res, sizeof(T) * (size_t)ad.B * 2,
                               hipMemcpyDeviceToDevice, s) != hipSuccess)
                return ISLS_ERR_LAUNCH;
        }
    }
    return ISLS_OK;
}

}  // namespace isls

using namespace isls;

ISLS_ENTRY(riccati_gain, isls_gain_args, launch_gain, a->B == 0)
ISLS_ENTRY(riccati_ff, isls_ff_args, launch_ff, a->B == 0)
ISLS_ENTRY(riccati_ff_prepare, isls_ff_prepare_args, launch_ff_prepare, a->B == 0)
ISLS_ENTRY(rollout_ls, isls_rollout_args, launch_rollout, a->B == 0)
ISLS_ENTRY(admm_update, isls_admm_args, launch_admm, a->B == 0)
ISLS_ENTRY(expand_quadratic, isls_expand_args, launch_expand, a->B == 0)
ISLS_ENTRY(linearize, isls_linearize_args, launch_linearize, a->B == 0)
ISLS_ENTRY(accept_step, isls_accept_args, launch_accept, a->B == 0)
ISLS_ENTRY(project_rows, isls_project_args, launch_project, false)
ISLS_ENTRY(sls_admm, isls_sls_admm_args, launch_sls_admm, false)
ISLS_ENTRY(dense_closed_loop, isls_dense_loop_args, launch_dense_closed_loop, false)
ISLS_ENTRY(mc_closed_loop, isls_mc_loop_args, launch_mc_closed_loop, false)
ISLS_ENTRY(mpc_step, isls_mpc_step_args, launch_mpc_step, false)
ISLS_ENTRY(sample_nominal, isls_sample_args, launch_sample_nominal, false)
ISLS_ENTRY(cov_closed_loop, isls_cov_args, launch_cov_closed_loop, false)
ISLS_ENTRY(sls_controller, isls_sls_controller_args, launch_sls_controller, false)
ISLS_ENTRY(columns_rollout, isls_columns_args, launch_columns_rollout, false)
ISLS_ENTRY(columns_admm, isls_columns_admm_args, launch_columns_admm, false)
ISLS_ENTRY(columns_iteration, isls_columns_iteration_args, launch_columns_iteration, false)
ISLS_ENTRY(outer_advance, isls_advance_args, launch_advance, false)
ISLS_ENTRY(ilqr_admm_outer, isls_outer_args, outer_iteration, false)
ISLS_ENTRY(reg_update, isls_reg_update_args, launch_reg_update, false)

ISLS_TYPED_PAIR(riccati_gain_ff, (const isls_gain_args *g, const isls_ff_args *ff, void *stream),
                if (!g || !ff) return ISLS_ERR_ARG;
                if (g->B == 0) return ISLS_OK;
                bool done = false;
                const int rc = launch_gain<T>(*g, (hipStream_t)stream, ff, &done, /*require_ff=*/true);
                return rc != ISLS_OK ? rc : (done ? ISLS_OK : ISLS_ERR_UNSUPPORTED);)
ISLS_TYPED_PAIR(riccati_gain_reg, (const isls_gain_args *g, const isls_ff_args *ff, const isls_reg_args *r, void *stream),
                if (!g || !r) return ISLS_ERR_ARG;
                return launch_gain_reg<T>(*g, (hipStream_t)stream, ff, *r);)
ISLS_TYPED_PAIR(sample_nominal_fb, (const isls_sample_args *a, const void *K, int64_t K_sb, void *stream),
                if (!a) return ISLS_ERR_ARG;
                return launch_sample_nominal_fb<T>(*a, K, K_sb, (hipStream_t)stream);)
ISLS_TYPED_PAIR(sls_closed_loop, (int32_t M, int32_t N, int32_t n, int32_t m, const void *A, const void *B, const void *K, const void *k,
                                  const void *x0, void *x_log, void *u_log, void *stream),
                return launch_sls_closed_loop<T>(M, N, n, m, A, B, K, k, x0, x_log, u_log, (hipStream_t)stream);)
ISLS_TYPED_PAIR(reduce_convergence, (int32_t B, const void *cost, const void *res, const int32_t *active, const int32_t *status,
                                     void *out5, void *stream),
                return launch_reduce<T>(B, cost, res, active, status, out5, (hipStream_t)stream);)
ISLS_TYPED_PAIR(reduce_convergence_table, (int32_t B, const void *cost, const void *res, const int32_t *active, const int32_t *status,
                                           void *table, int32_t rank, int32_t world, void *stream),
                if (rank < 0) return ISLS_ERR_ARG;
                return launch_reduce<T>(B, cost, res, active, status, table, (hipStream_t)stream, rank, world);)

ISLS_API int64_t isls_sls_controller_work_elems(int32_t B, int32_t N, int32_t n) { return sls_controller_work_elems(B, N, n); }

ISLS_API int64_t isls_mc_work_elems(int32_t P, int32_t M, int32_t N, int32_t n, int32_t m, int32_t K_form)
{
    return mc_work_elems(P, M, N, n, m, K_form);
}

ISLS_API int32_t isls_ff_segments(int32_t N, int32_t nseg_requested, int32_t *seg_len)
{
    int len = 0;
    const int n = ff_segments(N, nseg_requested, &len);
    if (seg_len) *seg_len = len;
    return n;
}

ISLS_API int64_t isls_ff_record_elems(int32_t B, int32_t N, int32_t n, int32_t m)
{
    if (B < 0 || N < 1 || n < 1 || m < 1 || n + m > kWave) return 0;
    const int64_t tpw = kWave / (n + m), rw = rec_stride(n, m);
    return ((B + tpw - 1) / tpw) * tpw * N * rw;
}

ISLS_API int isls_version(void) { return ISLS_VERSION; }

ISLS_API int isls_gain_memo_stats(int64_t *checks, int64_t *matches) { return gain_memo_stats(checks, matches); }

ISLS_API void isls_gain_memo_clear(void) { gain_memo_clear(); }

ISLS_API int32_t isls_dims_supported(int32_t n, int32_t m) { return dims_supported(n, m) ? 1 : 0; }

ISLS_API int32_t isls_dims_generic(int32_t n, int32_t m) { return dims_generic(n, m) ? 1 : 0; }

ISLS_API const char *isls_error_string(int code)
{
    switch (code) {
        case ISLS_OK: return "ok";
        case ISLS_ERR_ARG: return "bad argument (null pointer or dimension)";
        case ISLS_ERR_UNSUPPORTED: return "unsupported (n,m) pair, model, projection or L";
        case ISLS_ERR_LAUNCH: return "HIP launch failed";
        case ISLS_ERR_COMPILE: return "user model: run-time compile failed (isls_user_model_log) or hiprtc not found";
        default: return "unknown";
    }
}

ISLS_API void *isls_timing_create(void) { return new (std::nothrow) Timing(); }

ISLS_API void isls_timing_destroy(void *h)
{
    Timing *tm = static_cast<Timing *>(h);
    if (!tm) return;
    for (int k = 0; k < Timing::kKinds; ++k)
        for (auto &pr : tm->ev[k]) {
            hipEventDestroy(pr.first);
            hipEventDestroy(pr.second);
        }
    delete tm;
}

// Start a new measurement window (the recorded events of the previous one are reused).
ISLS_API int isls_timing_reset(void *h)
{
    Timing *tm = static_cast<Timing *>(h);
    if (!tm) return ISLS_ERR_ARG;
    tm->paused = false;
    for (int k = 0; k < Timing::kKinds; ++k) tm->used[k] = 0;
    return ISLS_OK;
}

// Suspend / resume event recording inside a measurement window without resetting it (an event pair per launch
// costs a few microseconds of queue bubbles; sampling every k-th step keeps the timed region representative).
ISLS_API int isls_timing_pause(void *h, int paused)
{
    Timing *tm = static_cast<Timing *>(h);
    if (!tm) return ISLS_ERR_ARG;
    tm->paused = paused != 0;
    return ISLS_OK;
}

// Sum of the event-bracketed durations of kernel family `kind` since isls_timing_reset(); *count = number of
// launches.  Synchronises on the recorded events (call it outside the timed region).
ISLS_API double isls_timing_read_ms(void *h, int kind, int *count)
{
    Timing *tm = static_cast<Timing *>(h);
    if (!tm || kind < 0 || kind >= Timing::kKinds) return -1.0;
    double total = 0.0;
    const size_t n = tm->used[kind];
    for (size_t i = 0; i < n; ++i) {
        float ms = 0.f;
        hipEventSynchronize(tm->ev[kind][i].second);
        if (hipEventElapsedTime(&ms, tm->ev[kind][i].first, tm->ev[kind][i].second) == hipSuccess) total += ms;
    }
    if (count) *count = (int)n;
    return total;
}
