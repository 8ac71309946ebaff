// gain_memo.hip -- the memo of the batch-shared Riccati gain table (gain_memo.hpp): its entries and its two small kernels.
#include <mutex>
#include <vector>

#include "gain_memo.hpp"

namespace isls {

// the words the shared-form recursion reads, in logical order (the declared strides are followed, not stored)
template <typename T>
struct MemoIn {
    View<T> v[3];                  // Cxx, Cuu, Cux (batch stride 0)
    int sz[3];                     // n n, m m, m n (0: no Cux)
    const T *par;                  // the model's parameter row [a, b0, b1]
    int N;
};
constexpr int kMemoPar = 3;

template <typename T, typename F>
__device__ __forceinline__ void memo_for_each(const MemoIn<T> &in, int tid, int nth, F &&f)
{
    int base = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int sz = in.sz[a], tot = in.N * sz;
        const T *src = in.v[a].p;
        const int64_t st = in.v[a].st;
        for (int w = tid; w < tot; w += nth) {
            const int t = w / sz, e = w - t * sz;
            f(src + (int64_t)t * st + e, base + w);
        }
        base += tot;
    }
    for (int w = tid; w < kMemoPar; w += nth) f(in.par + w, base + w);
}

__device__ __forceinline__ uint64_t memo_bits(double v) { return __builtin_bit_cast(uint64_t, v); }
__device__ __forceinline__ uint32_t memo_bits(float v) { return __builtin_bit_cast(uint32_t, v); }

// One workgroup.  Besides the verdict it leaves the snapshot equal to the inputs: a word that differs is replaced on the spot (the
// value is in a register already), so a miss needs no second sweep over the inputs -- block 0 of the gain launch that follows
// writes the table and sets `filled` (riccati.hip).  Between the two the entry is marked unfilled: a gain launch that never
// ran (a failed launch) cannot leave a new snapshot next to an old table.
template <typename T>
__global__ __launch_bounds__(1024) void gain_memo_check_kernel(MemoIn<T> in, T *snap, int32_t *hdr, int64_t *cnt)
{
    int diff = 0;
    memo_for_each(in, (int)threadIdx.x, (int)blockDim.x, [&](const T *src, int w) {
        const T v = *src;
        const bool other = memo_bits(v) != memo_bits(snap[w]);               // bit patterns
        if (other) snap[w] = v;
        diff |= other || (v != v);                                           // a NaN never matches
    });
    const int any = __syncthreads_or(diff);
    if (threadIdx.x == 0) {
        const int match = (hdr[kMemoFilled] != 0 && !any) ? 1 : 0;
        hdr[kMemoMatch] = match;
        if (!match) hdr[kMemoFilled] = 0;
        cnt[0] += 1;
        cnt[1] += match;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void gain_memo_broadcast_kernel(const T *table, T *K, const int32_t *active, const int32_t *hdr, int N, int kw,
                                                                  int step_words)
{
    if (!hdr[kMemoMatch]) return;
    const int b = blockIdx.x;
    if (active && !active[b]) return;
    typedef T V2 __attribute__((ext_vector_type(2)));
    const int kp = kw / 2, tot = N * kp;
    V2 *dst = reinterpret_cast<V2 *>(K + (int64_t)b * N * kw);
    for (int w = threadIdx.x; w < tot; w += blockDim.x) {
        const int t = w / kp, e = w - t * kp;
        V2 v = {T(0), T(0)};                                   // K[N-1] = 0
        if (t < N - 1) v = *reinterpret_cast<const V2 *>(table + (int64_t)t * step_words + 2 * e);
        st_stream(dst + w, v);
    }
}

// ---- entries -------------------------------------------------------------------------------------------------------------
namespace {
struct Entry {
    int dev, dtype, n, m, N, mode, cux;
    hipStream_t s;
    char *base;
    size_t snap_off, table_off;
};
std::mutex g_mu;
std::vector<Entry> g_entries;

size_t round16(size_t x) { return (x + 15) & ~(size_t)15; }
int memo_snap_words(int n, int m, int N, int cux) { return N * (n * n + m * m + (cux ? m * n : 0)) + kMemoPar; }
int memo_step_words(int n, int m) { return (kWave / (n + m)) * rec_lean_stride(n, m); }
}  // namespace

template <typename T>
bool gain_memo_acquire(const isls_gain_args &g, hipStream_t s, GainMemoRef &ref)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (cap != hipStreamCaptureStatusNone) return false;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const int dtype = sizeof(T) == 8 ? ISLS_DTYPE_F64 : ISLS_DTYPE_F32, cux = g.Cux.p ? 1 : 0;
    std::lock_guard<std::mutex> lock(g_mu);
    const Entry *hit = nullptr;
    for (const Entry &e : g_entries)
        if (e.dev == dev && e.s == s && e.dtype == dtype && e.n == g.n && e.m == g.m && e.N == g.N && e.mode == g.solve_mode && e.cux == cux) {
            hit = &e;
            break;
        }
    if (!hit) {
        Entry e = {dev, dtype, g.n, g.m, g.N, g.solve_mode, cux, s, nullptr, 0, 0};
        e.snap_off = round16(kMemoHdrWords * sizeof(int32_t) + 2 * sizeof(int64_t));
        e.table_off = e.snap_off + round16((size_t)memo_snap_words(g.n, g.m, g.N, cux) * sizeof(T));
        const size_t bytes = e.table_off + round16((size_t)g.N * memo_step_words(g.n, g.m) * sizeof(T));
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (hipMemsetAsync(p, 0, bytes, s) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); return false; }
        e.base = static_cast<char *>(p);
        g_entries.push_back(e);
        hit = &g_entries.back();
    }
    ref.hdr = reinterpret_cast<int32_t *>(hit->base);
    ref.cnt = reinterpret_cast<int64_t *>(hit->base + kMemoHdrWords * sizeof(int32_t));
    ref.snap = hit->base + hit->snap_off;
    ref.table = hit->base + hit->table_off;
    return true;
}
template bool gain_memo_acquire<double>(const isls_gain_args &, hipStream_t, GainMemoRef &);
template bool gain_memo_acquire<float>(const isls_gain_args &, hipStream_t, GainMemoRef &);

template <typename T>
static MemoIn<T> memo_inputs(const isls_gain_args &g)
{
    MemoIn<T> in;
    in.v[0] = View<T>(g.Cxx); in.v[1] = View<T>(g.Cuu); in.v[2] = View<T>(g.Cux);
    in.sz[0] = g.n * g.n; in.sz[1] = g.m * g.m; in.sz[2] = g.Cux.p ? g.m * g.n : 0;
    in.par = (const T *)g.lin_par;
    in.N = g.N;
    return in;
}

template <typename T>
int launch_gain_memo_check(const isls_gain_args &g, const GainMemoRef &ref, hipStream_t s)
{
    hipLaunchKernelGGL((gain_memo_check_kernel<T>), dim3(1), dim3(1024), 0, s, memo_inputs<T>(g), (T *)ref.snap, ref.hdr, ref.cnt);
    return check_launch();
}
template int launch_gain_memo_check<double>(const isls_gain_args &, const GainMemoRef &, hipStream_t);
template int launch_gain_memo_check<float>(const isls_gain_args &, const GainMemoRef &, hipStream_t);

template <typename T>
int launch_gain_memo_broadcast(const isls_gain_args &g, const GainMemoRef &ref, hipStream_t s)
{
    if ((g.m * g.n) % 2 != 0) return ISLS_ERR_UNSUPPORTED;    // (the shared form has n = 2 m)
    hipLaunchKernelGGL((gain_memo_broadcast_kernel<T>), dim3(g.B), dim3(256), 0, s, (const T *)ref.table, (T *)g.K, g.active, ref.hdr, g.N, g.m * g.n,
                       memo_step_words(g.n, g.m));
    return check_launch();
}
template int launch_gain_memo_broadcast<double>(const isls_gain_args &, const GainMemoRef &, hipStream_t);
template int launch_gain_memo_broadcast<float>(const isls_gain_args &, const GainMemoRef &, hipStream_t);

int gain_memo_stats(int64_t *checks, int64_t *matches)
{
    int64_t tot[2] = {0, 0};
    int cur = 0;
    std::lock_guard<std::mutex> lock(g_mu);
    if (!g_entries.empty() && hipGetDevice(&cur) != hipSuccess) return ISLS_ERR_LAUNCH;
    int rc = ISLS_OK;
    for (const Entry &e : g_entries) {
        int64_t c[2] = {0, 0};
        if (hipSetDevice(e.dev) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(c, e.base + kMemoHdrWords * sizeof(int32_t), sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = ISLS_ERR_LAUNCH;
            break;
        }
        tot[0] += c[0];
        tot[1] += c[1];
    }
    if (!g_entries.empty()) (void)hipSetDevice(cur);
    if (checks) *checks = tot[0];
    if (matches) *matches = tot[1];
    return rc;
}

void gain_memo_clear()
{
    int cur = 0;
    std::lock_guard<std::mutex> lock(g_mu);
    if (g_entries.empty() || hipGetDevice(&cur) != hipSuccess) return;
    for (const Entry &e : g_entries) {
        if (hipSetDevice(e.dev) != hipSuccess) continue;
        (void)hipDeviceSynchronize();                          // launches that still read the entry
        (void)hipFree(e.base);
    }
    g_entries.clear();
    (void)hipSetDevice(cur);
}

}  // namespace isls
