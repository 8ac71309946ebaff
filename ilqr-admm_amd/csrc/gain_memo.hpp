// gain_memo.hpp -- the batch-shared Riccati gain table kept across outer iterations, valid by the CONTENT of its inputs.
//
// Where the outer driver keeps one set of lean records for the whole batch (capi.hip `shared`, riccati.hip SH), the recursion
// that produces them reads the batch-shared Cxx / Cuu (/ Cux) tables and the model's parameter row and nothing else.  An entry
// of the memo holds a snapshot of exactly those words, the N lean records block 0 of the gain pass wrote from them, and the
// words `filled` / `match`.  Every call compares the inputs with the snapshot ON THE DEVICE, in stream order (check kernel,
// which also brings the snapshot up to the inputs and clears `filled` where they differ); the gain launch returns at its top
// when they match, and when they do not its block 0 writes its records straight into the table and sets `filled` behind its
// step loop (riccati.hip) -- the check of this call has finished by then and nothing else reads the entry while the gain launch
// runs.  On a match the pass that stands in for the recursion inside the gain launch stages the table's records anyway and
// writes the K array from them (riccati_ffrec.hip, FU).  The host decides nothing: no address, no engine state and no switch
// enters the decision, so an in-place write to a table, a new rho, a reallocated buffer or another layout cannot leave a stale
// table in use.
//
// Entries are keyed by (device, stream, precision, n, m, N, solve mode, Cux present), created lazily under a mutex, written by
// the library's kernels only and freed by isls_gain_memo_clear().
#pragma once

#include "isls_common.hpp"

namespace isls {

// header words of an entry (int32)
constexpr int kMemoFilled = 0, kMemoMatch = 1, kMemoNotPd = 2, kMemoHdrWords = 4;

struct GainMemoRef {
    int32_t *hdr = nullptr;        // [filled, match, not_pd, -]
    int64_t *cnt = nullptr;        // [checks, matches]
    void *snap = nullptr;          // Cxx[N,n,n] | Cuu[N,m,m] | Cux[N,m,n] (if present) | lin_par[3]
    void *table = nullptr;         // the run of records block 0 of the gain pass writes: [N][64 / (n + m)][rec_lean_stride]
};

// The entry for this call, created on first use.  false: no memo for this call (the stream is capturing, or an allocation
// failed) -- the driver then enqueues the launches it enqueued before the memo existed.
template <typename T> bool gain_memo_acquire(const isls_gain_args &g, hipStream_t s, GainMemoRef &ref);
// match = filled && inputs == snapshot (bit patterns); snapshot <- inputs; match == 0: filled <- 0; one workgroup
template <typename T> int launch_gain_memo_check(const isls_gain_args &g, const GainMemoRef &ref, hipStream_t s);
// match == 1: the K prefix of the table's records -> K[b, :, :, :] of every active trajectory.  Only for a call without a
// stand-in pass (the first feed-forward pass did not ride on the gain launch): that pass writes K itself.
template <typename T> int launch_gain_memo_broadcast(const isls_gain_args &g, const GainMemoRef &ref, hipStream_t s);
int gain_memo_stats(int64_t *checks, int64_t *matches);
void gain_memo_clear();

}  // namespace isls
