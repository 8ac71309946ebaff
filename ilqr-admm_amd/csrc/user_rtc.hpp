// user_rtc.hpp -- the host of the run-time compiled pieces (user_rtc.hip): the registry of user sources (models and costs), the
// cache of their hiprtc programs and the module launcher.  A program is keyed by (model, cost, dtype): the model slot is a
// built-in id, a user model or kNone, the cost slot a user cost or kNone.  (user model, kNone) is the model's own program
// (user_model.hip launches its kernels), (kNone, cost) the cost's expansion and value (user_cost.hip), and a key with both slots
// filled is the line search of that pair, which launch_rollout_user (rollout_kernel.hpp) serves for every key.  A caller names
// the kernel it launches by its Role; where a kernel lies in a program only user_rtc.hip's Names knows.
#pragma once

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rollout_kernel.hpp"

namespace isls {

// LDS words of the model of the built-in family (n, m, model) of families.def -- a dense LTI model's [A B], none for the others;
// -1: no such family.  A count of words, the same in both precisions.  (Here and not in isls_common.hpp: every run-time
// compiled program includes that header, and a code object's symbol order follows its text, skipped lines included.)
inline int family_lds_words(int n, int m, int model)
{
#define ISLS_FAMILY_WORDS_(NX_, NU_, MODEL_)                                                                                         \
    static_assert(Model<double, NX_, NU_, MODEL_>::LDS_WORDS == Model<float, NX_, NU_, MODEL_>::LDS_WORDS, "LDS words depend on T"); \
    if (n == NX_ && m == NU_ && model == MODEL_) return Model<double, NX_, NU_, MODEL_>::LDS_WORDS;
    ISLS_FOR_EACH_FAMILY(ISLS_FAMILY_WORDS_)
#undef ISLS_FAMILY_WORDS_
    return -1;
}

namespace urtc {

enum Kind { KIND_MODEL = 0, KIND_COST = 1 };                 // ids count from ISLS_{MODEL,COST}_USER_BASE per kind: every lookup takes it
constexpr int kNone = -1;                                    // the empty slot of a key

// What a kernel of a program is for.  A program holds the roles its key calls for and no others.  The rollout variants are no
// role: a program has one per (JM, OCC) the launch plan can pick (Program::ro).
enum Role {
    ROLE_LIN = 0, ROLE_LOOP, ROLE_STEP, ROLE_MC, ROLE_MPC,   // a user model's own program ...
    ROLE_STEP_TAB,                                           // ... of a table model
    ROLE_EXP, ROLE_VAL,                                      // every program of a cost ...
    ROLE_CON_UPDATE,                                         // ... with constraints
    ROLE_SMP_COST, ROLE_SMP_UPDATE, ROLE_SMP_COST_FB, ROLE_SMP_UPDATE_FB,   // every key with a model: the sampling round, open and closed loop
    ROLE_GRAD,                                               // a gradient program
    ROLE_COUNT
};

struct Program {                                             // one key: a model, a cost, or a (model, cost) pair in one dtype
    struct Variant { int jm, occ, slot; };
    bool tried = false, ok = false;
    std::vector<char> code;
    std::vector<std::string> names, lowered;                 // name expressions and their mangled names
    int slot[ROLE_COUNT];                                    // role -> index in names / functions; -1: the program does not hold it
    std::vector<Variant> ro;                                 // the rollout variants and theirs
    int mdlw = 0;                                            // LDS words of the model (plan_rollout)
    int ntab = 0;                                            // words per step of the cost's table (its side records enter the plan too)
    int mtab = 0;                                            // ... and of the user model's table (likewise)
    int field_cost = kNone, dtype = 0;                       // the cost whose field descriptor the program's module holds (kNone: none), in dtype
    std::map<int, std::pair<hipModule_t, std::vector<hipFunction_t>>> dev;   // device -> module, functions
    Program() { for (int &k : slot) k = -1; }
};

// A program on the current device (prepare): its kernels by role; NULL for one the program does not hold, which launch answers
// with ISLS_ERR_UNSUPPORTED.
struct Kernels {
    const Program *pg = nullptr;
    const std::vector<hipFunction_t> *fns = nullptr;
    hipFunction_t at(int slot) const { return slot < 0 ? nullptr : (*fns)[slot]; }
    hipFunction_t of(Role role) const { return at(pg->slot[role]); }
    hipFunction_t rollout(int jm, int occ) const
    {
        for (const auto &v : pg->ro)
            if (v.jm == jm && v.occ == occ) return at(v.slot);
        return nullptr;
    }
};

// isls_user_{model,cost}_create: register `source` (an id is assigned even when the compile fails) and compile its own program
// (the model's, or the cost's expansion and value) for fp64; n_tab: words per step of the source's table (0: none); n_con: path
// constraints of a cost, whose n_tab counts n_con multipliers and mu behind the user's words (ISLS_ERR_UNSUPPORTED: n_tab < n_con + 1)
// n_field = C > 0: a cost that reads a 2-D field of C channels of nx x ny samples (user_field.hpp); ISLS_ERR_UNSUPPORTED: C outside
// [1, 4], nx or ny < 4, C nx ny > 2^24, a model
int create(Kind kind, const char *source, int n, int m, int n_par, int n_tab, int32_t *id, int n_con = 0, int n_field = 0, int nx = 0,
           int ny = 0);
// The field of a cost registered with one.  set_field: `values` [C, nx, ny] on the current device, of `dtype`, into the two sample
// buffers (fp64 and fp32) the registration owns on that device -- allocated at the first call there, overwritten in place on stream
// `s` by every later one -- and origin, 1 / spacing into the descriptor of every module of the cost on the device (only when they
// differ from what stands: a same-grid set_field touches no descriptor).  Modules loaded later get the descriptor as they load.
// ISLS_ERR_ARG: no such cost, a cost without a field, values / origin / spacing NULL, a spacing <= 0 or not finite.
// field_dims: C, nx, ny (0, 0, 0: a cost without a field).  field_ptr: the sample buffer of `dtype` on the current device (NULL: not set).
int set_field(int cost, const void *values, int dtype, const double *origin, const double *spacing, hipStream_t s);
int field_dims(int cost, int *C, int *nx, int *ny);
int field_ptr(int cost, int dtype, void **ptr);
// Frees the sample buffers of the cost's field on every device (the registration itself, its programs and modules stay): the
// field is then set nowhere, and the next set_field allocates again and rewrites the descriptors.  ISLS_ERR_ARG: no such cost, a
// cost without a field.
int release_field(int cost);
// isls_user_*_log / _code / _load: the compiler's messages for a source so far; the code object of a key, compiled on first use;
// the same loaded onto the current device
int64_t copy_log(Kind kind, int id, char *buf, int64_t len);
int copy_code(int model, int cost, int dtype, void *buf, int64_t *len);
int load(int model, int cost, int dtype);
int dims(Kind kind, int id, int *n, int *m);                 // ISLS_ERR_ARG: no such id
int n_tab(int cost);                                         // words per step of the cost's table (0: none); ISLS_ERR_ARG: no such id
int n_con(int cost);                                         // constraints of the cost (0: none); ISLS_ERR_ARG: no such id
int model_n_tab(int model);                                  // the same of a user model's table; 0 for every built-in model
// A launch's model parameters against a table model's registration, before anything is compiled, loaded or launched (no GPU
// needed): a model with P parameters and a table of W words per step takes [par (P) | row 0 | ... | row N-1] -- par != NULL and
// par_sb == 0 (one block for the batch) or P + N * W (one per trajectory); rows_min < N: a buffer that need only reach that many
// rows (the plant of isls_mpc_step: row 0), par_sb == 0 or >= P + rows_min * W.  ISLS_ERR_ARG otherwise; any other model: ISLS_OK.
int check_model_table(int model, int N, const void *par, int64_t par_sb, int rows_min = -1);
// A launch's table fields against the cost's registration, before anything is compiled, loaded or launched (no GPU needed): a
// cost with a table of W words needs tab != NULL, tab_sb == 0 or N * W, and nvia == W (nvia < 0: not given); the fields of a cost
// without a table are ignored.  ISLS_ERR_ARG otherwise, and for an id nobody registered.
int check_table(int cost, int N, const void *tab, int64_t tab_sb, int nvia);
// The program of the key for a launch of dims (n, m) on the current device: compiled and loaded on first use -- never inside a
// capture of stream `s`.  (kNone, cost) asks for the cost's own kernels, which every program of the cost holds: one that is on
// this device already serves, the cost's own program is compiled only when there is none.
int prepare(int model, int cost, int dtype, int n, int m, hipStream_t s, Kernels *k);
// `grid` workgroups of `lanes` lanes; ISLS_ERR_UNSUPPORTED: no such kernel (f == NULL); grid <= 0: nothing to launch
int launch(hipFunction_t f, int grid, size_t smem, hipStream_t s, void **args, int lanes = kWave);
// The gradient program of a model or a cost (user_grad.hpp; one per source and dtype, apart from every key above): grad_build
// compiles it on first request (no GPU needed; ISLS_ERR_COMPILE with the log and the sentence on the contract in the source's
// log).  grad_prepare: the registration's n_par, the user's words per row n_row and the table's words per row n_tab (a cost with
// constraints: n_row + n_con + 1) and, fn != NULL, the kernel on the current device, compiled and loaded on first use.
int grad_build(Kind kind, int id, int dtype);
int grad_prepare(Kind kind, int id, int dtype, int n, int m, hipStream_t s, hipFunction_t *fn, int *n_par, int *n_row, int *n_tab);

template <typename T>
constexpr int dtype_of() { return sizeof(T) == 8 ? ISLS_DTYPE_F64 : ISLS_DTYPE_F32; }

}  // namespace urtc
}  // namespace isls
