// user_cost.hip -- user-written cost functions: the registry of compiled costs, their run-time compiled programs and the launches
// of their kernels (the device side is user_cost.hpp; hiprtc, module loading and the launcher are user_model.hip's, user_rtc.hpp).
//
// One hiprtc program per (cost, model, dtype): the model is a built-in id -- the program then instantiates the built-in family's
// rollout_kernel with the user's stage cost in it -- or a user model, whose source goes into the same program.  A program holds
// every (JM, OCC) variant the launch plan can pick for the pair's (n, m), user_expand_kernel and user_cost_value_kernel.  The
// rollout launch takes its plan from plan_rollout, the function the built-in families launch with.
#include <cstring>
#include <memory>
#include <mutex>

#include "user_rtc.hpp"

namespace isls {

namespace {

enum Fn { FN_EXP = 0, FN_VAL, FN_RO };                       // FN_RO + variant: the rollout kernels

struct CostProgram {
    urtc::Program prog[2];                                   // ISLS_DTYPE_F64, ISLS_DTYPE_F32
    int mdlw = 0;                                            // LDS words of the model (plan_rollout)
};

struct UserCost {
    std::string source;
    int n, m, npar;
    std::string log;
    std::map<int, std::unique_ptr<CostProgram>> with;        // model id (built-in or user; -1: no rollout kernels) -> program
};

std::mutex g_cmu;
std::vector<std::unique_ptr<UserCost>> g_costs;

UserCost *find_cost(int id)
{
    const int k = id - ISLS_COST_USER_BASE;
    return (k >= 0 && k < (int)g_costs.size()) ? g_costs[k].get() : nullptr;
}

constexpr int kNoModel = -1;

// the built-in family (n, m, model) and its LDS words
bool builtin_family(int n, int m, int model, int *mdlw)
{
#define ISLS_UC_FAMILY_(NX_, NU_, MODEL_) \
    if (n == NX_ && m == NU_ && model == MODEL_) { *mdlw = Model<double, NX_, NU_, MODEL_>::LDS_WORDS; return true; }
    ISLS_FOR_EACH_FAMILY(ISLS_UC_FAMILY_)
#undef ISLS_UC_FAMILY_
    return false;
}

// compile the cost with `model` for dtype (caller holds g_cmu)
int compile(UserCost &uc, int model, int dtype, CostProgram **out)
{
    auto &slot = uc.with[model];
    if (!slot) slot = std::make_unique<CostProgram>();
    CostProgram &cp = *slot;
    *out = &cp;
    urtc::Program &pg = cp.prog[dtype];
    if (pg.tried) return pg.ok ? ISLS_OK : ISLS_ERR_COMPILE;
    std::string msrc, prefix;
    int tmodel = model;                                      // the MODEL template argument
    if (model >= ISLS_MODEL_USER_BASE) {
        int n, m, npar;
        if (urtc::user_model_info(model, &msrc, &n, &m, &npar) != ISLS_OK || n != uc.n || m != uc.m) return ISLS_ERR_ARG;
        prefix = urtc::wrap_source("isls_user", "user_model", msrc) + "#define ISLS_USER_NPAR " + std::to_string(npar) + "\n";
        tmodel = ISLS_MODEL_USER;
        cp.mdlw = 0;
    } else if (model != kNoModel && !builtin_family(uc.n, uc.m, model, &cp.mdlw)) {
        return ISLS_ERR_UNSUPPORTED;
    }
    const char *T = dtype == ISLS_DTYPE_F64 ? "double" : "float";
    const std::string dims = std::to_string(uc.n) + ", " + std::to_string(uc.m);
    pg.names = {std::string("isls::user_expand_kernel<") + T + ", " + dims + ">",
                std::string("isls::user_cost_value_kernel<") + T + ", " + dims + ">"};
    pg.ro.clear();
    if (model != kNoModel) urtc::ro_variants_of(uc.n, uc.m, pg.ro);
    for (const auto &jo : pg.ro)
        pg.names.push_back(std::string("isls::rollout_kernel<") + T + ", " + dims + ", " + std::to_string(tmodel) + ", " +
                           std::to_string(jo.first) + ", " + std::to_string(jo.second) + ">");
    const std::string src = "#include \"user_cost_ad.hpp\"\n" + prefix + urtc::wrap_source("isls_user_cost", "user_cost", uc.source) +
                            "#define ISLS_USER_COST_NPAR " + std::to_string(uc.npar) + "\n#include \"user_cost.hpp\"\n";
    return urtc::compile_program(src, "user_cost.hip", pg, uc.log);
}

// look up cost `id` for a launch of dims (n, m) with `model` and get its functions
template <typename T>
int prepare(int id, int model, int n, int m, hipStream_t s, CostProgram **cp, const std::vector<hipFunction_t> **fns)
{
    std::lock_guard<std::mutex> lk(g_cmu);
    UserCost *uc = find_cost(id);
    if (!uc || uc->n != n || uc->m != m) return ISLS_ERR_ARG;
    const int dt = urtc::dtype_of<T>();
    if (model == kNoModel) {
        // expansion / value: every program of the cost holds them.  One that is on this device already serves (the pair the
        // engine loaded); the model-less program is compiled only when there is no such pair
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return ISLS_ERR_LAUNCH;
        for (auto &e : uc->with)
            if (e.second->prog[dt].ok && e.second->prog[dt].dev.count(dev)) { model = e.first; break; }
    }
    const int rc = compile(*uc, model, dt, cp);
    if (rc != ISLS_OK) return rc;
    return urtc::load_program((*cp)->prog[dt], fns, s);
}

}  // namespace

// ---- launches (dispatched from rollout.hip / misc.hip on a.cost_model >= ISLS_COST_USER_BASE) --------------------------------
template <typename T>
int launch_rollout_user_cost(RoP<T> &p, const isls_rollout_args &a, hipStream_t s, bool want_fused)
{
    if (!a.cost_par || a.cost_par_sb < 0) return ISLS_ERR_ARG;
    CostProgram *cp;
    const std::vector<hipFunction_t> *fns;
    int rc = prepare<T>(a.cost_model, a.model, a.n, a.m, s, &cp, &fns);
    if (rc != ISLS_OK) return rc;
    p.cpar_sb = a.cost_par_sb;
    RoLaunch pl;
    rc = ISLS_ERR_UNSUPPORTED;
    // the model enters the plan through its LDS words only (a dense LTI model's [A B]; none for the others and for user models)
#define ISLS_UC_PLAN_(NX_, NU_)                                                                                \
    if (a.n == NX_ && a.m == NU_)                                                                              \
        rc = cp->mdlw ? plan_rollout<T, NX_, NU_, NX_ * (NX_ + NU_)>(p, a, want_fused, nullptr, pl)            \
                      : plan_rollout<T, NX_, NU_, 0>(p, a, want_fused, nullptr, pl);
    ISLS_FOR_EACH_DIMS(ISLS_UC_PLAN_)
#undef ISLS_UC_PLAN_
    if (rc != ISLS_OK) return rc;
    const urtc::Program &pg = cp->prog[urtc::dtype_of<T>()];
    for (size_t i = 0; i < pg.ro.size(); ++i)
        if (pg.ro[i].first == pl.jm && pg.ro[i].second == pl.occ) {
            void *args[] = {&p};
            return urtc::launch((*fns)[FN_RO + i], pl.grid, pl.smem, s, args);
        }
    return ISLS_ERR_UNSUPPORTED;
}
template int launch_rollout_user_cost<double>(RoP<double> &, const isls_rollout_args &, hipStream_t, bool);
template int launch_rollout_user_cost<float>(RoP<float> &, const isls_rollout_args &, hipStream_t, bool);

template <typename T>
static int user_cost_value(int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *x, const void *u, void *cost,
                           const int32_t *active, hipStream_t s)
{
    if (R < 0 || N < 1 || !par || !cost || par_sb < 0) return ISLS_ERR_ARG;
    int n, m;
    {
        std::lock_guard<std::mutex> lk(g_cmu);
        const UserCost *uc = find_cost(id);
        if (!uc) return ISLS_ERR_ARG;
        n = uc->n; m = uc->m;
    }
    if (R == 0) return ISLS_OK;
    CostProgram *cp;
    const std::vector<hipFunction_t> *fns;
    const int rc = prepare<T>(id, kNoModel, n, m, s, &cp, &fns);
    if (rc != ISLS_OK) return rc;
    int R_ = R, N_ = N;
    const T *par_ = (const T *)par, *x_ = (const T *)x, *u_ = (const T *)u;
    T *cost_ = (T *)cost;
    void *args[] = {&R_, &N_, &par_, &par_sb, &x_, &u_, &cost_, &active};
    return urtc::launch((*fns)[FN_VAL], (R + 63) / 64, 0, s, args);
}

template <typename T>
int launch_expand_user_cost(const isls_expand_args &a, void *Cux, hipStream_t s)
{
    if (a.B < 0 || a.N < 1 || !a.c0x || !a.c0u || !a.cost_par || a.cost_par_sb < 0) return ISLS_ERR_ARG;
    if (a.B == 0) return ISLS_OK;
    CostProgram *cp;
    const std::vector<hipFunction_t> *fns;
    int rc = prepare<T>(a.cost_model, kNoModel, a.n, a.m, s, &cp, &fns);
    if (rc != ISLS_OK) return rc;
    const int K = a.n + a.m, NP = K * (K + 1) / 2, steps = NP <= kWave ? kWave / NP : 4;   // user_expand_kernel's S
    UserExpP<T> p;
    p.B = a.B; p.N = a.N; p.nbt = (a.N + steps - 1) / steps;
    p.par = (const T *)a.cost_par; p.par_sb = a.cost_par_sb;
    p.xhat = (const T *)a.xhat; p.uhat = (const T *)a.uhat;
    p.Qr = View<T>(a.Qr); p.Rr = View<T>(a.Rr);
    p.Cxx = (T *)a.Cxx; p.Cuu = (T *)a.Cuu; p.Cux = (T *)Cux; p.c0x = (T *)a.c0x; p.c0u = (T *)a.c0u;
    p.active = a.active;
    const int64_t grid = (int64_t)a.B * p.nbt;
    if (grid > 0x7fffffff) return ISLS_ERR_UNSUPPORTED;
    void *args[] = {&p};
    if ((rc = urtc::launch((*fns)[FN_EXP], (int)grid, 0, s, args)) != ISLS_OK || !a.cost) return rc;
    return user_cost_value<T>(a.cost_model, a.B, a.N, a.cost_par, a.cost_par_sb, a.xhat, a.uhat, a.cost, a.active, s);
}
template int launch_expand_user_cost<double>(const isls_expand_args &, void *, hipStream_t);
template int launch_expand_user_cost<float>(const isls_expand_args &, void *, hipStream_t);

}  // namespace isls

using namespace isls;

#define ISLS_API extern "C" __attribute__((visibility("default")))

ISLS_API int isls_user_cost_create(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t *id)
{
    if (!source || !id) return ISLS_ERR_ARG;
    if (!dims_supported(n, m) || n_par < 0 || n_par > ISLS_USER_MAX_PAR) return ISLS_ERR_UNSUPPORTED;
    const std::string src(source);
    if (urtc::refused_source(src)) return ISLS_ERR_ARG;     // a cost is plain arithmetic: no hand-written ISA through this door
    std::lock_guard<std::mutex> lk(g_cmu);
    auto uc = std::make_unique<UserCost>();
    uc->source = src; uc->n = n; uc->m = m; uc->npar = n_par;
    *id = ISLS_COST_USER_BASE + (int32_t)g_costs.size();
    g_costs.push_back(std::move(uc));
    CostProgram *cp;
    return compile(*g_costs.back(), kNoModel, ISLS_DTYPE_F64, &cp);   // the expansion and the value: every operation of the source
}

ISLS_API int64_t isls_user_cost_log(int32_t id, char *buf, int64_t len)
{
    std::lock_guard<std::mutex> lk(g_cmu);
    const UserCost *uc = find_cost(id);
    if (!uc) return ISLS_ERR_ARG;
    if (buf && len > 0) {
        const size_t k = uc->log.size() < (size_t)(len - 1) ? uc->log.size() : (size_t)(len - 1);
        memcpy(buf, uc->log.data(), k);
        buf[k] = '\0';
    }
    return (int64_t)uc->log.size();
}

ISLS_API int isls_user_cost_code(int32_t id, int32_t model, int32_t dtype, void *buf, int64_t *len)
{
    if (!len || (dtype != ISLS_DTYPE_F64 && dtype != ISLS_DTYPE_F32)) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_cmu);
    UserCost *uc = find_cost(id);
    if (!uc) return ISLS_ERR_ARG;
    CostProgram *cp;
    const int rc = compile(*uc, model < 0 ? kNoModel : model, dtype, &cp);
    if (rc != ISLS_OK) return rc;
    const std::vector<char> &code = cp->prog[dtype].code;
    const int64_t cap = *len;
    *len = (int64_t)code.size();
    if (buf) {
        if (cap < (int64_t)code.size()) return ISLS_ERR_ARG;
        memcpy(buf, code.data(), code.size());
    }
    return ISLS_OK;
}

ISLS_API int isls_user_cost_load(int32_t id, int32_t model, int32_t dtype)
{
    if (dtype != ISLS_DTYPE_F64 && dtype != ISLS_DTYPE_F32) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_cmu);
    UserCost *uc = find_cost(id);
    if (!uc) return ISLS_ERR_ARG;
    CostProgram *cp;
    const int rc = compile(*uc, model < 0 ? kNoModel : model, dtype, &cp);
    if (rc != ISLS_OK) return rc;
    const std::vector<hipFunction_t> *fns;
    return urtc::load_program(cp->prog[dtype], &fns, nullptr);
}

ISLS_API int isls_user_cost_value_f64(int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *x, const void *u,
                                      void *cost, void *stream)
{
    return user_cost_value<double>(id, R, N, par, par_sb, x, u, cost, nullptr, (hipStream_t)stream);
}
ISLS_API int isls_user_cost_value_f32(int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *x, const void *u,
                                      void *cost, void *stream)
{
    return user_cost_value<float>(id, R, N, par, par_sb, x, u, cost, nullptr, (hipStream_t)stream);
}

ISLS_API int isls_user_cost_expand_f64(const isls_expand_args *a, void *Cux, void *stream)
{
    if (!a || !is_user_cost(a->cost_model)) return ISLS_ERR_ARG;
    return launch_expand_user_cost<double>(*a, Cux, (hipStream_t)stream);
}
ISLS_API int isls_user_cost_expand_f32(const isls_expand_args *a, void *Cux, void *stream)
{
    if (!a || !is_user_cost(a->cost_model)) return ISLS_ERR_ARG;
    return launch_expand_user_cost<float>(*a, Cux, (hipStream_t)stream);
}
