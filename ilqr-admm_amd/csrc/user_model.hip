// user_model.hip -- user-written forward models: run-time compilation (hiprtc, gfx950), the registry of compiled models, module
// loading and the launches of their kernels (the device side is user_model.hpp).
//
// One hiprtc program per (model, dtype) holds every rollout_kernel variant the launch plan can pick for the model's (n, m), the
// linearisation, the dense closed loop and the row-wise step.  The rollout launch takes its plan from plan_rollout -- the very
// function the built-in families launch with -- and differs only in how it starts the kernel (hipModuleLaunchKernel of the
// matching instantiation in the model's module instead of hipLaunchKernelGGL).
#ifndef _GNU_SOURCE
#define _GNU_SOURCE                                          // dlmopen
#endif
#include <dlfcn.h>
#include <hip/hiprtc.h>

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rollout_kernel.hpp"
#include "user_rtc.hpp"

#ifndef ISLS_ROCM_PATH
#define ISLS_ROCM_PATH "/opt/rocm"                           // the Makefile passes the ROCm of its hipcc
#endif

namespace isls {

namespace {

// ---- hiprtc, dlopen-ed on the first create -------------------------------------------------------------------------------
struct Rtc {
    bool ok = false;
    hiprtcResult (*create)(hiprtcProgram *, const char *, const char *, int, const char *const *, const char *const *);
    hiprtcResult (*add_name)(hiprtcProgram, const char *);
    hiprtcResult (*compile)(hiprtcProgram, int, const char *const *);
    hiprtcResult (*log_size)(hiprtcProgram, size_t *);
    hiprtcResult (*log)(hiprtcProgram, char *);
    hiprtcResult (*code_size)(hiprtcProgram, size_t *);
    hiprtcResult (*code)(hiprtcProgram, char *);
    hiprtcResult (*lowered)(hiprtcProgram, const char *, const char **);
    hiprtcResult (*destroy)(hiprtcProgram *);
};

std::string dir_of(const void *addr)
{
    Dl_info info;
    if (!dladdr(addr, &info) || !info.dli_fname) return std::string();
    std::string f = info.dli_fname;
    const size_t k = f.rfind('/');
    return k == std::string::npos ? std::string(".") : f.substr(0, k);
}

const Rtc &rtc()
{
    static Rtc r;
    static std::once_flag once;
    std::call_once(once, [] {
        // The hiprtc of the ROCm whose hipcc built this library comes first, in a link namespace of its own: a process may hold
        // another hiprtc and comgr already (PyTorch ships its own, built on another LLVM), and the code of a user model must
        // come from the compiler that built the built-in kernels -- same instructions for the same template, same register
        // allocation.  Then the ROCm of $ROCM_PATH, then whatever the loader finds.
        void *h = nullptr;
        std::vector<std::string> own = {ISLS_ROCM_PATH "/lib/libhiprtc.so"};
        if (const char *rp = getenv("ROCM_PATH")) own.push_back(std::string(rp) + "/lib/libhiprtc.so");
        for (const auto &n : own)
            if ((h = dlmopen(LM_ID_NEWLM, n.c_str(), RTLD_NOW | RTLD_LOCAL)) != nullptr) break;
        const std::string hipdir = dir_of(reinterpret_cast<const void *>(&hipModuleLoadData));   // next to the HIP runtime
        for (const std::string &n : {std::string("libhiprtc.so"), std::string("libhiprtc.so.7"), hipdir + "/libhiprtc.so"}) {
            if (h) break;
            h = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
        }
        if (!h) return;
        bool all = true;
        auto sym = [&](auto &fp, const char *name) {
            fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(h, name));
            all = all && fp != nullptr;
        };
        sym(r.create, "hiprtcCreateProgram");
        sym(r.add_name, "hiprtcAddNameExpression");
        sym(r.compile, "hiprtcCompileProgram");
        sym(r.log_size, "hiprtcGetProgramLogSize");
        sym(r.log, "hiprtcGetProgramLog");
        sym(r.code_size, "hiprtcGetCodeSize");
        sym(r.code, "hiprtcGetCode");
        sym(r.lowered, "hiprtcGetLoweredName");
        sym(r.destroy, "hiprtcDestroyProgram");
        r.ok = all;
    });
    return r;
}

// ---- the registry ----------------------------------------------------------------------------------------------------------
enum Fn { FN_LIN = 0, FN_LOOP, FN_STEP, FN_RO };             // FN_RO + variant: the rollout kernels

using urtc::Program;

struct UserModel {
    std::string source;
    int n, m, npar;
    std::string log;
    Program prog[2];                                         // ISLS_DTYPE_F64, ISLS_DTYPE_F32
};

std::mutex g_mu;
std::vector<std::unique_ptr<UserModel>> g_models;

UserModel *find(int id)
{
    const int k = id - ISLS_MODEL_USER_BASE;
    return (k >= 0 && k < (int)g_models.size()) ? g_models[k].get() : nullptr;
}

bool contains_word(const std::string &s, const char *w)
{
    const size_t lw = strlen(w);
    for (size_t k = s.find(w); k != std::string::npos; k = s.find(w, k + 1)) {
        const bool l = k == 0 || !(isalnum((unsigned char)s[k - 1]) || s[k - 1] == '_');
        const bool r = k + lw >= s.size() || !(isalnum((unsigned char)s[k + lw]) || s[k + lw] == '_');
        if (l && r) return true;
    }
    return false;
}

// compile one dtype (caller holds g_mu)
int compile(UserModel &um, int dtype)
{
    Program &pg = um.prog[dtype];
    if (pg.tried) return pg.ok ? ISLS_OK : ISLS_ERR_COMPILE;
    const char *T = dtype == ISLS_DTYPE_F64 ? "double" : "float";
    const std::string dims = std::to_string(um.n) + ", " + std::to_string(um.m);
    pg.names = {std::string("isls::user_linearize_kernel<") + T + ", " + dims + ">",
                std::string("isls::dense_closed_loop_kernel<") + T + ", " + dims + ", " + std::to_string(ISLS_MODEL_USER) + ">",
                std::string("isls::user_step_kernel<") + T + ", " + dims + ">"};
    urtc::ro_variants_of(um.n, um.m, pg.ro);
    for (const auto &jo : pg.ro)
        pg.names.push_back(std::string("isls::rollout_kernel<") + T + ", " + dims + ", " + std::to_string(ISLS_MODEL_USER) + ", " +
                           std::to_string(jo.first) + ", " + std::to_string(jo.second) + ">");
    const std::string src = "#include \"user_model_ad.hpp\"\n" + urtc::wrap_source("isls_user", "user_model", um.source) +
                            "#define ISLS_USER_NPAR " + std::to_string(um.npar) + "\n#include \"user_model.hpp\"\n";
    return urtc::compile_program(src, "user_model.hip", pg, um.log);
}

// the model's functions on the current device: compiled and loaded on first use (caller holds g_mu)
int functions(UserModel &um, int dtype, const std::vector<hipFunction_t> **out, hipStream_t capture_check)
{
    const int rc = compile(um, dtype);
    if (rc != ISLS_OK) return rc;
    return urtc::load_program(um.prog[dtype], out, capture_check);
}

using urtc::dtype_of;
using urtc::launch;

// look up model `id` for a launch of dims (n, m) and get its functions
template <typename T>
int prepare(int id, int n, int m, hipStream_t s, UserModel **um, const std::vector<hipFunction_t> **fns)
{
    std::lock_guard<std::mutex> lk(g_mu);
    *um = find(id);
    if (!*um) return ISLS_ERR_ARG;
    if ((*um)->n != n || (*um)->m != m) return ISLS_ERR_ARG;
    return functions(**um, dtype_of<T>(), fns, s);
}

}  // namespace

// ---- what user_cost.hip shares (user_rtc.hpp) --------------------------------------------------------------------------------
namespace urtc {

bool refused_source(const std::string &src)
{
    return contains_word(src, "asm") || contains_word(src, "__asm") || contains_word(src, "__asm__") ||
           src.find("__builtin_amdgcn") != std::string::npos;
}

std::string wrap_source(const std::string &ns, const std::string &label, const std::string &body)
{
    return "namespace " + ns + " {\n#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)\n#line 1 \"" +
           label + "\"\n" + body + "\n#pragma clang attribute pop\n}  // namespace " + ns + "\n";
}

int compile_program(const std::string &src, const char *file, Program &pg, std::string &log)
{
    if (pg.tried) return pg.ok ? ISLS_OK : ISLS_ERR_COMPILE;
    pg.tried = true;
    const Rtc &r = rtc();
    if (!r.ok) {
        log += "libhiprtc.so could not be loaded: user models and costs need hiprtc (ROCm)\n";
        return ISLS_ERR_COMPILE;
    }
    const std::string csrc = dir_of(reinterpret_cast<const void *>(&find));
    hiprtcProgram prog;
    if (r.create(&prog, src.c_str(), file, 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        log += "hiprtcCreateProgram failed\n";
        return ISLS_ERR_COMPILE;
    }
    for (const auto &nm : pg.names) r.add_name(prog, nm.c_str());
    // the flags of the Makefile's build of the built-in kernels (-O3 -std=c++17, clang's HIP default contraction): the same
    // template gives the same instructions, so a user model that restates a built-in one gets its bits
    const std::string inc = "-I" + csrc;
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast-honor-pragmas", inc.c_str()};
    const hiprtcResult cr = r.compile(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    size_t ls = 0;
    if (r.log_size(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        std::string lg(ls, '\0');
        if (r.log(prog, &lg[0]) == HIPRTC_SUCCESS) log += lg.c_str();
    }
    bool ok = cr == HIPRTC_SUCCESS;
    size_t cs = 0;
    if (ok && r.code_size(prog, &cs) == HIPRTC_SUCCESS && cs > 0) {
        pg.code.resize(cs);
        ok = r.code(prog, pg.code.data()) == HIPRTC_SUCCESS;
    } else {
        ok = false;
    }
    pg.lowered.clear();
    for (const auto &nm : pg.names) {
        const char *low = nullptr;
        if (!ok || r.lowered(prog, nm.c_str(), &low) != HIPRTC_SUCCESS || !low) {
            ok = false;
            break;
        }
        pg.lowered.push_back(low);
    }
    r.destroy(&prog);
    pg.ok = ok;
    if (!ok) pg.code.clear();
    return ok ? ISLS_OK : ISLS_ERR_COMPILE;
}

int load_program(Program &pg, const std::vector<hipFunction_t> **out, hipStream_t capture_check)
{
    if (!pg.ok) return ISLS_ERR_COMPILE;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ISLS_ERR_LAUNCH;
    auto it = pg.dev.find(dev);
    if (it == pg.dev.end()) {
        if (capture_check) {                                 // no module load inside a stream capture: load first
            hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(capture_check, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return ISLS_ERR_LAUNCH;
        }
        hipModule_t mod;
        if (hipModuleLoadData(&mod, pg.code.data()) != hipSuccess) return ISLS_ERR_LAUNCH;
        std::vector<hipFunction_t> fns(pg.lowered.size());
        for (size_t i = 0; i < fns.size(); ++i)
            if (hipModuleGetFunction(&fns[i], mod, pg.lowered[i].c_str()) != hipSuccess) {
                hipModuleUnload(mod);
                return ISLS_ERR_LAUNCH;
            }
        it = pg.dev.emplace(dev, std::make_pair(mod, std::move(fns))).first;
    }
    *out = &it->second.second;
    return ISLS_OK;
}

int launch(hipFunction_t f, int grid, size_t smem, hipStream_t s, void **args)
{
    if (grid <= 0) return ISLS_OK;
    return hipModuleLaunchKernel(f, grid, 1, 1, 64, 1, 1, (unsigned)smem, s, args, nullptr) == hipSuccess ? ISLS_OK : ISLS_ERR_LAUNCH;
}

int user_model_info(int id, std::string *source, int *n, int *m, int *npar)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const UserModel *um = find(id);
    if (!um) return ISLS_ERR_ARG;
    if (source) *source = um->source;
    if (n) *n = um->n;
    if (m) *m = um->m;
    if (npar) *npar = um->npar;
    return ISLS_OK;
}

}  // namespace urtc

// ---- launches (dispatched from rollout.hip / misc.hip on a.model >= ISLS_MODEL_USER_BASE) -----------------------------------
template <typename T>
int launch_rollout_user(RoP<T> &p, const isls_rollout_args &a, hipStream_t s, bool want_fused)
{
    UserModel *um;
    const std::vector<hipFunction_t> *fns;
    int rc = prepare<T>(a.model, a.n, a.m, s, &um, &fns);
    if (rc != ISLS_OK) return rc;
    RoLaunch pl;
    rc = ISLS_ERR_UNSUPPORTED;
#define ISLS_UM_PLAN_(NX_, NU_) if (a.n == NX_ && a.m == NU_) rc = plan_rollout<T, NX_, NU_, 0>(p, a, want_fused, nullptr, pl);
    ISLS_FOR_EACH_DIMS(ISLS_UM_PLAN_)
#undef ISLS_UM_PLAN_
    if (rc != ISLS_OK) return rc;
    const Program &pg = um->prog[dtype_of<T>()];
    for (size_t i = 0; i < pg.ro.size(); ++i)
        if (pg.ro[i].first == pl.jm && pg.ro[i].second == pl.occ) {
            void *args[] = {&p};
            return launch((*fns)[FN_RO + i], pl.grid, pl.smem, s, args);
        }
    return ISLS_ERR_UNSUPPORTED;
}
template int launch_rollout_user<double>(RoP<double> &, const isls_rollout_args &, hipStream_t, bool);
template int launch_rollout_user<float>(RoP<float> &, const isls_rollout_args &, hipStream_t, bool);

template <typename T>
int launch_linearize_user(const isls_linearize_args &a, hipStream_t s)
{
    if (a.B < 0 || a.N < 1 || !a.model_par || !a.A || !a.Bm || !a.xhat || !a.uhat) return ISLS_ERR_ARG;
    if (a.B == 0) return ISLS_OK;
    UserModel *um;
    const std::vector<hipFunction_t> *fns;
    const int rc = prepare<T>(a.model, a.n, a.m, s, &um, &fns);
    if (rc != ISLS_OK) return rc;
    const int steps = kWave / (a.n + a.m);                   // steps per workgroup (user_linearize_kernel's S)
    UserLinP<T> p;
    p.B = a.B; p.N = a.N; p.nbt = (a.N + steps - 1) / steps;
    p.par = (const T *)a.model_par; p.par_sb = a.model_par_sb;
    p.xhat = (const T *)a.xhat; p.uhat = (const T *)a.uhat; p.A = (T *)a.A; p.Bm = (T *)a.Bm; p.active = a.active;
    const int64_t grid = (int64_t)a.B * p.nbt;
    if (grid > 0x7fffffff) return ISLS_ERR_UNSUPPORTED;
    void *args[] = {&p};
    return launch((*fns)[FN_LIN], (int)grid, 0, s, args);
}
template int launch_linearize_user<double>(const isls_linearize_args &, hipStream_t);
template int launch_linearize_user<float>(const isls_linearize_args &, hipStream_t);

template <typename T>
int launch_dense_closed_loop_user(const DenseLoopP<T> &p0, const isls_dense_loop_args &a, hipStream_t s)
{
    UserModel *um;
    const std::vector<hipFunction_t> *fns;
    const int rc = prepare<T>(a.model, a.n, a.m, s, &um, &fns);
    if (rc != ISLS_OK) return rc;
    DenseLoopP<T> p = p0;
    void *args[] = {&p};
    return launch((*fns)[FN_LOOP], (a.M + 63) / 64, sizeof(T), s, args);
}
template int launch_dense_closed_loop_user<double>(const DenseLoopP<double> &, const isls_dense_loop_args &, hipStream_t);
template int launch_dense_closed_loop_user<float>(const DenseLoopP<float> &, const isls_dense_loop_args &, hipStream_t);

template <typename T>
static int user_step(int32_t id, int32_t R, const void *par, int64_t par_sb, const void *x, const void *u, void *xn, hipStream_t s)
{
    if (R < 0 || !par || !x || !u || !xn || par_sb < 0) return ISLS_ERR_ARG;
    int n, m;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const UserModel *um = find(id);
        if (!um) return ISLS_ERR_ARG;
        n = um->n; m = um->m;
    }
    if (R == 0) return ISLS_OK;
    UserModel *um;
    const std::vector<hipFunction_t> *fns;
    const int rc = prepare<T>(id, n, m, s, &um, &fns);
    if (rc != ISLS_OK) return rc;
    int R_ = R;
    const T *par_ = (const T *)par, *x_ = (const T *)x, *u_ = (const T *)u;
    T *xn_ = (T *)xn;
    void *args[] = {&R_, &par_, &par_sb, &x_, &u_, &xn_};
    return launch((*fns)[FN_STEP], (R + 63) / 64, 0, s, args);
}

}  // namespace isls

using namespace isls;

#define ISLS_API extern "C" __attribute__((visibility("default")))

ISLS_API int isls_user_model_create(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t *id)
{
    if (!source || !id) return ISLS_ERR_ARG;
    if (!dims_supported(n, m) || n_par < 0 || n_par > ISLS_USER_MAX_PAR) return ISLS_ERR_UNSUPPORTED;
    const std::string src(source);
    // a model is plain arithmetic: no hand-written ISA through this door
    if (urtc::refused_source(src)) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    auto um = std::make_unique<UserModel>();
    um->source = src; um->n = n; um->m = m; um->npar = n_par;
    *id = ISLS_MODEL_USER_BASE + (int32_t)g_models.size();
    g_models.push_back(std::move(um));
    return compile(*g_models.back(), ISLS_DTYPE_F64);
}

ISLS_API int64_t isls_user_model_log(int32_t id, char *buf, int64_t len)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const UserModel *um = find(id);
    if (!um) return ISLS_ERR_ARG;
    if (buf && len > 0) {
        const size_t k = um->log.size() < (size_t)(len - 1) ? um->log.size() : (size_t)(len - 1);
        memcpy(buf, um->log.data(), k);
        buf[k] = '\0';
    }
    return (int64_t)um->log.size();
}

ISLS_API int isls_user_model_code(int32_t id, int32_t dtype, void *buf, int64_t *len)
{
    if (!len || (dtype != ISLS_DTYPE_F64 && dtype != ISLS_DTYPE_F32)) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    UserModel *um = find(id);
    if (!um) return ISLS_ERR_ARG;
    const int rc = compile(*um, dtype);
    if (rc != ISLS_OK) return rc;
    const std::vector<char> &code = um->prog[dtype].code;
    const int64_t cap = *len;
    *len = (int64_t)code.size();
    if (buf) {
        if (cap < (int64_t)code.size()) return ISLS_ERR_ARG;
        memcpy(buf, code.data(), code.size());
    }
    return ISLS_OK;
}

ISLS_API int isls_user_model_load(int32_t id, int32_t dtype)
{
    if (dtype != ISLS_DTYPE_F64 && dtype != ISLS_DTYPE_F32) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    UserModel *um = find(id);
    if (!um) return ISLS_ERR_ARG;
    const std::vector<hipFunction_t> *fns;
    return functions(*um, dtype, &fns, nullptr);
}

ISLS_API int isls_user_model_step_f64(int32_t id, int32_t R, const void *par, int64_t par_sb, const void *x, const void *u, void *xn,
                                      void *stream)
{
    return user_step<double>(id, R, par, par_sb, x, u, xn, (hipStream_t)stream);
}
ISLS_API int isls_user_model_step_f32(int32_t id, int32_t R, const void *par, int64_t par_sb, const void *x, const void *u, void *xn,
                                      void *stream)
{
    return user_step<float>(id, R, par, par_sb, x, u, xn, (hipStream_t)stream);
}
