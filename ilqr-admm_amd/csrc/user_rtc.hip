// user_rtc.hip -- run-time compilation (hiprtc, gfx950) for user-written models and costs: the hiprtc loader, the registry of
// sources, the cache of compiled programs, module loading and the line-search launch (user_rtc.hpp; the device side is
// user_model.hpp / user_cost.hpp, the launches of a model's and a cost's own kernels are user_model.hip / user_cost.hip).
//
// One hiprtc program per (model, cost, dtype).  (user model, none) holds the model's own kernels, (none, cost) the cost's,
// (model, cost) -- the model a built-in id or a user model, whose source goes into the same program -- the cost's again; and
// every key with a model holds each rollout_kernel variant the launch plan can pick for its (n, m) and the sampling round.
// program() registers every kernel under its Role (user_rtc.hpp) or its (JM, OCC), and a launch asks for it by that: where a
// name expression lies is written down nowhere else.  The rollout launch takes its plan from plan_rollout -- the very function
// the built-in families launch with -- and differs only in how it starts the kernel (hipModuleLaunchKernel of the matching
// instantiation in the key's module instead of hipLaunchKernelGGL).
#ifndef _GNU_SOURCE
#define _GNU_SOURCE                                          // dlmopen
#endif
#include <dlfcn.h>
#include <unistd.h>
#include <hip/hiprtc.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <tuple>

#include "user_rtc.hpp"
#include "user_field.hpp"                                    // FieldDesc: the descriptor a module of a field cost holds

#ifndef ISLS_ROCM_PATH
#define ISLS_ROCM_PATH "/opt/rocm"                           // the Makefile passes the ROCm of its hipcc
#endif

namespace isls {
namespace urtc {

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
    char ***env = nullptr;                                   // `environ` of the C library in hiprtc's link namespace (its own copy)
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
        r.env = reinterpret_cast<char ***>(dlsym(h, "environ"));
        r.ok = all;
    });
    return r;
}

// ---- sources and their compilation -------------------------------------------------------------------------------------------
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

// a user source is plain arithmetic: true when it holds `asm` (any spelling) or `__builtin_amdgcn`
bool refused_source(const std::string &src)
{
    return contains_word(src, "asm") || contains_word(src, "__asm") || contains_word(src, "__asm__") ||
           src.find("__builtin_amdgcn") != std::string::npos;
}

// `body` inside `namespace ns`, every function of it always_inline (a call that is not inlined would take its arrays through
// scratch memory), compiler messages pointing at `label`:<line of the user's text>
std::string wrap_source(const std::string &ns, const std::string &label, const std::string &body)
{
    return "namespace " + ns + " {\n#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)\n#line 1 \"" +
           label + "\"\n" + body + "\n#pragma clang attribute pop\n}  // namespace " + ns + "\n";
}

// Compile `src` (file name `file` in the messages) for gfx950 with pg.names as name expressions; fills pg.code / pg.lowered,
// appends the compiler's log to `log`.  Once per Program (pg.tried).
int compile_program(const std::string &src, const char *file, Program &pg, std::string &log)
{
    if (pg.tried) return pg.ok ? ISLS_OK : ISLS_ERR_COMPILE;
    pg.tried = true;
    const Rtc &r = rtc();
    if (!r.ok) {
        log += "libhiprtc.so could not be loaded: user models and costs need hiprtc (ROCm)\n";
        return ISLS_ERR_COMPILE;
    }
    const std::string csrc = dir_of(reinterpret_cast<const void *>(&rtc));   // the device headers lie next to the library
    // A link namespace of its own has a C library of its own, and that one keeps the environment pointer of the moment it was
    // loaded.  A setenv in the process since then reallocates the array: the compiler's getenv calls would walk a freed block
    // (seen as a segmentation fault in the first compile after os.environ had grown).  Hand it the current array.
    if (r.env && r.env != &environ) *r.env = environ;
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

int write_field(const Program &pg, int dev, hipModule_t mod);   // (below, with the registry)

// the program's functions (in the order of pg.names) on the current device, loaded on first use -- never inside a stream capture
// (capture_check: the stream to test, or nullptr); a module of a field cost gets the field's descriptor where the field is set
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
        if (write_field(pg, dev, mod) != ISLS_OK) {
            hipModuleUnload(mod);
            return ISLS_ERR_LAUNCH;
        }
        it = pg.dev.emplace(dev, std::make_pair(mod, std::move(fns))).first;
    }
    if (out) *out = &it->second.second;
    return ISLS_OK;
}

// ---- the registry and the program cache (both under g_mu) --------------------------------------------------------------------
struct Source {
    std::string source;
    int n, m, npar, ntab;                                    // ntab: words per step of the source's table (0: none)
    int ncon = 0;                                            // path constraints of a cost (ntab then counts their multipliers and mu)
    // the field of a cost (user_field.hpp): C channels of nx x ny samples; per device the two sample buffers the registration
    // owns and the origin and 1 / spacing that stand in the descriptors there (set: isls_user_cost_set_field has been there)
    struct FieldDev {
        void *v64 = nullptr, *v32 = nullptr;
        double org[2] = {0, 0}, inv[2] = {0, 0};
        bool set = false;
    };
    int nfield = 0, fnx = 0, fny = 0;
    std::map<int, FieldDev> fdev;
    std::string log;
};

std::mutex g_mu;
std::vector<std::unique_ptr<Source>> g_src[2];               // [Kind]: id - ISLS_{MODEL,COST}_USER_BASE -> source
std::map<std::tuple<int, int, int>, Program> g_prog;         // (cost, dtype, model) -> program: the programs of a cost lie together

Source *find(Kind kind, int id)
{
    const int k = id - (kind == KIND_MODEL ? ISLS_MODEL_USER_BASE : ISLS_COST_USER_BASE);
    return (k >= 0 && k < (int)g_src[kind].size()) ? g_src[kind][k].get() : nullptr;
}

// ---- the field of a cost: its descriptor in the modules, its samples in the registration's buffers ----------------------------
template <typename T>
int write_field_as(const Source &src, const Source::FieldDev &fd, hipModule_t mod)
{
    hipDeviceptr_t sym = nullptr;
    size_t bytes = 0;
    const hipError_t e = hipModuleGetGlobal(&sym, &bytes, mod, "isls_user_cost_field");
    if (e == hipErrorNotFound) return ISLS_OK;               // a source that never reads its field: the compiler kept no descriptor
    if (e != hipSuccess || bytes != sizeof(FieldDesc<T>)) return ISLS_ERR_LAUNCH;
    FieldDesc<T> d;
    d.set((const T *)(sizeof(T) == 8 ? fd.v64 : fd.v32), src.fnx, src.fny, fd.org, fd.inv);
    return hipMemcpyHtoD(sym, &d, sizeof(d)) == hipSuccess ? ISLS_OK : ISLS_ERR_LAUNCH;
}

// the descriptor of pg's module `mod` on device `dev`: written where the program is a field cost's and the field is set there
int write_field(const Program &pg, int dev, hipModule_t mod)
{
    const Source *src = pg.field_cost != kNone ? find(KIND_COST, pg.field_cost) : nullptr;
    if (!src || src->nfield == 0) return ISLS_OK;
    const auto it = src->fdev.find(dev);
    if (it == src->fdev.end() || !it->second.set) return ISLS_OK;   // set_field writes it when it comes
    return pg.dtype == ISLS_DTYPE_F64 ? write_field_as<double>(*src, it->second, mod) : write_field_as<float>(*src, it->second, mod);
}

// ISLS_ERR_ARG for a launch of a field cost on a device its field was never set on, before anything is compiled, loaded or launched
int check_field(const Source *uc)
{
    if (!uc || uc->nfield == 0) return ISLS_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ISLS_ERR_LAUNCH;
    const auto it = uc->fdev.find(dev);
    return it != uc->fdev.end() && it->second.set ? ISLS_OK : ISLS_ERR_ARG;
}

template <typename From, typename To>
__global__ __launch_bounds__(256) void field_convert_kernel(const From *src, To *dst, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (To)src[i];
}

// the (JM, OCC) variants the launch plan of these dimensions can pick
template <int NX, int NU>
void ro_variants(std::vector<std::pair<int, int>> &v)
{
    for (int occ = 2; occ >= 1; --occ)
        for (int i = 0; i < (occ == 2 ? 3 : 4); ++i) {
            const std::pair<int, int> jo(ro_jm_variant<NX, NU>(occ, i), occ);
            bool seen = false;
            for (const auto &e : v) seen = seen || e == jo;
            if (!seen) v.push_back(jo);
        }
}

// The text of a program: the dual-number header (the cost's where there is a cost), the user model and the user cost (either may
// be absent), each in its namespace with the defines of its registration behind it, and the device side `device_hpp` last.
std::string program_text(const Source *um, const Source *uc, const char *device_hpp, int dtype)
{
    std::string src;
    // a cost with a field: isls::field (user_field.hpp) ahead of the source that calls it; the text of every other program is
    // what it was, line for line
    if (uc && uc->nfield > 0)
        src = "#define ISLS_USER_COST_NFIELD " + std::to_string(uc->nfield) + "\n#define ISLS_USER_COST_FIELD_T " +
              (dtype == ISLS_DTYPE_F64 ? "double" : "float") + "\n#include \"user_field.hpp\"\n";
    src += uc ? "#include \"user_cost_ad.hpp\"\n" : "#include \"user_model_ad.hpp\"\n";
    if (um) src += wrap_source("isls_user", "user_model", um->source) + "#define ISLS_USER_NPAR " + std::to_string(um->npar) + "\n";
    if (um && um->ntab > 0) src += "#define ISLS_USER_MODEL_NTAB " + std::to_string(um->ntab) + "\n";
    if (uc) src += wrap_source("isls_user_cost", "user_cost", uc->source) + "#define ISLS_USER_COST_NPAR " + std::to_string(uc->npar) + "\n";
    if (uc && uc->ntab > 0) src += "#define ISLS_USER_COST_NTAB " + std::to_string(uc->ntab) + "\n";
    if (uc && uc->ncon > 0) src += "#define ISLS_USER_COST_NCON " + std::to_string(uc->ncon) + "\n";
    return src + "#include \"" + device_hpp + "\"\n";
}

// The name expressions of a program as it is put together: kernel `k` of dims (n, m) in T, its further template arguments in
// `more`, goes behind the names so far and its slot to the role or to the rollout variant.  Nobody else knows a position.
struct Names {
    Program &pg;
    std::string head;                                        // "<T, n, m"
    Names(Program &pg_, int dtype, int n, int m)
        : pg(pg_), head(std::string(dtype == ISLS_DTYPE_F64 ? "<double, " : "<float, ") + std::to_string(n) + ", " + std::to_string(m)) {}
    int add(const char *k, const std::string &more = std::string())
    {
        pg.names.push_back(std::string("isls::") + k + head + more + ">");
        return (int)pg.names.size() - 1;
    }
    void role(Role r, const char *k, const std::string &more = std::string()) { pg.slot[r] = add(k, more); }
};

// a failed compile of a cost that calls isls::field and was registered without one: the sentence that says so, behind the compiler's
void no_field_sentence(Source &uc)
{
    if (uc.nfield == 0 && uc.source.find("isls::field") != std::string::npos)
        uc.log += "the source calls isls::field, but the cost was registered without a field: isls::field exists only in the programs "
                  "of a cost created with one (isls_user_cost_create_field; costs.Custom(field=...)).\n";
}

// The program of (model, cost, dtype), compiled on first use: a user model alone holds its own kernels, every key with a cost the
// cost's, every key with a model the rollout variants of its dimensions and the sampling round.  The compiler's messages go to
// the cost's log, to the model's when there is no cost.  ISLS_ERR_ARG: no such source, or a model and a cost of different
// dimensions; ISLS_ERR_UNSUPPORTED: a built-in model with no family for the cost's dimensions.
int program(int model, int cost, int dtype, Program **out)
{
    Source *um = is_user_model(model) ? find(KIND_MODEL, model) : nullptr, *uc = cost != kNone ? find(KIND_COST, cost) : nullptr;
    if ((is_user_model(model) && !um) || (cost != kNone && !uc) || (!um && !uc)) return ISLS_ERR_ARG;
    if (um && uc && (um->n != uc->n || um->m != uc->m)) return ISLS_ERR_ARG;
    const int n = uc ? uc->n : um->n, m = uc ? uc->m : um->m;
    const int mdlw = !um && model != kNone ? family_lds_words(n, m, model) : 0;
    if (mdlw < 0) return ISLS_ERR_UNSUPPORTED;
    Program &pg = g_prog[std::make_tuple(cost, dtype, model)];
    *out = &pg;
    if (pg.tried) return pg.ok ? ISLS_OK : ISLS_ERR_COMPILE;
    pg.mdlw = mdlw;
    pg.ntab = uc ? uc->ntab : 0;
    pg.mtab = um ? um->ntab : 0;
    pg.field_cost = uc && uc->nfield > 0 ? cost : kNone;
    pg.dtype = dtype;
    Names nm(pg, dtype, n, m);
    const std::string tmodel = ", " + std::to_string(um ? ISLS_MODEL_USER : model);   // the MODEL template argument
    if (uc) {
        nm.role(ROLE_EXP, "user_expand_kernel");
        nm.role(ROLE_VAL, "user_cost_value_kernel");
    } else {
        nm.role(ROLE_LIN, "user_linearize_kernel");
        nm.role(ROLE_LOOP, "dense_closed_loop_kernel", tmodel);
        nm.role(ROLE_STEP, "user_step_kernel");
        nm.role(ROLE_MC, "mc_closed_loop_kernel", tmodel);
        nm.role(ROLE_MPC, "mpc_step_kernel", tmodel);
    }
    if (model != kNone) {
        std::vector<std::pair<int, int>> ro;
#define ISLS_URTC_VARIANTS_(NX_, NU_) if (n == NX_ && m == NU_) ro_variants<NX_, NU_>(ro);
        ISLS_FOR_EACH_DIMS(ISLS_URTC_VARIANTS_)
#undef ISLS_URTC_VARIANTS_
        for (const auto &jo : ro)
            pg.ro.push_back({jo.first, jo.second, nm.add("rollout_kernel", tmodel + ", " + std::to_string(jo.first) + ", " + std::to_string(jo.second))});
        nm.role(ROLE_SMP_COST, "sample_cost_kernel", tmodel);
        nm.role(ROLE_SMP_UPDATE, "sample_update_kernel", tmodel);
        nm.role(ROLE_SMP_COST_FB, "sample_cost_fb_kernel", tmodel);
        nm.role(ROLE_SMP_UPDATE_FB, "sample_update_fb_kernel", tmodel);
    }
    if (um && !uc && um->ntab > 0) nm.role(ROLE_STEP_TAB, "user_step_tab_kernel");           // a row of the table per state row
    if (uc && uc->ncon > 0) nm.role(ROLE_CON_UPDATE, "user_constraint_update_kernel");
    const int rc = compile_program(program_text(um, uc, uc ? "user_cost.hpp" : "user_model.hpp", dtype), uc ? "user_cost.hip" : "user_model.hip",
                                   pg, (uc ? uc : um)->log);
    if (rc != ISLS_OK && uc) no_field_sentence(*uc);
    return rc;
}

bool dtype_ok(int dtype) { return dtype == ISLS_DTYPE_F64 || dtype == ISLS_DTYPE_F32; }

// The gradient program of a source (user_grad.hpp): the text of its own program with user_grad.hpp as the device side and one
// name expression, compiled on first request and kept apart from g_prog -- no key there, no code object there changes.  The
// compiler's messages go to the source's log; a failure adds the sentence that names the contract.
std::map<std::tuple<int, int, int>, Program> g_grad;         // (kind, id, dtype) -> program

int grad_program(Kind kind, int id, int dtype, Program **out)
{
    Source *src = find(kind, id);
    if (!src) return ISLS_ERR_ARG;
    Program &pg = g_grad[std::make_tuple((int)kind, id, dtype)];
    *out = &pg;
    if (pg.tried) return pg.ok ? ISLS_OK : ISLS_ERR_COMPILE;
    const bool cost = kind == KIND_COST;
    Names nm(pg, dtype, src->n, src->m);
    nm.role(ROLE_GRAD, cost ? "user_cost_grad_kernel" : "user_model_grad_kernel");
    pg.field_cost = cost && src->nfield > 0 ? id : kNone;
    pg.dtype = dtype;
    const std::string text = program_text(cost ? nullptr : src, cost ? src : nullptr, "user_grad.hpp", dtype);
    const int rc = compile_program(text, cost ? "user_cost_grad.hip" : "user_model_grad.hip", pg, src->log);
    if (rc != ISLS_OK && cost) no_field_sentence(*src);
    if (rc != ISLS_OK)
        src->log += std::string("the gradient program instantiates the source with P = S = a dual number: what it does with `par` and "
                                "`row` must keep to the S contract of user_model_ad.hpp (arithmetic, comparisons and the listed "
                                "functions; no integer cast, no plain-number copy of them).  The ") +
                    (cost ? "cost" : "model") + "'s other programs are not affected.\n";
    return rc;
}

}  // namespace

// ---- what user_model.hip and user_cost.hip build their entry points and launches from ------------------------------------------
int create(Kind kind, const char *source, int n, int m, int n_par, int n_tab, int32_t *id, int n_con, int n_field, int nx, int ny)
{
    if (!source || !id) return ISLS_ERR_ARG;
    if (!dims_supported(n, m) || n_par < 0 || n_par > ISLS_USER_MAX_PAR) return ISLS_ERR_UNSUPPORTED;
    if (n_tab < 0 || n_tab > ISLS_USER_MAX_TAB) return ISLS_ERR_UNSUPPORTED;
    // constraints: a cost's, and the row then holds a multiplier each and mu behind the user's words
    if (n_con < 0 || (n_con > 0 && (kind != KIND_COST || n_tab < n_con + 1))) return ISLS_ERR_UNSUPPORTED;
    if (n_field != 0 && (kind != KIND_COST || n_field < 1 || n_field > ISLS_USER_MAX_FIELD || nx < 4 || ny < 4 ||
                         (int64_t)n_field * nx * ny > ISLS_USER_MAX_FIELD_WORDS))
        return ISLS_ERR_UNSUPPORTED;
    auto src = std::make_unique<Source>();
    src->nfield = n_field; src->fnx = n_field ? nx : 0; src->fny = n_field ? ny : 0;
    src->source = source; src->n = n; src->m = m; src->npar = n_par; src->ntab = n_tab; src->ncon = n_con;
    if (refused_source(src->source)) return ISLS_ERR_ARG;     // plain arithmetic: no hand-written ISA through this door
    std::lock_guard<std::mutex> lk(g_mu);
    *id = (kind == KIND_MODEL ? ISLS_MODEL_USER_BASE : ISLS_COST_USER_BASE) + (int32_t)g_src[kind].size();
    g_src[kind].push_back(std::move(src));
    Program *pg;                                             // fp64 at once: every operation of the source meets the compiler
    return kind == KIND_MODEL ? program(*id, kNone, ISLS_DTYPE_F64, &pg) : program(kNone, *id, ISLS_DTYPE_F64, &pg);
}

int64_t copy_log(Kind kind, int id, char *buf, int64_t len)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = find(kind, id);
    if (!src) return ISLS_ERR_ARG;
    if (buf && len > 0) {
        const size_t k = src->log.size() < (size_t)(len - 1) ? src->log.size() : (size_t)(len - 1);
        memcpy(buf, src->log.data(), k);
        buf[k] = '\0';
    }
    return (int64_t)src->log.size();
}

int copy_code(int model, int cost, int dtype, void *buf, int64_t *len)
{
    if (!len || !dtype_ok(dtype)) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    Program *pg;
    const int rc = program(model, cost, dtype, &pg);
    if (rc != ISLS_OK) return rc;
    const int64_t cap = *len;
    *len = (int64_t)pg->code.size();
    if (buf) {
        if (cap < *len) return ISLS_ERR_ARG;
        memcpy(buf, pg->code.data(), pg->code.size());
    }
    return ISLS_OK;
}

int load(int model, int cost, int dtype)
{
    if (!dtype_ok(dtype)) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    Program *pg;
    const int rc = program(model, cost, dtype, &pg);
    return rc != ISLS_OK ? rc : load_program(*pg, nullptr, nullptr);
}

int dims(Kind kind, int id, int *n, int *m)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = find(kind, id);
    if (!src) return ISLS_ERR_ARG;
    *n = src->n; *m = src->m;
    return ISLS_OK;
}

int n_tab(int cost)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = find(KIND_COST, cost);
    return src ? src->ntab : ISLS_ERR_ARG;
}

int n_con(int cost)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = find(KIND_COST, cost);
    return src ? src->ncon : ISLS_ERR_ARG;
}

int model_n_tab(int model)
{
    if (!is_user_model(model)) return 0;
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = find(KIND_MODEL, model);
    return src ? src->ntab : ISLS_ERR_ARG;
}

int check_model_table(int model, int N, const void *par, int64_t par_sb, int rows_min)
{
    if (!is_user_model(model)) return ISLS_OK;
    int P, W;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const Source *src = find(KIND_MODEL, model);
        if (!src) return ISLS_ERR_ARG;
        P = src->npar; W = src->ntab;
    }
    if (W <= 0) return ISLS_OK;
    if (!par || N < 1) return ISLS_ERR_ARG;
    if (rows_min >= 0 && rows_min < N) return par_sb == 0 || par_sb >= (int64_t)P + (int64_t)rows_min * W ? ISLS_OK : ISLS_ERR_ARG;
    return par_sb == 0 || par_sb == (int64_t)P + (int64_t)N * W ? ISLS_OK : ISLS_ERR_ARG;
}

int check_table(int cost, int N, const void *tab, int64_t tab_sb, int nvia)
{
    const int W = n_tab(cost);
    if (W <= 0) return W < 0 ? ISLS_ERR_ARG : ISLS_OK;
    const bool ok = tab != nullptr && (tab_sb == 0 || tab_sb == (int64_t)N * W) && (nvia < 0 || nvia == W);
    return ok ? ISLS_OK : ISLS_ERR_ARG;
}

int prepare(int model, int cost, int dtype, int n, int m, hipStream_t s, Kernels *k)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = cost != kNone ? find(KIND_COST, cost) : find(KIND_MODEL, model);
    if (!src || src->n != n || src->m != m) return ISLS_ERR_ARG;
    if (cost != kNone && check_field(src) != ISLS_OK) return ISLS_ERR_ARG;   // a field cost whose field was never set here
    if (model == kNone) {
        // the cost's own kernels: every program of the cost holds them.  One that is on this device already serves (the pair the
        // engine loaded); the cost's own program is compiled only when there is no such pair
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return ISLS_ERR_LAUNCH;
        for (auto it = g_prog.lower_bound(std::make_tuple(cost, dtype, kNone)); it != g_prog.end(); ++it) {
            if (std::get<0>(it->first) != cost || std::get<1>(it->first) != dtype) break;
            if (it->second.ok && it->second.dev.count(dev)) { model = std::get<2>(it->first); break; }
        }
    }
    Program *pg;
    const int rc = program(model, cost, dtype, &pg);
    if (rc != ISLS_OK) return rc;
    k->pg = pg;
    return load_program(*pg, &k->fns, s);
}

int grad_build(Kind kind, int id, int dtype)
{
    if (!dtype_ok(dtype)) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    Program *pg;
    return grad_program(kind, id, dtype, &pg);
}

int grad_prepare(Kind kind, int id, int dtype, int n, int m, hipStream_t s, hipFunction_t *fn, int *n_par, int *n_row, int *n_tab)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = find(kind, id);
    if (!src || src->n != n || src->m != m) return ISLS_ERR_ARG;
    *n_par = src->npar; *n_tab = src->ntab;
    *n_row = src->ncon > 0 ? src->ntab - src->ncon - 1 : src->ntab;
    if (!fn) return ISLS_OK;
    if (kind == KIND_COST && check_field(src) != ISLS_OK) return ISLS_ERR_ARG;
    Program *pg;
    int rc = grad_program(kind, id, dtype, &pg);
    if (rc != ISLS_OK) return rc;
    Kernels k = {pg, nullptr};
    if ((rc = load_program(*pg, &k.fns, s)) != ISLS_OK) return rc;
    *fn = k.of(ROLE_GRAD);
    return ISLS_OK;
}

int field_dims(int cost, int *C, int *nx, int *ny)
{
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = find(KIND_COST, cost);
    if (!src || !C || !nx || !ny) return ISLS_ERR_ARG;
    *C = src->nfield; *nx = src->fnx; *ny = src->fny;
    return ISLS_OK;
}

int field_ptr(int cost, int dtype, void **ptr)
{
    if (!dtype_ok(dtype) || !ptr) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    const Source *src = find(KIND_COST, cost);
    if (!src || src->nfield == 0) return ISLS_ERR_ARG;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ISLS_ERR_LAUNCH;
    const auto it = src->fdev.find(dev);
    *ptr = it == src->fdev.end() || !it->second.set ? nullptr : (dtype == ISLS_DTYPE_F64 ? it->second.v64 : it->second.v32);
    return ISLS_OK;
}

int set_field(int cost, const void *values, int dtype, const double *origin, const double *spacing, hipStream_t s)
{
    if (!dtype_ok(dtype) || !values || !origin || !spacing) return ISLS_ERR_ARG;
    for (int a = 0; a < 2; ++a)                              // (a NaN fails every comparison)
        if (!(spacing[a] > 0.0) || !(spacing[a] <= 1.79e308) || !(origin[a] >= -1.79e308 && origin[a] <= 1.79e308)) return ISLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_mu);
    Source *src = find(KIND_COST, cost);
    if (!src || src->nfield == 0) return ISLS_ERR_ARG;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ISLS_ERR_LAUNCH;
    const int n = src->nfield * src->fnx * src->fny;          // <= 2^24
    Source::FieldDev &fd = src->fdev[dev];
    const double inv[2] = {1.0 / spacing[0], 1.0 / spacing[1]};
    const bool same_grid = fd.set && fd.org[0] == origin[0] && fd.org[1] == origin[1] && fd.inv[0] == inv[0] && fd.inv[1] == inv[1];
    if (!same_grid) {
        // the first field on this device, or another grid: buffers are allocated and descriptors written below, neither of which
        // a stream capture can hold -- refused before anything is enqueued, so samples and descriptors never part ways
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return ISLS_ERR_LAUNCH;
    }
    if (!fd.v64) {
        if (hipMalloc(&fd.v64, (size_t)n * sizeof(double)) != hipSuccess) { fd.v64 = nullptr; return ISLS_ERR_LAUNCH; }
        if (hipMalloc(&fd.v32, (size_t)n * sizeof(float)) != hipSuccess) {
            (void)hipFree(fd.v64);
            fd.v64 = fd.v32 = nullptr;
            return ISLS_ERR_LAUNCH;
        }
    }
    // the samples: the copy of the caller's precision as it is, the other by the conversion kernel, both in place on `s`
    const int grid = (n + 255) / 256;
    if (dtype == ISLS_DTYPE_F64) {
        if (hipMemcpyAsync(fd.v64, values, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s) != hipSuccess) return ISLS_ERR_LAUNCH;
        hipLaunchKernelGGL((field_convert_kernel<double, float>), dim3(grid), dim3(256), 0, s, (const double *)fd.v64, (float *)fd.v32, n);
    } else {
        if (hipMemcpyAsync(fd.v32, values, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return ISLS_ERR_LAUNCH;
        hipLaunchKernelGGL((field_convert_kernel<float, double>), dim3(grid), dim3(256), 0, s, (const float *)fd.v32, (double *)fd.v64, n);
    }
    if (hipGetLastError() != hipSuccess) return ISLS_ERR_LAUNCH;
    if (same_grid) return ISLS_OK;
    // the first field on this device, or another grid: into the descriptor of every module of the cost that is here already.  What
    // is in flight on `s` still reads the old one, so it ends first (not inside a capture of `s`).
    if (fd.set && hipStreamSynchronize(s) != hipSuccess) return ISLS_ERR_LAUNCH;
    fd.org[0] = origin[0]; fd.org[1] = origin[1]; fd.inv[0] = inv[0]; fd.inv[1] = inv[1];
    fd.set = true;
    auto write = [&](Program &pg) {
        const auto it = pg.dev.find(dev);
        return pg.field_cost != cost || it == pg.dev.end() ? (int)ISLS_OK : write_field(pg, dev, it->second.first);
    };
    int rc = ISLS_OK;
    for (auto &kv : g_prog)
        if (rc == ISLS_OK) rc = write(kv.second);
    for (auto &kv : g_grad)
        if (rc == ISLS_OK) rc = write(kv.second);
    // a descriptor that could not be written leaves the modules on two grids: the field counts as not set here (every launch is
    // ISLS_ERR_ARG) until a set_field goes through, which writes all of them again
    if (rc != ISLS_OK) fd.set = false;
    return rc;
}

int release_field(int cost)
{
    std::lock_guard<std::mutex> lk(g_mu);
    Source *src = find(KIND_COST, cost);
    if (!src || src->nfield == 0) return ISLS_ERR_ARG;
    int cur = 0;
    if (src->fdev.empty()) return ISLS_OK;
    if (hipGetDevice(&cur) != hipSuccess) return ISLS_ERR_LAUNCH;
    int rc = ISLS_OK;
    for (auto &kv : src->fdev) {                             // hipFree waits for what still reads the buffers
        if (!kv.second.v64) continue;
        if (hipSetDevice(kv.first) != hipSuccess || hipFree(kv.second.v64) != hipSuccess || hipFree(kv.second.v32) != hipSuccess)
            rc = ISLS_ERR_LAUNCH;
    }
    (void)hipSetDevice(cur);
    src->fdev.clear();                                       // not set anywhere: a launch is ISLS_ERR_ARG until the next set_field
    return rc;
}

int launch(hipFunction_t f, int grid, size_t smem, hipStream_t s, void **args, int lanes)
{
    if (!f) return ISLS_ERR_UNSUPPORTED;
    if (grid <= 0) return ISLS_OK;
    return hipModuleLaunchKernel(f, grid, 1, 1, lanes, 1, 1, (unsigned)smem, s, args, nullptr) == hipSuccess ? ISLS_OK : ISLS_ERR_LAUNCH;
}

}  // namespace urtc

// ---- the line search of every key (dispatched from rollout.hip on a user model or a user cost) ---------------------------------
template <typename T>
int launch_rollout_user(RoP<T> &p, const isls_rollout_args &a, hipStream_t s, bool want_fused)
{
    const bool ucost = is_user_cost(a.cost_model);
    if (ucost && (!a.cost_par || a.cost_par_sb < 0)) return ISLS_ERR_ARG;
    urtc::Kernels k;
    int rc = ucost ? urtc::check_table(a.cost_model, a.N, a.ztab, a.ztab_sb, a.nvia) : ISLS_OK;   // the table: ztab, ztab_sb, nvia
    if (rc != ISLS_OK) return rc;
    if ((rc = urtc::check_model_table(a.model, a.N, a.model_par, a.model_par_sb)) != ISLS_OK) return rc;   // a model's: behind model_par
    rc = urtc::prepare(a.model, ucost ? a.cost_model : urtc::kNone, urtc::dtype_of<T>(), a.n, a.m, s, &k);
    if (rc != ISLS_OK) return rc;
    const urtc::Program *pg = k.pg;
    if (ucost) p.cpar_sb = a.cost_par_sb;
    RoLaunch pl;
    rc = ISLS_ERR_UNSUPPORTED;
    // the model enters the plan through its LDS words only (a dense LTI model's [A B]; none for the others and for user models),
    // a cost's table and a user model's through the side records of their rows behind them
#define ISLS_URTC_PLAN_(NX_, NU_)                                                                              \
    if (a.n == NX_ && a.m == NU_)                                                                              \
        rc = pg->mdlw ? plan_rollout<T, NX_, NU_, NX_ * (NX_ + NU_)>(p, a, want_fused, nullptr, pl, pg->ntab)  \
                      : plan_rollout<T, NX_, NU_, 0>(p, a, want_fused, nullptr, pl, pg->ntab, pg->mtab);
    ISLS_FOR_EACH_DIMS(ISLS_URTC_PLAN_)
#undef ISLS_URTC_PLAN_
    if (rc != ISLS_OK) return rc;
    void *args[] = {&p};
    return urtc::launch(k.rollout(pl.jm, pl.occ), pl.grid, pl.smem, s, args);
}
template int launch_rollout_user<double>(RoP<double> &, const isls_rollout_args &, hipStream_t, bool);
template int launch_rollout_user<float>(RoP<float> &, const isls_rollout_args &, hipStream_t, bool);

}  // namespace isls
