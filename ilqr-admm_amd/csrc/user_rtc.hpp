// user_rtc.hpp -- what the run-time compiled pieces share (user_model.hip implements it; user_cost.hip uses it too): one hiprtc
// program per dtype with its name expressions, its code object and its module per device, and the module launcher.
#pragma once

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rollout_kernel.hpp"

namespace isls {
namespace urtc {

struct Program {                                             // one dtype of a model, or of a (cost, model) pair
    bool tried = false, ok = false;
    std::vector<char> code;
    std::vector<std::string> names, lowered;                 // name expressions and their mangled names
    std::vector<std::pair<int, int>> ro;                     // (JM, OCC) of the rollout variants among the names
    std::map<int, std::pair<hipModule_t, std::vector<hipFunction_t>>> dev;   // device -> module, functions
};

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
inline void ro_variants_of(int n, int m, std::vector<std::pair<int, int>> &v)
{
    v.clear();
#define ISLS_URTC_VARIANTS_(NX_, NU_) if (n == NX_ && m == NU_) ro_variants<NX_, NU_>(v);
    ISLS_FOR_EACH_DIMS(ISLS_URTC_VARIANTS_)
#undef ISLS_URTC_VARIANTS_
}

// a user source is plain arithmetic: true when it holds `asm` (any spelling) or `__builtin_amdgcn`
bool refused_source(const std::string &src);
// `body` inside `namespace ns`, every function of it always_inline (a call that is not inlined would take its arrays through
// scratch memory), compiler messages pointing at `label`:<line of the user's text>
std::string wrap_source(const std::string &ns, const std::string &label, const std::string &body);
// Compile `src` (file name `file` in the messages) for gfx950 with pg.names as name expressions, with the flags of the library's
// own kernels; fills pg.code / pg.lowered, appends the compiler's log to `log`.  Once per Program (pg.tried).
int compile_program(const std::string &src, const char *file, Program &pg, std::string &log);
// the program's functions (index: pg.names) on the current device, loaded on first use -- never inside a stream capture
// (capture_check: the stream to test, or nullptr)
int load_program(Program &pg, const std::vector<hipFunction_t> **out, hipStream_t capture_check);
int launch(hipFunction_t f, int grid, size_t smem, hipStream_t s, void **args);
// a registered user model (ISLS_ERR_ARG: no such id)
int user_model_info(int id, std::string *source, int *n, int *m, int *npar);

template <typename T>
constexpr int dtype_of() { return sizeof(T) == 8 ? ISLS_DTYPE_F64 : ISLS_DTYPE_F32; }

}  // namespace urtc
}  // namespace isls
