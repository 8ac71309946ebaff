// entry.hpp -- how a .hip file writes the extern "C" entry points of libisls_hip.so (declared in include/isls_hip.h).
#pragma once

#define ISLS_API extern "C" __attribute__((visibility("default")))

// Both precisions of an entry point: the body sees T.
#define ISLS_TYPED_PAIR(name, PARAMS, ...)                                   \
    ISLS_API int isls_##name##_f64 PARAMS { using T = double; __VA_ARGS__ }  \
    ISLS_API int isls_##name##_f32 PARAMS { using T = float; __VA_ARGS__ }
// The pairs over one argument block.  EMPTY: the expression over `a` that means "empty batch: nothing to check, nothing to
// do" (false: the launcher sees every call).
#define ISLS_ENTRY(name, args_t, launcher, EMPTY)                            \
    ISLS_TYPED_PAIR(name, (const args_t *a, void *stream),                   \
                    if (!a) return ISLS_ERR_ARG;                             \
                    if (EMPTY) return ISLS_OK;                               \
                    return launcher<T>(*a, (hipStream_t)stream);)
