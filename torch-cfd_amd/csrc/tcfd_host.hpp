// tcfd_host.hpp -- host-side helpers shared by every translation unit of the library: the error state's setter, the
// failure macros of the C ABI's entry points, environment switches and the workspace alignment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/tcfd.h"

int tcfd_set_error(int code, const char* fmt, ...);  // defined in tcfd_ns2d.hip; returns `code`
#define FAIL(...) tcfd_set_error(__VA_ARGS__)
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return FAIL(TCFD_EHIP, "%s: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

// integer switch from the environment; unset or empty: `dflt`
static inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
