// host.h -- what the host files of the C-ABI library (mi_X.hip, one for each public header include/mi_X.h) share: the calling thread's last error
// (mi_rast_last_error), HIP_TRY, the 256-byte carving of workspaces and state buffers, and the overlap check of a call's byte ranges.
#pragma once

#include "../../include/mi_rast.h"

#include <hip/hip_runtime.h>

#include <string>

namespace mirast {

// ONE object for the whole library (inline, in a named namespace): what fail() stores in any host file is what mi_rast_last_error()
// (mi_rast.hip) returns.  In an anonymous namespace every file would have its own, and the add-on calls' messages would be lost.
inline thread_local std::string g_last_error;

inline int fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(MI_RAST_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
    } while (0)

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t v) { return (v + ALIGN - 1) & ~(ALIGN - 1); }

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        size_t o = off;
        off = align_up(off + bytes);
        return o;
    }
};

// a byte range of a call's arguments, for the check that no output meets another tensor
struct Range {
    const char* lo;
    size_t bytes;
    bool out;
};

inline bool overlap(const Range& a, const Range& b)
{
    return a.bytes && b.bytes && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes;
}

// true when an output range meets any other range
inline bool outputs_overlap(const Range* r, int n)
{
    for (int a = 0; a < n; a++)
        for (int b = a + 1; b < n; b++)
            if ((r[a].out || r[b].out) && overlap(r[a], r[b])) return true;
    return false;
}

}  // namespace mirast
