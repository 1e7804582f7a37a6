// lib_common.h -- the host-side error plumbing every single-file library (gab, gls, gmr, gop, grl, gdc, gev, gfs) has behind its C ABI: the text
// <lib>_last_error() returns, fail() that writes it, and the check that follows a launch.  Each library is its own shared object and
// includes this once, so the `static` buffer below is that library's own (and each calling thread's own).  libgsr keeps its own in
// gsr_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// after a launch: return `code` with "<what>: <HIP's text>" when the launch was refused
#define LAUNCH_CHECK(code, what)                                                                      \
    do {                                                                                              \
        hipError_t e_ = hipGetLastError();                                                            \
        if (e_ != hipSuccess) return fail(code, "%s: %s", what, hipGetErrorString(e_));               \
    } while (0)
