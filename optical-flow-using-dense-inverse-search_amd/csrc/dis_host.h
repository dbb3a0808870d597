// dis_host.h -- what the translation units of the C-ABI that call HIP share:
// error reporting into the calling thread's dis_last_error slot, and the
// device selection of the entry points that take a device index.
#pragma once

#include <string>

#include <hip/hip_runtime.h>

#include "dis_abi.h"

namespace dis {

dis_status set_error(dis_status s, const std::string& msg);  // (dis_runtime.hip owns the slot)
dis_status use_device(int device);  // one of the HIP devices present, and now the calling thread's

}  // namespace dis

static inline dis_status fail(dis_status s, const std::string& msg) { return dis::set_error(s, msg); }

#define DIS_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(DIS_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

// a rule of dis_args.h: nullptr, or why the call is refused
#define DIS_ARG(rule) \
    do { if (const char* why_ = (rule)) return fail(DIS_ERR_INVALID_ARGUMENT, why_); } while (0)
