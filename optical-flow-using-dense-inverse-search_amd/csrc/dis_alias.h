// dis_alias.h -- which buffers of a warm-started call (dis_calc_batch_init_u8)
// may share memory. Host-only and pure: tests/cpp/init_alias_host.cpp runs it
// under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace dis {

// [a, a + na) and [b, b + nb) share a byte (empty ranges share none; the sums
// are formed so that a range ending at the top of the address space does not
// wrap)
inline bool ranges_overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb)
{
    if (na == 0 || nb == 0) return false;
    return a <= b ? b - a < na : a - b < nb;
}

// The rules: `init` may start exactly where `flow` starts (flow in, flow out:
// the init plane is complete before any output is written), otherwise the two
// must be disjoint; `init` must not touch either frame batch.
// Returns nullptr if the call may go ahead, else what is wrong.
inline const char* check_init_aliasing(uintptr_t init, size_t init_bytes, uintptr_t flow, size_t flow_bytes,
                                       uintptr_t i0, uintptr_t i1, size_t frame_bytes)
{
    if (init != flow && ranges_overlap(init, init_bytes, flow, flow_bytes))
        return "init partially overlaps flow (it may be the flow buffer itself, or disjoint from it)";
    if (ranges_overlap(init, init_bytes, i0, frame_bytes) || ranges_overlap(init, init_bytes, i1, frame_bytes))
        return "init overlaps the frames";
    return nullptr;
}

}  // namespace dis
