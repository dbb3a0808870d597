// dis_convert.hip -- dis_flow_convert's kernel (include/dis_abi.h): `count`
// flow values between DIS_FLOW_F32 and DIS_FLOW_F16. No reference counterpart
// (the reference knows float flows only).
//
// f32 -> f16 is narrow2 (dis_half.h), the conversion every flow writer of the
// engine uses; f16 -> f32 is exact. A thread converts four values: one 16-byte
// access on the f32 side, one 8-byte access on the f16 side. The launcher peels
// `head` values so that the wide side of the body is aligned; when the other
// side then is too (two buffers offset by the same number of values from
// aligned bases are), the body runs vectorised. The head, the tail and an
// unalignable body go value by value.
#include <cstdint>
#include <type_traits>

#include "dis_half.h"
#include "dis_kernels.h"

namespace dis {
namespace {

struct ConvertArgs {
    const void* src;
    void* dst;
    long long count;
    long long head;  // values in front of the vector body
    long long nvec;  // 4-value groups of the body (0: everything value by value)
};

__device__ __forceinline__ __half narrow1(float v) { return __low2half(narrow2(make_float2(v, 0.0f))); }

// grid: ceil((nvec + count - 4 nvec) / 256) blocks of 256 threads: threads
// [0, nvec) take a group each, the rest one leftover value each
template <bool NARROW>
__global__ void __launch_bounds__(256) k_flow_convert(ConvertArgs a)
{
    using S = std::conditional_t<NARROW, float, __half>;
    using D = std::conditional_t<NARROW, __half, float>;
    const S* const src = static_cast<const S*>(a.src);
    D* const dst = static_cast<D*>(a.dst);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < a.nvec) {
        const long long k = a.head + 4 * i;
        if constexpr (NARROW) {
            const float4 v = *reinterpret_cast<const float4*>(src + k);
            *reinterpret_cast<half2x2*>(dst + k) =
                half2x2{narrow2(make_float2(v.x, v.y)), narrow2(make_float2(v.z, v.w))};
        } else {
            const half2x2 h = *reinterpret_cast<const half2x2*>(src + k);
            const float2 lo = widen2(h.a), hi = widen2(h.b);
            *reinterpret_cast<float4*>(dst + k) = make_float4(lo.x, lo.y, hi.x, hi.y);
        }
        return;
    }
    // leftovers: the head, then what follows the body
    long long k = i - a.nvec;
    if (k >= a.head) k += 4 * a.nvec;
    if (k >= a.count) return;
    if constexpr (NARROW)
        dst[k] = narrow1(src[k]);
    else
        dst[k] = __half2float(src[k]);
}

}  // namespace

hipError_t launch_flow_convert(const void* src, int src_format, void* dst, size_t count, hipStream_t s)
{
    if (!count) return hipSuccess;
    const bool narrow = src_format == DIS_FLOW_F32;
    // the f32 side is the wide one: `head` values bring it to 16 bytes
    const uintptr_t wide = reinterpret_cast<uintptr_t>(narrow ? src : dst);
    const uintptr_t thin = reinterpret_cast<uintptr_t>(narrow ? dst : src);
    ConvertArgs a{};
    a.src = src;
    a.dst = dst;
    a.count = (long long)count;
    if ((wide & 3) == 0) {
        const long long head = (long long)(((16 - (wide & 15)) & 15) / 4);
        if (head <= a.count && ((thin + 2 * (uintptr_t)head) & 7) == 0) {
            a.head = head;
            a.nvec = (a.count - head) / 4;
        }
    }
    const long long threads = a.nvec + (a.count - 4 * a.nvec);
    const long long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (narrow)
        hipLaunchKernelGGL(k_flow_convert<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_flow_convert<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dis
