// dis_motion.h -- what the global-motion kernels of dis_motion.hip (the affine
// family) and dis_homography.hip (the eight-parameter family) share: the
// loaders of a field's vectors, a lane's walk over its pixels of a chunk, the
// LDL^T solve, and the stores of a synthesised field. Device code only; every
// operation is separately rounded (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dis_args.h"
#include "dis_half.h"

namespace dis {
namespace {

constexpr int kMotionThreads = 256;  // the slots of a chunk
constexpr int kMotionSteps = kMotionChunk / kMotionThreads;  // pixels of a slot: 64
constexpr int kMotionBurst = 8;      // loads a lane issues before it uses the first
constexpr int kSolveThreads = 64;
constexpr int kMotionFlowThreads = 256;
constexpr unsigned kNanBits = 0x7fc00000u;

__device__ __forceinline__ bool vec_ok(float2 q) { return fabsf(q.x) < 1e9f && fabsf(q.y) < 1e9f; }  // false for NaN

struct LoadF32 {
    static constexpr int kBytes = 8;
    static __device__ __forceinline__ float2 at(const void* p, long long i) { return static_cast<const float2*>(p)[i]; }
};
struct LoadF16 {
    static constexpr int kBytes = 4;
    static __device__ __forceinline__ float2 at(const void* p, long long i)
    {
        return widen2(static_cast<const __half2*>(p)[i]);
    }
};

// A lane's walk over its pixels of a chunk: pixel q = y * W + x, then 256 further.
struct Walk {
    long long q;
    int x, y, dx, dy, W;
    __device__ __forceinline__ Walk(long long q0, int W_) : q(q0), W(W_)
    {
        y = (int)(q0 / W_);
        x = (int)(q0 - (long long)y * W_);
        dx = kMotionThreads % W_;
        dy = kMotionThreads / W_;
    }
    __device__ __forceinline__ void next()
    {
        q += kMotionThreads;
        x += dx;
        y += dy;
        if (x >= W) x -= W, ++y;
    }
};

// A x = b for R right-hand sides by LDL^T without pivoting, in place; false when
// a pivot is not above 2^-20 of its diagonal element.
template <int M, int R>
__device__ __forceinline__ bool ldl_solve(const double (&A)[M][M], double (&b)[R][M])
{
    double L[M][M], d[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * d[k];
        if (!(dj > 0x1p-20 * A[j][j])) return false;
        d[j] = dj;
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = t / dj;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double* const z = b[r];
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
            for (int k = 0; k < i; ++k) z[i] = z[i] - L[i][k] * z[k];
        }
#pragma unroll
        for (int i = 0; i < M; ++i) z[i] = z[i] / d[i];
#pragma unroll
        for (int i = M - 1; i >= 0; --i) {
#pragma unroll
            for (int k = i + 1; k < M; ++k) z[i] = z[i] - L[k][i] * z[k];
        }
    }
    return true;
}

// What a field kernel stores: `word` is one vector; quad: a lane's four at once
// (p0 even and the pointer aligned to 16 bytes for f32, 8 for f16).
struct StoreF32 {
    using word = float2;
    static __device__ __forceinline__ word pack(float2 v) { return v; }
    static __device__ __forceinline__ word nan()
    {
        const float q = __uint_as_float(kNanBits);
        return make_float2(q, q);
    }
    static __device__ __forceinline__ void one(void* out, long long p, word o) { static_cast<float2*>(out)[p] = o; }
    static __device__ __forceinline__ void quad(void* out, long long p0, const word* o)
    {
        float4* const d = reinterpret_cast<float4*>(static_cast<float2*>(out) + p0);
        d[0] = make_float4(o[0].x, o[0].y, o[1].x, o[1].y);
        d[1] = make_float4(o[2].x, o[2].y, o[3].x, o[3].y);
    }
};
struct StoreF16 {
    using word = unsigned;  // the bits of one __half2
    static __device__ __forceinline__ word pack(float2 v)
    {
        const __half2 h = narrow2(v);
        word w;
        __builtin_memcpy(&w, &h, 4);
        return w;
    }
    static __device__ __forceinline__ word nan() { return 0x7e007e00u; }
    static __device__ __forceinline__ void one(void* out, long long p, word o) { static_cast<unsigned*>(out)[p] = o; }
    static __device__ __forceinline__ void quad(void* out, long long p0, const word* o)
    {
        uint2* const d = reinterpret_cast<uint2*>(static_cast<unsigned*>(out) + p0);
        d[0] = make_uint2(o[0], o[1]);
        d[1] = make_uint2(o[2], o[3]);
    }
};

}  // namespace
}  // namespace dis
