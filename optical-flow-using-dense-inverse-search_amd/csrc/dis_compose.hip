// dis_compose.hip -- flows chained over a video: composition of flow fields
// (dis_flow_compose) and advection of points (dis_flow_advect_points),
// include/dis_abi.h. No reference counterpart: the reference computes one pair.
//
// With a the field frame 0 -> k and b the field k -> k+1, the composed field at
// pixel (x, y) is a(x, y) + b sampled bilinearly at (x + a(x, y)): the sampler
// of dis_consistency.hip's fb_pixel (same taps, same weights, same order of
// sums) with a different tail. A pixel whose own vector, target or any of its
// four taps is not to be trusted gets the canonical quiet NaN and valid 0; no
// tap index is formed before the vector and the target have been tested, so it
// lies in the frame for every input. Every float operation is separately
// rounded (-ffp-contract=off), so tests/composeref.py restates it bit for bit.
//
// Bandwidth plus gathers: each lane owns 4 consecutive pixels of a row, with
// 16-byte loads of a (two for f32, one for f16), 8-byte / 4-byte taps of b, one
// dword of valid_a, 16-byte (f32) or 8-byte (f16) stores of out and one dword
// of valid_out, when pointers and W allow (chosen at run time, as k_fb_check's
// forms are); the scalar forms move the same bytes. No LDS, no atomics. out may
// be a itself and valid_out valid_a itself: a lane reads its own pixels of both
// before it writes them, and b and mask_b never overlap an output. The formats
// of a, b and out are template parameters (a loader or storer each).
#include <cmath>
#include <cstdint>

#include "dis_half.h"
#include "dis_kernels.h"
#include "dis_sample.h"

namespace dis {
namespace {

constexpr int kComposeThreads = 256;
constexpr int kAdvectThreads = 256;

// A field's vectors by index, widened to float2.
struct LoadF32 {
    static constexpr bool kF16 = false;
    static __device__ __forceinline__ float2 at(const void* p, long long i) { return static_cast<const float2*>(p)[i]; }
};
struct LoadF16 {
    static constexpr bool kF16 = true;
    static __device__ __forceinline__ float2 at(const void* p, long long i)
    {
        return widen2(static_cast<const __half2*>(p)[i]);
    }
};

// The output's vectors: `word` is one stored vector; quad: a lane's four at
// once (p0 even and the pointer aligned to 16 bytes for f32, 8 for f16).
struct StoreF32 {
    using word = float2;
    static __device__ __forceinline__ word pack(float2 v) { return v; }
    static __device__ __forceinline__ word nan()
    {
        const float q = __uint_as_float(0x7fc00000u);
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

__device__ __forceinline__ bool vec_ok(float2 q) { return fabsf(q.x) < 1e9f && fabsf(q.y) < 1e9f; }  // false for NaN

// Field B (vectors from index `base` on, W x H; M its mask bytes from `base` on,
// or null) sampled at (px, py), which the caller has tested to lie inside
// [0, W-1] x [0, H-1]: fb_pixel's taps and sums. False when a tap vector is
// invalid or a tap's mask byte is 0 (tested on the inputs, whatever the weights).
template <class LB>
__device__ __forceinline__ bool sample_field(const void* __restrict__ B, const uint8_t* __restrict__ M, long long base,
                                             int W, int H, float px, float py, float* su, float* sv)
{
    const float x0 = floorf(px), y0 = floorf(py);
    const float a = px - x0, b = py - y0;
    const int ix0 = (int)x0, iy0 = (int)y0;  // in [0, W-1] x [0, H-1]
    const int ix1 = min(ix0 + 1, W - 1), iy1 = min(iy0 + 1, H - 1);
    const float ia = 1.0f - a, ib = 1.0f - b;
    const float w00 = ia * ib, w01 = a * ib, w10 = ia * b, w11 = a * b;
    const long long r0 = base + (long long)iy0 * W, r1 = base + (long long)iy1 * W;
    const float2 b00 = LB::at(B, r0 + ix0), b01 = LB::at(B, r0 + ix1);
    const float2 b10 = LB::at(B, r1 + ix0), b11 = LB::at(B, r1 + ix1);
    bool ok = vec_ok(b00) && vec_ok(b01) && vec_ok(b10) && vec_ok(b11);
    if (M) ok = ok && M[r0 + ix0] && M[r0 + ix1] && M[r1 + ix0] && M[r1 + ix1];
    *su = ((w00 * b00.x + w01 * b01.x) + w10 * b10.x) + w11 * b11.x;
    *sv = ((w00 * b00.y + w01 * b01.y) + w10 * b10.y) + w11 * b11.y;
    return ok;
}

__device__ __forceinline__ bool inside(float px, float py, int W, int H)  // false for NaN
{
    return px >= 0.0f && px <= (float)(W - 1) && py >= 0.0f && py <= (float)(H - 1);
}

struct ComposeArgs {
    const void* a;           // float2 or __half2 vectors (may be `out`)
    const void* b;
    void* out;
    const uint8_t* valid_a;  // may be null (may be `valid_out`)
    const uint8_t* mask_b;   // may be null
    uint8_t* valid_out;      // may be null
    long long items;         // n * H * cw lanes of work
    int W, H, cw;            // cw = ceil(W / 4) lanes per row
    int vec_a;          // a 16-byte aligned and W even (f16: W % 4 == 0): 16-byte loads of a lane's vectors
    int vec_valid_a;    // valid_a 4-byte aligned and W % 4 == 0: one dword per lane
    int vec_out;        // out 16-byte (f16: 8-byte) aligned and W even: a lane's four vectors in two stores
    int vec_valid_out;  // valid_out 4-byte aligned and W % 4 == 0: one dword per lane
};

template <class LA, class LB, class ST>
__global__ void __launch_bounds__(kComposeThreads) k_flow_compose(ComposeArgs a)
{
    const long long t = (long long)blockIdx.x * kComposeThreads + threadIdx.x;
    if (t >= a.items) return;
    const long long row = t / a.cw;  // field * H + y
    const int x0 = (int)(t - row * a.cw) * 4;
    const long long f = row / a.H;
    const int y = (int)(row - f * a.H);
    const long long p0 = row * a.W + x0;  // first pixel of this lane
    const long long base = f * a.H * (long long)a.W;  // first pixel of this lane's field
    const int m = min(4, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    // everything this lane reads of a and valid_a, before any store (in place)
    float2 q[4];
    load_flow4<LA::kF16>(a.a, p0, m, a.vec_a, q);
    unsigned va[4] = {255u, 255u, 255u, 255u};
    if (a.valid_a) {
        if (a.vec_valid_a) {  // (W % 4 == 0: m == 4)
            const unsigned d = *reinterpret_cast<const unsigned*>(a.valid_a + p0);
#pragma unroll
            for (int i = 0; i < 4; ++i) va[i] = (d >> (8 * i)) & 255u;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < m) va[i] = a.valid_a[p0 + i];
        }
    }
    typename ST::word o[4];
    unsigned vd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[i] = ST::nan();
        vd[i] = 0u;
        if (i >= m || !vec_ok(q[i]) || !va[i]) continue;
        const float px = (float)(x0 + i) + q[i].x, py = (float)y + q[i].y;
        if (!inside(px, py, a.W, a.H)) continue;
        float su, sv;
        if (!sample_field<LB>(a.b, a.mask_b, base, a.W, a.H, px, py, &su, &sv)) continue;
        o[i] = ST::pack(make_float2(q[i].x + su, q[i].y + sv));
        vd[i] = 255u;
    }
    if (a.vec_out && m == 4) {  // (W even: p0 is, so both stores are aligned)
        ST::quad(a.out, p0, o);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) ST::one(a.out, p0 + i, o[i]);
    }
    if (!a.valid_out) return;
    if (a.vec_valid_out) {  // (W % 4 == 0: m == 4)
        *reinterpret_cast<unsigned*>(a.valid_out + p0) = pack4(vd);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) a.valid_out[p0 + i] = (uint8_t)vd[i];
    }
}

struct AdvectArgs {
    const void* flow;      // float2 or __half2 vectors
    const uint2* points;   // (x, y) float pairs as bits (may be `points_out`)
    uint2* points_out;
    uint8_t* status;       // may be null
    long long items;       // n * count points
    long long count;       // points per field
    int W, H;
};

template <class LB>
__global__ void __launch_bounds__(kAdvectThreads) k_flow_advect(AdvectArgs a)
{
    const long long t = (long long)blockIdx.x * kAdvectThreads + threadIdx.x;
    if (t >= a.items) return;
    const long long f = t / a.count;
    uint2 p = a.points[t];  // a point that stays put keeps its bits
    const float x = __uint_as_float(p.x), y = __uint_as_float(p.y);
    unsigned st = 0u;
    float su, sv;
    if (inside(x, y, a.W, a.H) &&
        sample_field<LB>(a.flow, nullptr, f * a.H * (long long)a.W, a.W, a.H, x, y, &su, &sv)) {
        p = make_uint2(__float_as_uint(x + su), __float_as_uint(y + sv));
        st = 255u;
    }
    a.points_out[t] = p;
    if (a.status) a.status[t] = (uint8_t)st;
}

template <class LA, class LB>
void launch_compose_ab(const ComposeArgs& a, bool out16, unsigned grid, hipStream_t s, Timing t)
{
    if (out16)
        DIS_LAUNCH(t, (k_flow_compose<LA, LB, StoreF16>), dim3(grid), dim3(kComposeThreads), 0, s, a);
    else
        DIS_LAUNCH(t, (k_flow_compose<LA, LB, StoreF32>), dim3(grid), dim3(kComposeThreads), 0, s, a);
}

}  // namespace

static_assert(kComposeThreads == kFlatThreads && kAdvectThreads == kFlatThreads,
              "flow_compose_blocks and flow_advect_blocks (dis_args.h) count blocks of 256 lanes");

hipError_t launch_flow_compose(const void* a, int a_f16, const void* b, int b_f16, int n, int W, int H,
                               const uint8_t* valid_a, const uint8_t* mask_b, void* out, int out_f16,
                               uint8_t* valid_out, hipStream_t s, Timing t)
{
    const long long blocks = flow_compose_blocks(n, W, H);
    if (blocks < 1) return hipErrorInvalidValue;
    const uintptr_t aa = reinterpret_cast<uintptr_t>(a), oa = reinterpret_cast<uintptr_t>(out);
    const uintptr_t va = reinterpret_cast<uintptr_t>(valid_a), vo = reinterpret_cast<uintptr_t>(valid_out);
    ComposeArgs g{};
    g.a = a;
    g.b = b;
    g.out = out;
    g.valid_a = valid_a;
    g.mask_b = mask_b;
    g.valid_out = valid_out;
    g.W = W;
    g.H = H;
    g.cw = (W + 3) / 4;
    g.items = (long long)n * H * g.cw;
    g.vec_a = ((aa & 15) == 0 && (W & (a_f16 ? 3 : 1)) == 0) ? 1 : 0;
    g.vec_valid_a = (valid_a && (va & 3) == 0 && (W & 3) == 0) ? 1 : 0;
    g.vec_out = ((oa & (out_f16 ? 7 : 15)) == 0 && (W & 1) == 0) ? 1 : 0;
    g.vec_valid_out = (valid_out && (vo & 3) == 0 && (W & 3) == 0) ? 1 : 0;
    const unsigned grid = (unsigned)blocks;
    if (a_f16 && b_f16)
        launch_compose_ab<LoadF16, LoadF16>(g, out_f16 != 0, grid, s, t);
    else if (a_f16)
        launch_compose_ab<LoadF16, LoadF32>(g, out_f16 != 0, grid, s, t);
    else if (b_f16)
        launch_compose_ab<LoadF32, LoadF16>(g, out_f16 != 0, grid, s, t);
    else
        launch_compose_ab<LoadF32, LoadF32>(g, out_f16 != 0, grid, s, t);
    return hipGetLastError();
}

hipError_t launch_flow_advect(const void* flow, int f16, int n, int W, int H, const float* points, int count,
                              float* points_out, uint8_t* status, hipStream_t s, Timing t)
{
    const long long blocks = flow_advect_blocks(n, count);
    if (blocks < 1) return hipErrorInvalidValue;
    AdvectArgs g{};
    g.flow = flow;
    g.points = reinterpret_cast<const uint2*>(points);
    g.points_out = reinterpret_cast<uint2*>(points_out);
    g.status = status;
    g.count = count;
    g.items = (long long)n * count;
    g.W = W;
    g.H = H;
    const unsigned grid = (unsigned)blocks;
    if (f16)
        DIS_LAUNCH(t, (k_flow_advect<LoadF16>), dim3(grid), dim3(kAdvectThreads), 0, s, g);
    else
        DIS_LAUNCH(t, (k_flow_advect<LoadF32>), dim3(grid), dim3(kAdvectThreads), 0, s, g);
    return hipGetLastError();
}

}  // namespace dis
