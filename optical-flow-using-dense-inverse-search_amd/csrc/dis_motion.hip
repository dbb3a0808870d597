// dis_motion.hip -- the global motion of flow fields: a translation, similarity
// or affine model fitted to the trusted vectors by least squares, refitted on
// the vectors that agree with it (dis_flow_fit_motion, include/dis_abi.h), and
// the field of a model (dis_motion_to_flow). No reference counterpart.
//
// The result is defined by its arithmetic: twelve f64 sums per pass, added in a
// fixed order (slots of a chunk, the butterfly over the slots, the chunks in
// turn), then an LDL^T solve. Every operation is separately rounded
// (-ffp-contract=off), so tests/motionref.py restates it bit for bit.
//
//   k_motion_accum    a block per chunk of 16384 pixels and field: lane i is slot
//                     i and adds the terms of pixels chunk * 16384 + k * 256 + i,
//                     k = 0..63, skipping the pixels that are no members (adding
//                     +0.0 changes no sum); the 256 slots are combined pairwise,
//                     six rounds across the lanes of a wave and two over the
//                     four waves through LDS; the twelve sums go to the
//                     workspace. Members of pass 0 are the trusted pixels, of a
//                     later pass those within the threshold of the previous
//                     pass's model, which the workspace holds. Specialised on
//                     pass 0 and, per block, on a chunk wholly inside the field:
//                     the pass is bound by instruction issue.
//   k_motion_solve    a block per field: twelve lanes add the chunk sums in
//                     order, one lane solves and writes the centred model for the
//                     next pass; the last pass also writes params and info.
//   k_motion_inliers  the plane of pixels that agree with the final model, and
//                     their count added to info (integer atomics: any order).
//   k_motion_flow     the field of six parameters, four pixels a lane.
#include <cmath>
#include <cstdint>

#include "dis_args.h"
#include "dis_half.h"
#include "dis_kernels.h"
#include "dis_motion.h"  // the loaders, Walk, ldl_solve and the field stores, shared with dis_homography.hip

namespace dis {
namespace {

struct MotionArgs {
    const void* flow;     // float2 or __half2 vectors
    const uint8_t* mask;  // may be null
    double* ws;           // per field: kMotionHead doubles (the centred model first), then twelve per chunk
    uint8_t* inliers;     // k_motion_inliers only
    unsigned* info;       // k_motion_inliers only; may be null
    long long px;         // W * H
    long long ws_field;   // doubles of a field's part of the workspace
    double t2;            // threshold^2
    int W, H, chunks;
    int f16;              // k_motion_inliers only: the field holds __half2 vectors
};

// The centred model of the previous pass and the test of a vector against it.
struct Model {
    double c[6], t2;
    __device__ __forceinline__ void load(const double* head, double t2_)
    {
#pragma unroll
        for (int i = 0; i < 6; ++i) c[i] = head[i];
        t2 = t2_;
    }
    __device__ __forceinline__ bool agrees(double xd, double yd, double u, double v) const  // false for a NaN model
    {
        const double eu = (c[0] + c[1] * xd) + c[2] * yd, ev = (c[3] + c[4] * xd) + c[5] * yd;
        const double ru = u - eu, rv = v - ev;
        return ru * ru + rv * rv <= t2;
    }
};

// A lane's 64 pixels of one chunk into its twelve sums, in bursts of loads.
// FULL: the chunk lies inside the field (no pixel needs the test against its
// end); FIRST: pass 0, every trusted pixel is a member.
template <class LD, bool FULL, bool FIRST>
__device__ __forceinline__ void accum_chunk(const MotionArgs& a, const char* field, const uint8_t* mask, const Model& m,
                                            Walk w, double cx, double cy, double* s)
{
    for (int k0 = 0; k0 < kMotionSteps; k0 += kMotionBurst) {
        float2 q[kMotionBurst];
        unsigned mb[kMotionBurst];
#pragma unroll
        for (int j = 0; j < kMotionBurst; ++j) {  // a pixel past the field's end is no member
            const long long p = w.q + (long long)j * kMotionThreads;
            const bool in = FULL || p < a.px;
            q[j] = make_float2(__uint_as_float(kNanBits), 0.0f);
            mb[j] = 255u;
            if (in) q[j] = LD::at(field, p);
            if (in && mask) mb[j] = mask[p];
        }
#pragma unroll
        for (int j = 0; j < kMotionBurst; ++j) {
            const double xd = (double)w.x - cx, yd = (double)w.y - cy;
            const double u = (double)q[j].x, v = (double)q[j].y;
            bool member = vec_ok(q[j]) && mb[j] != 0u;
            if (!FIRST) member = member && m.agrees(xd, yd, u, v);
            if (member) {
                s[0] += 1.0;
                s[1] += xd;
                s[2] += yd;
                s[3] += xd * xd;
                s[4] += xd * yd;
                s[5] += yd * yd;
                s[6] += u;
                s[7] += xd * u;
                s[8] += yd * u;
                s[9] += v;
                s[10] += xd * v;
                s[11] += yd * v;
            }
            w.next();
        }
    }
}

template <class LD, bool FIRST>
__global__ void __launch_bounds__(kMotionThreads) k_motion_accum(MotionArgs a)
{
    __shared__ double part[kMotionThreads / 64][kMotionTerms];
    const int f = (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x - (unsigned)f * (unsigned)a.chunks);
    const int lane = threadIdx.x;
    const char* const field = static_cast<const char*>(a.flow) + (size_t)f * a.px * LD::kBytes;
    const uint8_t* const mask = a.mask ? a.mask + (size_t)f * a.px : nullptr;
    const double cx = (double)(a.W - 1) * 0.5, cy = (double)(a.H - 1) * 0.5;
    Model m{};
    if (!FIRST) m.load(a.ws + f * a.ws_field, a.t2);
    const Walk w((long long)chunk * kMotionChunk + lane, a.W);
    double s[kMotionTerms];
#pragma unroll
    for (int t = 0; t < kMotionTerms; ++t) s[t] = 0.0;
    if (((long long)chunk + 1) * kMotionChunk <= a.px)  // (the same for every lane of the block)
        accum_chunk<LD, true, FIRST>(a, field, mask, m, w, cx, cy, s);
    else
        accum_chunk<LD, false, FIRST>(a, field, mask, m, w, cx, cy, s);
    // slots 2i and 2i + 1, round after round: the lanes of a wave, then the waves
#pragma unroll
    for (int t = 0; t < kMotionTerms; ++t) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) s[t] += __shfl_xor(s[t], o, 64);
    }
    if ((lane & 63) == 0) {
#pragma unroll
        for (int t = 0; t < kMotionTerms; ++t) part[lane >> 6][t] = s[t];
    }
    __syncthreads();
    if (lane < kMotionTerms)
        a.ws[f * a.ws_field + kMotionHead + (long long)chunk * kMotionTerms + lane] =
            (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// The centred model c of the sums S (1, x, y, xx, xy, yy, u, xu, yu, v, xv, yv).
template <int MODEL>
__device__ __forceinline__ bool fit_model(const double* S, double* c)
{
    if (MODEL == DIS_MOTION_AFFINE) {
        const double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
        double b[2][3] = {{S[6], S[7], S[8]}, {S[9], S[10], S[11]}};
        if (!ldl_solve<3, 2>(A, b)) return false;
        c[0] = b[0][0], c[1] = b[0][1], c[2] = b[0][2], c[3] = b[1][0], c[4] = b[1][1], c[5] = b[1][2];
        return true;
    }
    if (MODEL == DIS_MOTION_SIMILARITY) {  // (tx, ty, s, r): u = tx + s x' - r y', v = ty + r x' + s y'
        const double q = S[3] + S[5];
        const double A[4][4] = {{S[0], 0.0, S[1], -S[2]}, {0.0, S[0], S[2], S[1]}, {S[1], S[2], q, 0.0}, {-S[2], S[1], 0.0, q}};
        double b[1][4] = {{S[6], S[9], S[7] + S[11], S[10] - S[8]}};
        if (!ldl_solve<4, 1>(A, b)) return false;
        c[0] = b[0][0], c[1] = b[0][2], c[2] = -b[0][3], c[3] = b[0][1], c[4] = b[0][3], c[5] = b[0][2];
        return true;
    }
    const double A[1][1] = {{S[0]}};
    double b[2][1] = {{S[6]}, {S[9]}};
    if (!ldl_solve<1, 2>(A, b)) return false;
    c[0] = b[0][0], c[1] = 0.0, c[2] = 0.0, c[3] = b[1][0], c[4] = 0.0, c[5] = 0.0;
    return true;
}

struct MotionSolveArgs {
    double* ws;
    float* params;   // the last pass only
    unsigned* info;  // the last pass only; may be null
    long long ws_field;
    int W, H, chunks;
    int first, last;
};

template <int MODEL>
__global__ void __launch_bounds__(kSolveThreads) k_motion_solve(MotionSolveArgs a)
{
    __shared__ double S[kMotionTerms];
    const long long f = blockIdx.x;  // (f * 6 passes 2^31 from 357,913,942 fields on)
    const int t = threadIdx.x;
    double* const head = a.ws + f * a.ws_field;
    if (t < kMotionTerms) {  // the chunks in turn; eight loads in flight
        const double* const p = head + kMotionHead + t;
        double acc = 0.0;
        for (int c0 = 0; c0 < a.chunks; c0 += 8) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = c0 + j < a.chunks ? p[(long long)(c0 + j) * kMotionTerms] : 0.0;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];  // (+0.0 past the last chunk changes nothing)
        }
        S[t] = acc;
    }
    __syncthreads();
    if (t != 0) return;
    double c[6];
    const bool ok = fit_model<MODEL>(S, c);
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 6; ++i) c[i] = __longlong_as_double(0x7ff8000000000000ll);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) head[i] = c[i];
    if (a.first) head[6] = S[0];  // the trusted pixels
    if (!a.last) return;
    const double cx = (double)(a.W - 1) * 0.5, cy = (double)(a.H - 1) * 0.5;
    const double p[6] = {(c[0] - c[1] * cx) - c[2] * cy, c[1], c[2], (c[3] - c[4] * cx) - c[5] * cy, c[4], c[5]};
#pragma unroll
    for (int i = 0; i < 6; ++i) a.params[f * 6 + i] = ok ? (float)p[i] : __uint_as_float(kNanBits);
    if (a.info) {
        unsigned* const o = a.info + f * 4;
        o[0] = ok ? 1u : 0u;
        o[1] = (unsigned)head[6];
        o[2] = (unsigned)S[0];
        o[3] = 0u;  // k_motion_inliers counts here
    }
}

__global__ void __launch_bounds__(kMotionThreads) k_motion_inliers(MotionArgs a)
{
    const int f = (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x - (unsigned)f * (unsigned)a.chunks);
    const int lane = threadIdx.x;
    const uint8_t* const mask = a.mask ? a.mask + (size_t)f * a.px : nullptr;
    uint8_t* const out = a.inliers + (size_t)f * a.px;
    const double cx = (double)(a.W - 1) * 0.5, cy = (double)(a.H - 1) * 0.5;
    Model m;
    m.load(a.ws + f * a.ws_field, a.t2);
    Walk w((long long)chunk * kMotionChunk + lane, a.W);
    unsigned count = 0;
    for (int k = 0; k < kMotionSteps; ++k) {
        if (w.q < a.px) {
            const float2 q = a.f16 ? LoadF16::at(a.flow, f * a.px + w.q) : LoadF32::at(a.flow, f * a.px + w.q);
            bool in = vec_ok(q) && (!mask || mask[w.q] != 0);
            in = in && m.agrees((double)w.x - cx, (double)w.y - cy, (double)q.x, (double)q.y);
            out[w.q] = in ? 255 : 0;
            count += in ? 1u : 0u;
        }
        w.next();
    }
    if (!a.info) return;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) count += __shfl_xor(count, o, 64);
    if ((lane & 63) == 0 && count) atomicAdd(a.info + (long long)f * 4 + 3, count);
}

struct MotionFlowArgs {
    const float* params;  // six per field
    void* out;
    long long items;      // n * H * cw lanes of work
    int W, H, cw;         // cw = ceil(W / 4) lanes per row
    int vec_out;          // out 16-byte (f16: 8-byte) aligned and W even: a lane's four vectors in two stores
};

template <class ST>
__global__ void __launch_bounds__(kMotionFlowThreads) k_motion_flow(MotionFlowArgs a)
{
    const long long t = (long long)blockIdx.x * kMotionFlowThreads + threadIdx.x;
    if (t >= a.items) return;
    const long long row = t / a.cw;  // field * H + y
    const int x0 = (int)(t - row * a.cw) * 4;
    const long long f = row / a.H;
    const float y = (float)(int)(row - f * a.H);
    const long long p0 = row * a.W + x0;
    const int m = min(4, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    float p[6];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        p[i] = a.params[f * 6 + i];
        finite = finite && fabsf(p[i]) <= 3.40282347e38f;  // false for NaN and the infinities
    }
    typename ST::word o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x = (float)(x0 + i);
        o[i] = finite ? ST::pack(make_float2((p[0] + p[1] * x) + p[2] * y, (p[3] + p[4] * x) + p[5] * y)) : ST::nan();
    }
    if (a.vec_out && m == 4) {  // (W even: p0 is, so both stores are aligned)
        ST::quad(a.out, p0, o);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) ST::one(a.out, p0 + i, o[i]);
    }
}

template <int MODEL>
void launch_solve(const MotionSolveArgs& a, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_motion_solve<MODEL>, dim3((unsigned)n), dim3(kSolveThreads), 0, s, a);
}

}  // namespace

hipError_t launch_fit_motion(const void* flow, int f16, const uint8_t* mask, int n, int W, int H, int model, int iterations,
                             float threshold, float* params, unsigned* info, uint8_t* inliers, void* workspace,
                             hipStream_t s)
{
    const long long blocks = motion_blocks(n, W, H);
    if (blocks < 1 || !workspace || iterations < 0) return hipErrorInvalidValue;
    MotionArgs a{};
    a.flow = flow;
    a.mask = mask;
    a.ws = static_cast<double*>(workspace);
    a.px = (long long)W * H;
    a.chunks = (int)motion_chunks(W, H);
    a.ws_field = (long long)a.chunks * kMotionTerms + kMotionHead;
    a.t2 = (double)threshold * (double)threshold;
    a.W = W;
    a.H = H;
    MotionSolveArgs v{};
    v.ws = a.ws;
    v.params = params;
    v.info = info;
    v.ws_field = a.ws_field;
    v.W = W;
    v.H = H;
    v.chunks = a.chunks;
    const dim3 grid((unsigned)blocks), block(kMotionThreads);
    for (int pass = 0; pass <= iterations; ++pass) {
        v.first = pass == 0;
        v.last = pass == iterations;
        if (f16 && pass == 0)
            hipLaunchKernelGGL((k_motion_accum<LoadF16, true>), grid, block, 0, s, a);
        else if (f16)
            hipLaunchKernelGGL((k_motion_accum<LoadF16, false>), grid, block, 0, s, a);
        else if (pass == 0)
            hipLaunchKernelGGL((k_motion_accum<LoadF32, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((k_motion_accum<LoadF32, false>), grid, block, 0, s, a);
        if (model == DIS_MOTION_AFFINE)
            launch_solve<DIS_MOTION_AFFINE>(v, n, s);
        else if (model == DIS_MOTION_SIMILARITY)
            launch_solve<DIS_MOTION_SIMILARITY>(v, n, s);
        else
            launch_solve<DIS_MOTION_TRANSLATION>(v, n, s);
    }
    if (inliers) {
        a.inliers = inliers;
        a.info = info;
        a.f16 = f16;
        hipLaunchKernelGGL(k_motion_inliers, grid, block, 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_motion_flow(const float* params, int n, int W, int H, void* out, int out_f16, hipStream_t s)
{
    const long long blocks = motion_flow_blocks(n, W, H);
    if (blocks < 1) return hipErrorInvalidValue;
    const uintptr_t oa = reinterpret_cast<uintptr_t>(out);
    MotionFlowArgs a{};
    a.params = params;
    a.out = out;
    a.W = W;
    a.H = H;
    a.cw = (W + 3) / 4;
    a.items = (long long)n * H * a.cw;
    a.vec_out = ((oa & (out_f16 ? 7 : 15)) == 0 && (W & 1) == 0) ? 1 : 0;
    if (out_f16)
        hipLaunchKernelGGL(k_motion_flow<StoreF16>, dim3((unsigned)blocks), dim3(kMotionFlowThreads), 0, s, a);
    else
        hipLaunchKernelGGL(k_motion_flow<StoreF32>, dim3((unsigned)blocks), dim3(kMotionFlowThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dis
