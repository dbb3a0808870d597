// dis_homography.hip -- the eight-parameter (projective) motion family beside
// dis_motion.hip's affine one: the fit of a homography to the trusted vectors
// of flow fields (dis_flow_fit_homography, include/dis_abi.h), the field of a
// model (dis_homography_to_flow) and the warp of images by models without a
// field (dis_warp_homography_u8). No reference counterpart.
//
// The fit is the linearised (algebraic) least-squares fit in centred coordinates
// scaled by a power of two, refitted on the vectors whose geometric residual
// against the previous model is within the threshold. It is defined by its
// arithmetic: 27 f64 sums per pass, added in dis_flow_fit_motion's order (slots
// of a chunk, the butterfly over the slots, the chunks in turn), then an 8 x 8
// LDL^T solve. Every operation is separately rounded (-ffp-contract=off), so
// tests/homographyref.py restates it bit for bit.
//
//   k_homography_accum    k_motion_accum with 27 terms a pixel;
//   k_homography_solve    a block per field: 27 lanes add the chunk sums in
//                         order, one lane solves, tests the model (finite, d >
//                         1/8 at the frame's corners) and writes the centred
//                         model for the next pass; the last pass also writes
//                         params and info;
//   k_homography_inliers  the plane of pixels that agree with the final model;
//   k_homography_flow     the field of eight parameters, four pixels a lane;
//   k_warp_homography     k_warp_motion's direct form (64 x 16 tile, four pixels
//                         a lane, the wide stores) with the projective vector.
#include <cmath>
#include <cstdint>

#include "dis_args.h"
#include "dis_half.h"
#include "dis_kernels.h"
#include "dis_motion.h"
#include "dis_sample.h"

namespace dis {
namespace {

constexpr int kHT = kHomographyTerms;
constexpr int kWhThreads = 256;  // 16 lanes x 16 rows

struct HomographyArgs {
    const void* flow;     // float2 or __half2 vectors
    const uint8_t* mask;  // may be null
    double* ws;           // per field: kMotionHead doubles (the centred model first), then 27 per chunk
    uint8_t* inliers;     // k_homography_inliers only
    unsigned* info;       // k_homography_inliers only; may be null
    long long px;         // W * H
    long long ws_field;   // doubles of a field's part of the workspace
    double t2s;           // threshold^2 / s^2
    double is;            // 1 / s (a power of two: the products with it are exact)
    int W, H, chunks;
    int f16;              // k_homography_inliers only: the field holds __half2 vectors
};

// The centred, scaled model of the previous pass and the test of a vector
// against it: the geometric residual, with its division.
struct HModel {
    double c[8], t2s;
    __device__ __forceinline__ void load(const double* head, double t2s_)
    {
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = head[i];
        t2s = t2s_;
    }
    __device__ __forceinline__ bool agrees(double a, double b, double U, double V) const  // false for a NaN model
    {
        const double g = c[6] * a + c[7] * b;
        const double d = 1.0 + g;
        const double eU = (((c[0] + c[1] * a) + c[2] * b) - a * g) / d;
        const double eV = (((c[3] + c[4] * a) + c[5] * b) - b * g) / d;
        const double rU = U - eU, rV = V - eV;
        return d > 0.0 && rU * rU + rV * rV <= t2s;
    }
};

// A lane's 64 pixels of one chunk into its 27 sums, in bursts of loads. FULL:
// the chunk lies inside the field; FIRST: pass 0, every trusted pixel is a member.
template <class LD, bool FULL, bool FIRST>
__device__ __forceinline__ void haccum_chunk(const HomographyArgs& h, const char* field, const uint8_t* mask,
                                             const HModel& m, Walk w, double cx, double cy, double* s)
{
    for (int k0 = 0; k0 < kMotionSteps; k0 += kMotionBurst) {
        float2 q[kMotionBurst];
        unsigned mb[kMotionBurst];
#pragma unroll
        for (int j = 0; j < kMotionBurst; ++j) {  // a pixel past the field's end is no member
            const long long p = w.q + (long long)j * kMotionThreads;
            const bool in = FULL || p < h.px;
            q[j] = make_float2(__uint_as_float(kNanBits), 0.0f);
            mb[j] = 255u;
            if (in) q[j] = LD::at(field, p);
            if (in && mask) mb[j] = mask[p];
        }
#pragma unroll
        for (int j = 0; j < kMotionBurst; ++j) {
            const double a = ((double)w.x - cx) * h.is, b = ((double)w.y - cy) * h.is;
            const double U = (double)q[j].x * h.is, V = (double)q[j].y * h.is;
            bool member = vec_ok(q[j]) && mb[j] != 0u;
            if (!FIRST) member = member && m.agrees(a, b, U, V);
            if (member) {
                const double A = a + U, B = b + V;
                const double aa = a * a, ab = a * b, bb = b * b;
                const double aA = a * A, bA = b * A, aB = a * B, bB = b * B;
                const double Q = A * A + B * B;
                s[0] += 1.0;
                s[1] += a;
                s[2] += b;
                s[3] += aa;
                s[4] += ab;
                s[5] += bb;
                s[6] += aA;
                s[7] += bA;
                s[8] += aa * A;
                s[9] += ab * A;
                s[10] += bb * A;
                s[11] += aB;
                s[12] += bB;
                s[13] += aa * B;
                s[14] += ab * B;
                s[15] += bb * B;
                s[16] += aa * Q;
                s[17] += ab * Q;
                s[18] += bb * Q;
                s[19] += U;
                s[20] += a * U;
                s[21] += b * U;
                s[22] += V;
                s[23] += a * V;
                s[24] += b * V;
                s[25] += aA * U + aB * V;
                s[26] += bA * U + bB * V;
            }
            w.next();
        }
    }
}

template <class LD, bool FIRST>
__global__ void __launch_bounds__(kMotionThreads) k_homography_accum(HomographyArgs h)
{
    __shared__ double part[kMotionThreads / 64][kHT];
    const int f = (int)(blockIdx.x / (unsigned)h.chunks), chunk = (int)(blockIdx.x - (unsigned)f * (unsigned)h.chunks);
    const int lane = threadIdx.x;
    const char* const field = static_cast<const char*>(h.flow) + (size_t)f * h.px * LD::kBytes;
    const uint8_t* const mask = h.mask ? h.mask + (size_t)f * h.px : nullptr;
    const double cx = (double)(h.W - 1) * 0.5, cy = (double)(h.H - 1) * 0.5;
    HModel m{};
    if (!FIRST) m.load(h.ws + f * h.ws_field, h.t2s);
    const Walk w((long long)chunk * kMotionChunk + lane, h.W);
    double s[kHT];
#pragma unroll
    for (int t = 0; t < kHT; ++t) s[t] = 0.0;
    if (((long long)chunk + 1) * kMotionChunk <= h.px)  // (the same for every lane of the block)
        haccum_chunk<LD, true, FIRST>(h, field, mask, m, w, cx, cy, s);
    else
        haccum_chunk<LD, false, FIRST>(h, field, mask, m, w, cx, cy, s);
    // slots 2i and 2i + 1, round after round: the lanes of a wave, then the waves
#pragma unroll
    for (int t = 0; t < kHT; ++t) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) s[t] += __shfl_xor(s[t], o, 64);
    }
    if ((lane & 63) == 0) {
#pragma unroll
        for (int t = 0; t < kHT; ++t) part[lane >> 6][t] = s[t];
    }
    __syncthreads();
    if (lane < kHT)
        h.ws[f * h.ws_field + kMotionHead + (long long)chunk * kHT + lane] =
            (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

struct HomographySolveArgs {
    double* ws;
    float* params;   // the last pass only
    unsigned* info;  // the last pass only; may be null
    long long ws_field;
    double s, is;    // the scale and 1 / s
    int W, H, chunks;
    int first, last;
};

// The centred, scaled model c of the 27 sums; false when a pivot fails.
__device__ __forceinline__ bool fit_homography(const double* S, double* c)
{
    double N[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) N[i][j] = 0.0;
    }
    const double G[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) N[i][j] = N[3 + i][3 + j] = G[i][j];
    }
    const double c6[6] = {-S[6], -S[8], -S[9], -S[11], -S[13], -S[14]};   // column 6, rows 0..5
    const double c7[6] = {-S[7], -S[9], -S[10], -S[12], -S[14], -S[15]};  // column 7
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        N[i][6] = N[6][i] = c6[i];
        N[i][7] = N[7][i] = c7[i];
    }
    N[6][6] = S[16];
    N[6][7] = N[7][6] = S[17];
    N[7][7] = S[18];
    double b[1][8] = {{S[19], S[20], S[21], S[22], S[23], S[24], -S[25], -S[26]}};
    if (!ldl_solve<8, 1>(N, b)) return false;
#pragma unroll
    for (int i = 0; i < 8; ++i) c[i] = b[0][i];
    return true;
}

__global__ void __launch_bounds__(kSolveThreads) k_homography_solve(HomographySolveArgs h)
{
    __shared__ double S[kHT];
    const long long f = blockIdx.x;  // (f * 8 passes 2^31 from 268,435,456 fields on)
    const int t = threadIdx.x;
    double* const head = h.ws + f * h.ws_field;
    if (t < kHT) {  // the chunks in turn; eight loads in flight
        const double* const p = head + kMotionHead + t;
        double acc = 0.0;
        for (int c0 = 0; c0 < h.chunks; c0 += 8) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = c0 + j < h.chunks ? p[(long long)(c0 + j) * kHT] : 0.0;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];  // (+0.0 past the last chunk changes nothing)
        }
        S[t] = acc;
    }
    __syncthreads();
    if (t != 0) return;
    double c[8];
    bool ok = fit_homography(S, c);
    const double cx = (double)(h.W - 1) * 0.5, cy = (double)(h.H - 1) * 0.5;
    const double a0 = (0.0 - cx) * h.is, a1 = ((double)(h.W - 1) - cx) * h.is;
    const double b0 = (0.0 - cy) * h.is, b1 = ((double)(h.H - 1) - cy) * h.is;
    double g00 = 0.0;
    if (ok) {
#pragma unroll
        for (int i = 0; i < 8; ++i) ok = ok && fabs(c[i]) <= 1.7976931348623157e308;  // false for NaN and the infinities
    }
    if (ok) {  // d at the four corners: a horizon near the frame is no camera shake
        g00 = c[6] * a0 + c[7] * b0;
        const double g10 = c[6] * a1 + c[7] * b0, g01 = c[6] * a0 + c[7] * b1, g11 = c[6] * a1 + c[7] * b1;
        ok = 1.0 + g00 > 0.125 && 1.0 + g10 > 0.125 && 1.0 + g01 > 0.125 && 1.0 + g11 > 0.125;
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = __longlong_as_double(0x7ff8000000000000ll);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) head[i] = c[i];
    if (h.first) head[8] = S[0];  // the trusted pixels
    if (!h.last) return;
    // conjugated back to frame coordinates and normalised by the bottom-right entry w = d(0, 0)
    const double w = 1.0 + g00, ax = cx * h.is, ay = cy * h.is;
    const double p[8] = {((((h.s * c[0]) - c[1] * cx) - c[2] * cy) + cx * g00) / w,
                         ((c[1] + ax * c[6]) - g00) / w,
                         (c[2] + ax * c[7]) / w,
                         ((((h.s * c[3]) - c[4] * cx) - c[5] * cy) + cy * g00) / w,
                         (c[4] + ay * c[6]) / w,
                         ((c[5] + ay * c[7]) - g00) / w,
                         (c[6] * h.is) / w,
                         (c[7] * h.is) / w};
#pragma unroll
    for (int i = 0; i < 8; ++i) h.params[f * 8 + i] = ok ? (float)p[i] : __uint_as_float(kNanBits);
    if (h.info) {
        unsigned* const o = h.info + f * 4;
        o[0] = ok ? 1u : 0u;
        o[1] = (unsigned)head[8];
        o[2] = (unsigned)S[0];
        o[3] = 0u;  // k_homography_inliers counts here
    }
}

__global__ void __launch_bounds__(kMotionThreads) k_homography_inliers(HomographyArgs h)
{
    const int f = (int)(blockIdx.x / (unsigned)h.chunks), chunk = (int)(blockIdx.x - (unsigned)f * (unsigned)h.chunks);
    const int lane = threadIdx.x;
    const uint8_t* const mask = h.mask ? h.mask + (size_t)f * h.px : nullptr;
    uint8_t* const out = h.inliers + (size_t)f * h.px;
    const double cx = (double)(h.W - 1) * 0.5, cy = (double)(h.H - 1) * 0.5;
    HModel m;
    m.load(h.ws + f * h.ws_field, h.t2s);
    Walk w((long long)chunk * kMotionChunk + lane, h.W);
    unsigned count = 0;
    for (int k = 0; k < kMotionSteps; ++k) {
        if (w.q < h.px) {
            const float2 q = h.f16 ? LoadF16::at(h.flow, f * h.px + w.q) : LoadF32::at(h.flow, f * h.px + w.q);
            bool in = vec_ok(q) && (!mask || mask[w.q] != 0);
            in = in && m.agrees(((double)w.x - cx) * h.is, ((double)w.y - cy) * h.is, (double)q.x * h.is,
                                (double)q.y * h.is);
            out[w.q] = in ? 255 : 0;
            count += in ? 1u : 0u;
        }
        w.next();
    }
    if (!h.info) return;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) count += __shfl_xor(count, o, 64);
    if ((lane & 63) == 0 && count) atomicAdd(h.info + (long long)f * 4 + 3, count);
}

// The vector of eight parameters at pixel (x, y); false where d is not > 0 (the
// pixel gets the canonical NaN). The division is the correctly rounded f32 one.
__device__ __forceinline__ bool homography_vector(const float* p, int x, int y, float2* q)
{
    const float fx = (float)x, fy = (float)y;
    const float g = p[6] * fx + p[7] * fy;
    const float d = 1.0f + g;
    q->x = (((p[0] + p[1] * fx) + p[2] * fy) - fx * g) / d;
    q->y = (((p[3] + p[4] * fx) + p[5] * fy) - fy * g) / d;
    return d > 0.0f;
}

__device__ __forceinline__ bool load_model(const float* params, long long f, float* p)  // false: not all finite
{
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        p[i] = params[f * 8 + i];
        finite = finite && fabsf(p[i]) <= 3.40282347e38f;  // false for NaN and the infinities
    }
    return finite;
}

struct HomographyFlowArgs {
    const float* params;  // eight per field
    void* out;
    long long items;      // n * H * cw lanes of work
    int W, H, cw;         // cw = ceil(W / 4) lanes per row
    int vec_out;          // out 16-byte (f16: 8-byte) aligned and W even: a lane's four vectors in two stores
};

template <class ST>
__global__ void __launch_bounds__(kMotionFlowThreads) k_homography_flow(HomographyFlowArgs a)
{
    const long long t = (long long)blockIdx.x * kMotionFlowThreads + threadIdx.x;
    if (t >= a.items) return;
    const long long row = t / a.cw;  // field * H + y
    const int x0 = (int)(t - row * a.cw) * 4;
    const long long f = row / a.H;
    const int y = (int)(row - f * a.H);
    const long long p0 = row * a.W + x0;
    const int m = min(4, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    float p[8];
    const bool finite = load_model(a.params, f, p);
    typename ST::word o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float2 q;
        const bool ahead = homography_vector(p, x0 + i, y, &q);
        o[i] = finite && ahead ? ST::pack(q) : ST::nan();
    }
    if (a.vec_out && m == 4) {  // (W even: p0 is, so both stores are aligned)
        ST::quad(a.out, p0, o);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) ST::one(a.out, p0 + i, o[i]);
    }
}

struct WarpHomographyArgs {
    const uint8_t* src;
    const float* params;  // eight per image
    uint8_t* dst;
    uint8_t* valid;       // may be null
    long long src_stride, src_image_stride;  // bytes
    int W, H;
    int tiles_x, tiles;   // tiles of a row of tiles, of an image
    int zero_border;      // DIS_BORDER_ZERO
    int vec_row;          // src and both strides 4-byte aligned: (4 channels) one dword per tap
    int vec_dst;          // dst 4-byte (4 channels: 16-byte) aligned and W % 4 == 0: dword / 16-byte stores
    int vec_valid;        // valid 4-byte aligned and W % 4 == 0: one dword per lane
};

template <int C>
__global__ void __launch_bounds__(kWhThreads) k_warp_homography(WarpHomographyArgs a)
{
    const long long f = blockIdx.x / (unsigned)a.tiles;
    const int tile = (int)(blockIdx.x - f * a.tiles);
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * kWarpMotionTileW + (int)(threadIdx.x & 15u) * 4, y = ty * kWarpMotionTileH + (int)(threadIdx.x >> 4);
    if (y >= a.H || x0 >= a.W) return;
    const uint8_t* const S = a.src + f * a.src_image_stride;
    float p[8];
    const bool finite = load_model(a.params, f, p);
    const int m = min(4, a.W - x0);  // pixels of this lane (a row's last lane may have fewer)
    const long long p0 = (f * a.H + y) * a.W + x0;
    unsigned o[4 * C];  // the lane's output bytes, in store order
    unsigned vd[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        vd[i] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) o[C * i + c] = 0u;
        if (i < m) {
            const float nanv = __uint_as_float(kNanBits);
            float2 q;
            if (!(homography_vector(p, x0 + i, y, &q) && finite)) q = make_float2(nanv, nanv);
            vd[i] = warp_pixel<C>(S, a.src_stride, x0 + i, y, a.W, a.H, q.x, q.y, 1.0f, a.zero_border, a.vec_row,
                                  &o[C * i]);
        }
    }
    uint8_t* const d = a.dst + p0 * C;
    if (a.vec_dst) {  // (W % 4 == 0: m == 4, p0 * C a multiple of 4, of 16 with 4 channels)
        if constexpr (C == 4) {
            *reinterpret_cast<uint4*>(d) = make_uint4(pack4(o), pack4(o + 4), pack4(o + 8), pack4(o + 12));
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) reinterpret_cast<unsigned*>(d)[k] = pack4(o + 4 * k);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) {
#pragma unroll
                for (int c = 0; c < C; ++c) d[C * i + c] = (uint8_t)o[C * i + c];
            }
    }
    if (!a.valid) return;
    if (a.vec_valid) {
        *reinterpret_cast<unsigned*>(a.valid + p0) = pack4(vd);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < m) a.valid[p0 + i] = (uint8_t)vd[i];
    }
}

}  // namespace

hipError_t launch_fit_homography(const void* flow, int f16, const uint8_t* mask, int n, int W, int H, int iterations,
                                 float threshold, float* params, unsigned* info, uint8_t* inliers, void* workspace,
                                 hipStream_t s)
{
    const long long blocks = motion_blocks(n, W, H);
    if (blocks < 1 || !workspace || iterations < 0) return hipErrorInvalidValue;
    const double sc = (double)homography_scale(W, H);
    HomographyArgs a{};
    a.flow = flow;
    a.mask = mask;
    a.ws = static_cast<double*>(workspace);
    a.px = (long long)W * H;
    a.chunks = (int)motion_chunks(W, H);
    a.ws_field = (long long)a.chunks * kHT + kMotionHead;
    a.t2s = ((double)threshold * (double)threshold) / (sc * sc);
    a.is = 1.0 / sc;
    a.W = W;
    a.H = H;
    HomographySolveArgs v{};
    v.ws = a.ws;
    v.params = params;
    v.info = info;
    v.ws_field = a.ws_field;
    v.s = sc;
    v.is = a.is;
    v.W = W;
    v.H = H;
    v.chunks = a.chunks;
    const dim3 grid((unsigned)blocks), block(kMotionThreads);
    for (int pass = 0; pass <= iterations; ++pass) {
        v.first = pass == 0;
        v.last = pass == iterations;
        if (f16 && pass == 0)
            hipLaunchKernelGGL((k_homography_accum<LoadF16, true>), grid, block, 0, s, a);
        else if (f16)
            hipLaunchKernelGGL((k_homography_accum<LoadF16, false>), grid, block, 0, s, a);
        else if (pass == 0)
            hipLaunchKernelGGL((k_homography_accum<LoadF32, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((k_homography_accum<LoadF32, false>), grid, block, 0, s, a);
        hipLaunchKernelGGL(k_homography_solve, dim3((unsigned)n), dim3(kSolveThreads), 0, s, v);
    }
    if (inliers) {
        a.inliers = inliers;
        a.info = info;
        a.f16 = f16;
        hipLaunchKernelGGL(k_homography_inliers, grid, block, 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_homography_flow(const float* params, int n, int W, int H, void* out, int out_f16, hipStream_t s)
{
    const long long blocks = motion_flow_blocks(n, W, H);
    if (blocks < 1) return hipErrorInvalidValue;
    const uintptr_t oa = reinterpret_cast<uintptr_t>(out);
    HomographyFlowArgs a{};
    a.params = params;
    a.out = out;
    a.W = W;
    a.H = H;
    a.cw = (W + 3) / 4;
    a.items = (long long)n * H * a.cw;
    a.vec_out = ((oa & (out_f16 ? 7 : 15)) == 0 && (W & 1) == 0) ? 1 : 0;
    if (out_f16)
        hipLaunchKernelGGL(k_homography_flow<StoreF16>, dim3((unsigned)blocks), dim3(kMotionFlowThreads), 0, s, a);
    else
        hipLaunchKernelGGL(k_homography_flow<StoreF32>, dim3((unsigned)blocks), dim3(kMotionFlowThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_warp_homography(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                                  const float* params, int n, int W, int H, int zero_border, uint8_t* dst,
                                  uint8_t* valid, hipStream_t s)
{
    const long long blocks = warp_motion_blocks(n, W, H);
    if (blocks < 1 || (channels != 1 && channels != 3 && channels != 4)) return hipErrorInvalidValue;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(src);
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), va = reinterpret_cast<uintptr_t>(valid);
    WarpHomographyArgs a{};
    a.src = src;
    a.params = params;
    a.dst = dst;
    a.valid = valid;
    a.src_stride = (long long)src_stride;
    a.src_image_stride = (long long)src_image_stride;
    a.W = W;
    a.H = H;
    a.tiles_x = (W + kWarpMotionTileW - 1) / kWarpMotionTileW;
    a.tiles = a.tiles_x * ((H + kWarpMotionTileH - 1) / kWarpMotionTileH);
    a.zero_border = zero_border;
    a.vec_row = (((sa | src_stride | src_image_stride) & 3) == 0) ? 1 : 0;
    a.vec_dst = ((da & (channels == 4 ? 15 : 3)) == 0 && (W & 3) == 0) ? 1 : 0;
    a.vec_valid = (valid && (va & 3) == 0 && (W & 3) == 0) ? 1 : 0;
    const dim3 grid((unsigned)blocks), block(kWhThreads);
    if (channels == 1)
        hipLaunchKernelGGL(k_warp_homography<1>, grid, block, 0, s, a);
    else if (channels == 3)
        hipLaunchKernelGGL(k_warp_homography<3>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(k_warp_homography<4>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace dis
