// dis_fill.hip -- untrusted flow vectors replaced from trusted ones by
// validity-weighted push-pull (dis_flow_fill, include/dis_abi.h; Gortler et
// al., "The Lumigraph", section 4). No reference counterpart.
//
// Pull: level l+1 averages the trusted children of each cell (m = f + sum of
// differences to the first trusted child f, times k[count]: exact when the
// children are equal); a cell without a trusted child is stored as the
// canonical NaN. Push: from the 1 x 1 top down, a cell that is not trusted gets
// the bilinear 9/3/3/1 upsample of the complete level above it, in lerp form.
// Every float operation is separately rounded (-ffp-contract=off), so
// tests/fillref.py restates it bit for bit.
//
// Three stages instead of a launch per level:
//   k_fill_pull  a block reduces one 64 x 32 tile of level lo (its origin a
//                multiple of the tile, so a cell's children 2X, 2X+1 lie in the
//                tile: no halo) to levels lo+1 .. lo+5 in LDS and writes them to
//                the workspace; lo = 0 reads the caller's field and mask;
//   k_fill_top   one block per field pulls the pass's last level up to 1 x 1 and
//                pushes back down, all in LDS, and writes only the cells it
//                filled; when that level does not fit the block, another tile
//                pass runs on it first (launch_flow_fill's loop);
//   k_fill_push  a block loads its tile's cells of level lo+5 with a halo, the
//                pulled levels lo+4 .. lo+1 with theirs, expands in LDS and
//                writes level lo: the output and the level map for lo = 0.
// The level a filled cell's data came from travels down beside the vectors: a
// stage that fills a cell of level b writes the level into the NaN of the cell's
// first child in level b-1 (bits 0x7fc00000 | level: still a NaN, still "not
// trusted"), where only the pass below reads it. `out` may be `flow` itself: a
// lane reads its own pixels before it writes them and no other lane reads them.
#include <cmath>
#include <cstdint>

#include "dis_args.h"
#include "dis_half.h"
#include "dis_kernels.h"
#include "dis_sample.h"

namespace dis {
namespace {

constexpr int kFillThreads = 256;
constexpr int kFillSpan = 5;         // levels of one tile pass
constexpr int kFillTopThreads = 512;
constexpr int kFillTopCells = 6208;  // LDS cells of the top block: 8 + 1 bytes each; 56,196 bytes with the levels' sizes
constexpr unsigned kNanBits = 0x7fc00000u;

__device__ __forceinline__ float2 nan2()
{
    const float q = __uint_as_float(kNanBits);
    return make_float2(q, q);
}
__device__ __forceinline__ bool cell_ok(float2 m) { return m.x == m.x; }  // a pulled cell: NaN = no trusted child

// The level-lo cells of a tile pass: the caller's field (trusted: the vector
// test; the mask is the kernels') or a level of the workspace.
struct SrcF32 {
    static constexpr bool kF16 = false, kField = true;
    static __device__ __forceinline__ bool ok(float2 q) { return fabsf(q.x) < 1e9f && fabsf(q.y) < 1e9f; }  // false for NaN
};
struct SrcF16 {
    static constexpr bool kF16 = true, kField = true;
    static __device__ __forceinline__ bool ok(float2 q) { return fabsf(q.x) < 1e9f && fabsf(q.y) < 1e9f; }
};
struct SrcCells {
    static constexpr bool kF16 = false, kField = false;
    static __device__ __forceinline__ bool ok(float2 q) { return cell_ok(q); }
};

// What a push pass writes: `word` is one stored vector; quad: a lane's four at
// once (p0 even and the pointer aligned to 16 bytes for f32, 8 for f16).
struct StoreF32 {
    using word = float2;
    static __device__ __forceinline__ word pack(float2 v) { return v; }
    static __device__ __forceinline__ word nan() { return nan2(); }
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

// One cell of level l+1 from its four children (c00, c01, c10, c11) of level l.
// The differences are selects: an untrusted vector never reaches the sums.
__device__ __forceinline__ float2 pull_cell(float2 v00, bool o00, float2 v01, bool o01, float2 v10, bool o10, float2 v11,
                                            bool o11)
{
    const int c = (int)o00 + (int)o01 + (int)o10 + (int)o11;
    const float2 f = o00 ? v00 : o01 ? v01 : o10 ? v10 : v11;
    const float k = c == 1 ? 1.0f : c == 2 ? 0.5f : c == 3 ? __uint_as_float(0x3eaaaaabu) : 0.25f;
    const float ax = o00 ? v00.x - f.x : 0.0f, ay = o00 ? v00.y - f.y : 0.0f;
    const float bx = o01 ? v01.x - f.x : 0.0f, by = o01 ? v01.y - f.y : 0.0f;
    const float cx = o10 ? v10.x - f.x : 0.0f, cy = o10 ? v10.y - f.y : 0.0f;
    const float dx = o11 ? v11.x - f.x : 0.0f, dy = o11 ? v11.y - f.y : 0.0f;
    const float2 m = make_float2(f.x + ((ax + bx) + (cx + dx)) * k, f.y + ((ay + by) + (cy + dy)) * k);
    return c ? m : nan2();
}

// r of cell (x, y) from the complete level above it (w1 x h1), of which `g1`
// holds the rows from oy and the columns from ox on, rw cells a row; the caller
// has made sure that the four taps lie in that window. `parent`: the index of
// the cell's parent in the window.
__device__ __forceinline__ float2 push_cell(const float2* g1, int rw, int ox, int oy, int w1, int h1, int x, int y,
                                            int* parent)
{
    const int px = x >> 1, py = y >> 1;
    const int qx = min(max(px + ((x & 1) ? 1 : -1), 0), w1 - 1);
    const int qy = min(max(py + ((y & 1) ? 1 : -1), 0), h1 - 1);
    const int rp = (py - oy) * rw - ox, rq = (qy - oy) * rw - ox;
    const float2 P = g1[rp + px], Q = g1[rp + qx], R = g1[rq + px], S = g1[rq + qx];
    const float h0x = P.x + 0.25f * (Q.x - P.x), h0y = P.y + 0.25f * (Q.y - P.y);
    const float h1x = R.x + 0.25f * (S.x - R.x), h1y = R.y + 0.25f * (S.y - R.y);
    *parent = rp + px;
    return make_float2(h0x + 0.25f * (h1x - h0x), h0y + 0.25f * (h1y - h0y));
}

// The level of an untrusted cell as its first child's NaN carries it downwards.
__device__ __forceinline__ float2 level_note(unsigned lv)
{
    return make_float2(__uint_as_float(kNanBits | lv), __uint_as_float(kNanBits));
}

// One tile pass over levels lo .. lo+nl of n fields. Index k means level lo+k.
struct FillTileArgs {
    const void* src;      // level lo of field 0: the caller's field (lo == 0) or its cells in the workspace
    const uint8_t* mask;  // lo == 0: trust bytes, may be null
    void* dst;            // push: level lo of field 0 (out, or the same cells as src)
    uint8_t* level;       // push, lo == 0: the level map, may be null
    float2* ws;           // the workspace
    long long ws_field;   // its cells per field
    long long src_field;  // vectors per field of src and dst (W * H, or ws_field)
    long long off[kFillSpan + 1];  // level lo+k of field 0 begins at ws + off[k] (k >= 1; k == 0 when lo > 0)
    long long note_off;   // push, lo > 0: level lo-1 likewise, for the level notes; note_w its width
    int note_w;
    int w[kFillSpan + 1], h[kFillSpan + 1];
    int lo, nl;           // nl in 0..5 levels above lo (0: a 1 x 1 field)
    int tx, ty;           // tiles per field
    int vec_src;          // 16-byte loads of a lane's four vectors (see load_flow4)
    int vec_mask;         // mask 4-byte aligned and W % 4 == 0: one dword per lane
    int vec_dst;          // dst 16-byte (f16: 8-byte) aligned and the width even: two stores per lane
    int vec_level;        // level 4-byte aligned and W % 4 == 0: one dword per lane
};

// A lane's four cells of level lo from x0 on in row y of field f (m of them in
// the row), widened, and which of them are trusted.
template <class SRC>
__device__ __forceinline__ void load_quad(const FillTileArgs& a, long long f, int x0, int y, int m, float2* q, bool* ok)
{
    const long long p0 = f * a.src_field + (long long)y * a.w[0] + x0;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = make_float2(0.0f, 0.0f);
    load_flow4<SRC::kF16>(a.src, p0, m, a.vec_src, q);
    unsigned mb[4] = {255u, 255u, 255u, 255u};
    if (SRC::kField && a.mask) {
        if (a.vec_mask) {  // (W % 4 == 0: m == 4)
            const unsigned d = *reinterpret_cast<const unsigned*>(a.mask + p0);
#pragma unroll
            for (int i = 0; i < 4; ++i) mb[i] = (d >> (8 * i)) & 255u;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < m) mb[i] = a.mask[p0 + i];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) ok[i] = i < m && SRC::ok(q[i]) && mb[i] != 0u;
}

// Level k (k >= 2) of the tile from level k-1 in LDS (sw cells a row), into LDS
// and the workspace. Cells beyond the level's sides were stored as NaN.
__device__ __forceinline__ void pull_from_lds(const FillTileArgs& a, long long f, int k, int X0, int Y0,
                                              const float2* src, int sw, float2* dst)
{
    const int dw = kFillTileW >> k, dh = kFillTileH >> k;
    for (int i = threadIdx.x; i < dw * dh; i += kFillThreads) {
        const int X = i % dw, Y = i / dw;
        const float2* const r0 = src + (2 * Y) * sw + 2 * X;
        const float2 v00 = r0[0], v01 = r0[1], v10 = r0[sw], v11 = r0[sw + 1];
        const float2 m = pull_cell(v00, cell_ok(v00), v01, cell_ok(v01), v10, cell_ok(v10), v11, cell_ok(v11));
        dst[i] = m;
        const int gx = (X0 >> k) + X, gy = (Y0 >> k) + Y;
        if (gx < a.w[k] && gy < a.h[k]) a.ws[f * a.ws_field + a.off[k] + (long long)gy * a.w[k] + gx] = m;
    }
}

template <class SRC>
__global__ void __launch_bounds__(kFillThreads) k_fill_pull(FillTileArgs a)
{
    __shared__ float2 s1[(kFillTileW >> 1) * (kFillTileH >> 1)];
    __shared__ float2 s2[(kFillTileW >> 2) * (kFillTileH >> 2)];
    __shared__ float2 s3[(kFillTileW >> 3) * (kFillTileH >> 3)];
    __shared__ float2 s4[(kFillTileW >> 4) * (kFillTileH >> 4)];
    __shared__ float2 s5[(kFillTileW >> 5) * (kFillTileH >> 5)];
    long long b = blockIdx.x;
    const int bx = (int)(b % a.tx);
    b /= a.tx;
    const int by = (int)(b % a.ty);
    const long long f = b / a.ty;
    const int X0 = bx * kFillTileW, Y0 = by * kFillTileH;
    {
        // level 1: a lane's two cells from four cells each of two rows
        const int cx = (threadIdx.x & 15) * 2, cy = threadIdx.x >> 4;
        const int x0 = X0 + 2 * cx, y0 = Y0 + 2 * cy;
        const int m = min(4, a.w[0] - x0);
        float2 q[2][4];
        bool ok[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (m > 0 && y0 + r < a.h[0]) {
                load_quad<SRC>(a, f, x0, y0 + r, m, q[r], ok[r]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) q[r][i] = make_float2(0.0f, 0.0f), ok[r][i] = false;
            }
        }
        const float2 m0 = pull_cell(q[0][0], ok[0][0], q[0][1], ok[0][1], q[1][0], ok[1][0], q[1][1], ok[1][1]);
        const float2 m1 = pull_cell(q[0][2], ok[0][2], q[0][3], ok[0][3], q[1][2], ok[1][2], q[1][3], ok[1][3]);
        s1[cy * (kFillTileW >> 1) + cx] = m0;
        s1[cy * (kFillTileW >> 1) + cx + 1] = m1;
        const int gx = (X0 >> 1) + cx, gy = (Y0 >> 1) + cy;
        if (gy < a.h[1]) {
            float2* const row = a.ws + f * a.ws_field + a.off[1] + (long long)gy * a.w[1];
            if (gx < a.w[1]) row[gx] = m0;
            if (gx + 1 < a.w[1]) row[gx + 1] = m1;
        }
    }
    if (a.nl < 2) return;
    __syncthreads();
    pull_from_lds(a, f, 2, X0, Y0, s1, kFillTileW >> 1, s2);
    if (a.nl < 3) return;
    __syncthreads();
    pull_from_lds(a, f, 3, X0, Y0, s2, kFillTileW >> 2, s3);
    if (a.nl < 4) return;
    __syncthreads();
    pull_from_lds(a, f, 4, X0, Y0, s3, kFillTileW >> 3, s4);
    if (a.nl < 5) return;
    __syncthreads();
    pull_from_lds(a, f, 5, X0, Y0, s4, kFillTileW >> 4, s5);
}

// The top of a field: levels `base` (w x h cells, at ws + off of field 0) to L.
struct FillTopArgs {
    float2* ws;
    long long ws_field;
    long long off;       // level `base` of field 0
    long long note_off;  // level base-1 likewise, for the level notes (base > 1); note_w its width
    int note_w;
    int w, h, base;
};

__global__ void __launch_bounds__(kFillTopThreads) k_fill_top(FillTopArgs a)
{
    __shared__ float2 cell[kFillTopCells];
    __shared__ uint8_t lev[kFillTopCells];
    __shared__ int gw[kMaxFillLevels], gh[kMaxFillLevels], go[kMaxFillLevels], gn;
    const int tid = threadIdx.x;
    if (tid == 0) {  // the levels' sides and where they begin in `cell`
        int w = a.w, h = a.h, o = 0, k = 0;
        for (;; ++k) {
            gw[k] = w, gh[k] = h, go[k] = o;
            if (w == 1 && h == 1) break;
            o += w * h;
            w = (w + 1) / 2, h = (h + 1) / 2;
        }
        gn = k;
    }
    __syncthreads();
    const int nk = gn;
    float2* const g0 = a.ws + blockIdx.x * a.ws_field + a.off;
    for (int i = tid; i < a.w * a.h; i += kFillTopThreads) cell[i] = g0[i];
    for (int k = 0; k < nk; ++k) {
        __syncthreads();
        const int sw = gw[k], sh = gh[k], dw = gw[k + 1], dh = gh[k + 1];
        const float2* const src = cell + go[k];
        float2* const dst = cell + go[k + 1];
        for (int i = tid; i < dw * dh; i += kFillTopThreads) {
            const int X = i % dw, Y = i / dw;
            const bool in_x = 2 * X + 1 < sw, in_y = 2 * Y + 1 < sh;
            const float2* const r0 = src + (2 * Y) * sw + 2 * X;
            const float2 v00 = r0[0], v01 = in_x ? r0[1] : nan2();
            const float2 v10 = in_y ? r0[sw] : nan2(), v11 = in_x && in_y ? r0[sw + 1] : nan2();
            dst[i] = pull_cell(v00, cell_ok(v00), v01, cell_ok(v01), v10, cell_ok(v10), v11, cell_ok(v11));
        }
    }
    __syncthreads();
    if (!cell_ok(cell[go[nk]])) return;  // an empty field: every cell below stays NaN
    if (tid == 0) lev[go[nk]] = (uint8_t)(a.base + nk);
    for (int k = nk - 1; k >= 0; --k) {
        __syncthreads();
        const int w = gw[k], h = gh[k], w1 = gw[k + 1], h1 = gh[k + 1];
        float2* const cur = cell + go[k];
        const float2* const up = cell + go[k + 1];
        for (int i = tid; i < w * h; i += kFillTopThreads) {
            unsigned lv = (unsigned)(a.base + k);
            if (!cell_ok(cur[i])) {
                const int x = i % w, y = i / w;
                int parent;
                const float2 r = push_cell(up, w1, 0, 0, w1, h1, x, y, &parent);
                lv = lev[go[k + 1] + parent];
                cur[i] = r;
                if (k == 0) {  // only what was filled goes back to the workspace
                    g0[i] = r;
                    if (a.base > 1)
                        a.ws[blockIdx.x * a.ws_field + a.note_off + (long long)(2 * y) * a.note_w + 2 * x] = level_note(lv);
                }
            }
            lev[go[k] + i] = (uint8_t)lv;
        }
    }
}

// The windows of a push tile: level k's own cells and a halo of kHalo[k] cells
// on every side, which the taps of level k-1's window need (its parents and
// their neighbours): 1, then ceil(halo / 2) + 1 = 2.
constexpr int halo(int k) { return k == 0 ? 0 : k == 1 ? 1 : 2; }
constexpr int win_w(int k) { return (kFillTileW >> k) + 2 * halo(k); }
constexpr int win_h(int k) { return (kFillTileH >> k) + 2 * halo(k); }
constexpr int win_at(int k)  // where window k begins in the block's LDS
{
    return k <= 1 ? 0 : win_at(k - 1) + win_w(k - 1) * win_h(k - 1);
}
constexpr int kWinCells = 34 * 18 + 20 * 12 + 12 * 8 + 8 * 6 + 6 * 5;

template <class SRC, class ST>
__global__ void __launch_bounds__(kFillThreads) k_fill_push(FillTileArgs a)
{
    static_assert(win_at(kFillSpan) + win_w(kFillSpan) * win_h(kFillSpan) == kWinCells, "window sizes");
    __shared__ float2 g[kWinCells];
    __shared__ uint8_t lev[kWinCells];
    long long b = blockIdx.x;
    const int bx = (int)(b % a.tx);
    b /= a.tx;
    const int by = (int)(b % a.ty);
    const long long f = b / a.ty;
    const int X0 = bx * kFillTileW, Y0 = by * kFillTileH;
    float2* const wsf = a.ws + f * a.ws_field;
#pragma unroll
    for (int k = kFillSpan; k >= 1; --k) {
        if (k > a.nl) continue;
        const int rw = win_w(k), rh = win_h(k), at = win_at(k);
        const int ox = (X0 >> k) - halo(k), oy = (Y0 >> k) - halo(k);
        if (k < a.nl) __syncthreads();
        for (int i = threadIdx.x; i < rw * rh; i += kFillThreads) {
            const int x = ox + i % rw, y = oy + i / rw;
            if (x < 0 || y < 0 || x >= a.w[k] || y >= a.h[k]) continue;
            float2 v = wsf[a.off[k] + (long long)y * a.w[k] + x];
            unsigned lv = (unsigned)(a.lo + k);
            if (k == a.nl) {
                // the pass's last level is complete, unless the field is empty; the level of
                // a cell filled from above is noted in its first child (own cells only: only
                // this block writes their children; a halo cell's lev[] may therefore be wrong,
                // and is never consumed: the parent of an own cell is an own cell)
                const bool own = x >= (X0 >> k) && x < (X0 >> k) + (kFillTileW >> k) && y >= (Y0 >> k) &&
                                 y < (Y0 >> k) + (kFillTileH >> k);
                if (!cell_ok(v)) {
                    lv = 255u;
                } else if (own && a.lo + k > 1) {
                    const unsigned bits =
                        __float_as_uint(wsf[a.off[k - 1] + (long long)(2 * y) * a.w[k - 1] + 2 * x].x);
                    if ((bits & 0xffffff00u) == kNanBits && (bits & 255u)) lv = bits & 255u;
                }
            } else if (!cell_ok(v)) {
                int parent;
                v = push_cell(g + win_at(k + 1), win_w(k + 1), (X0 >> (k + 1)) - halo(k + 1),
                              (Y0 >> (k + 1)) - halo(k + 1), a.w[k + 1], a.h[k + 1], x, y, &parent);
                lv = lev[win_at(k + 1) + parent];
            }
            g[at + i] = v;
            lev[at + i] = (uint8_t)lv;
        }
    }
    __syncthreads();
    // level lo: a lane's four cells at a time, read before they are written
#pragma unroll
    for (int it = 0; it < kFillTileW * kFillTileH / (4 * kFillThreads); ++it) {
        const int j = threadIdx.x + it * kFillThreads;
        const int x0 = X0 + (j % (kFillTileW / 4)) * 4, y = Y0 + j / (kFillTileW / 4);
        const int m = min(4, a.w[0] - x0);
        if (m <= 0 || y >= a.h[0]) continue;
        float2 q[4];
        bool ok[4];
        load_quad<SRC>(a, f, x0, y, m, q, ok);
        const long long p0 = f * a.src_field + (long long)y * a.w[0] + x0;
        typename ST::word o[4];
        unsigned lv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[i] = ST::pack(q[i]);
            lv[i] = (unsigned)a.lo;
            if (ok[i] || i >= m) continue;
            lv[i] = 255u;
            float2 r = nan2();
            if (a.nl > 0) {
                int parent;
                r = push_cell(g, win_w(1), (X0 >> 1) - halo(1), (Y0 >> 1) - halo(1), a.w[1], a.h[1], x0 + i, y, &parent);
                lv[i] = lev[parent];
            }
            o[i] = lv[i] == 255u ? ST::nan() : ST::pack(r);
            if (!SRC::kField)
                wsf[a.note_off + (long long)(2 * y) * a.note_w + 2 * (x0 + i)] = level_note(lv[i]);
        }
        if (a.vec_dst && m == 4) {  // (the width even: p0 is, so both stores are aligned)
            ST::quad(a.dst, p0, o);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < m) ST::one(a.dst, p0 + i, o[i]);
        }
        if (!SRC::kField || !a.level) continue;
        if (a.vec_level) {  // (W % 4 == 0: m == 4)
            *reinterpret_cast<unsigned*>(a.level + p0) = pack4(lv);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < m) a.level[p0 + i] = (uint8_t)lv[i];
        }
    }
}

// LDS cells the top block needs for levels base .. L
long long top_cells(const FillLevels& g, int base)
{
    long long c = 0;
    for (int l = base; l <= g.L; ++l) c += (long long)g.w[l] * g.h[l];
    return c;
}

}  // namespace

hipError_t launch_flow_fill(const void* flow, int f16, const uint8_t* mask, int n, int W, int H, void* out, int out_f16,
                            uint8_t* level, void* workspace, hipStream_t s)
{
    if (fill_tile_blocks(n, W, H) < 1) return hipErrorInvalidValue;
    FillLevels g;
    fill_levels(W, H, &g);
    if (g.L > 0 && !workspace) return hipErrorInvalidValue;
    // tile passes of five levels from level 0 up, until the rest fits the top block
    int lo[kMaxFillLevels], nl[kMaxFillLevels], passes = 0, base = 0;
    do {
        lo[passes] = base;
        nl[passes] = g.L - base < kFillSpan ? g.L - base : kFillSpan;
        base += nl[passes++];
    } while (top_cells(g, base) > kFillTopCells);
    float2* const ws = static_cast<float2*>(workspace);
    const uintptr_t wa = reinterpret_cast<uintptr_t>(workspace);
    FillTileArgs ta[kMaxFillLevels];
    for (int p = 0; p < passes; ++p) {
        FillTileArgs& a = ta[p];
        a = FillTileArgs{};
        a.ws = ws;
        a.ws_field = (long long)g.cells;
        a.lo = lo[p];
        a.nl = nl[p];
        for (int k = 0; k <= nl[p]; ++k) {
            a.w[k] = g.w[lo[p] + k], a.h[k] = g.h[lo[p] + k];
            a.off[k] = (long long)g.off[lo[p] + k];
        }
        a.tx = (a.w[0] + kFillTileW - 1) / kFillTileW;
        a.ty = (a.h[0] + kFillTileH - 1) / kFillTileH;
        if (p == 0) {
            const uintptr_t fa = reinterpret_cast<uintptr_t>(flow), oa = reinterpret_cast<uintptr_t>(out);
            const uintptr_t ma = reinterpret_cast<uintptr_t>(mask), la = reinterpret_cast<uintptr_t>(level);
            a.src = flow;
            a.mask = mask;
            a.dst = out;
            a.level = level;
            a.src_field = (long long)W * H;
            a.vec_src = ((fa & 15) == 0 && (W & (f16 ? 3 : 1)) == 0) ? 1 : 0;
            a.vec_mask = (mask && (ma & 3) == 0 && (W & 3) == 0) ? 1 : 0;
            a.vec_dst = ((oa & (out_f16 ? 7 : 15)) == 0 && (W & 1) == 0) ? 1 : 0;
            a.vec_level = (level && (la & 3) == 0 && (W & 3) == 0) ? 1 : 0;
        } else {
            a.src = a.dst = ws + a.off[0];
            a.src_field = a.ws_field;
            a.note_off = (long long)g.off[lo[p] - 1];
            a.note_w = g.w[lo[p] - 1];
            // a lane's four cells in two 16-byte accesses: every row and every field begin on one
            a.vec_src = a.vec_dst = (((wa + 8 * (uintptr_t)a.off[0]) & 15) == 0 && (a.w[0] & 1) == 0 &&
                                     (n == 1 || (a.ws_field & 1) == 0)) ? 1 : 0;
        }
    }
    for (int p = 0; p < passes; ++p) {
        if (!nl[p]) continue;
        const unsigned grid = (unsigned)((long long)n * ta[p].tx * ta[p].ty);
        if (p > 0)
            hipLaunchKernelGGL((k_fill_pull<SrcCells>), dim3(grid), dim3(kFillThreads), 0, s, ta[p]);
        else if (f16)
            hipLaunchKernelGGL((k_fill_pull<SrcF16>), dim3(grid), dim3(kFillThreads), 0, s, ta[p]);
        else
            hipLaunchKernelGGL((k_fill_pull<SrcF32>), dim3(grid), dim3(kFillThreads), 0, s, ta[p]);
    }
    if (g.L > 0) {
        FillTopArgs a{};
        a.ws = ws;
        a.ws_field = (long long)g.cells;
        a.off = (long long)g.off[base];
        a.note_off = base > 1 ? (long long)g.off[base - 1] : 0;
        a.note_w = base > 1 ? g.w[base - 1] : 0;
        a.w = g.w[base], a.h = g.h[base], a.base = base;
        hipLaunchKernelGGL(k_fill_top, dim3((unsigned)n), dim3(kFillTopThreads), 0, s, a);
    }
    for (int p = passes - 1; p >= 0; --p) {
        const unsigned grid = (unsigned)((long long)n * ta[p].tx * ta[p].ty);
        if (p > 0)
            hipLaunchKernelGGL((k_fill_push<SrcCells, StoreF32>), dim3(grid), dim3(kFillThreads), 0, s, ta[p]);
        else if (f16 && out_f16)
            hipLaunchKernelGGL((k_fill_push<SrcF16, StoreF16>), dim3(grid), dim3(kFillThreads), 0, s, ta[p]);
        else if (f16)
            hipLaunchKernelGGL((k_fill_push<SrcF16, StoreF32>), dim3(grid), dim3(kFillThreads), 0, s, ta[p]);
        else if (out_f16)
            hipLaunchKernelGGL((k_fill_push<SrcF32, StoreF16>), dim3(grid), dim3(kFillThreads), 0, s, ta[p]);
        else
            hipLaunchKernelGGL((k_fill_push<SrcF32, StoreF32>), dim3(grid), dim3(kFillThreads), 0, s, ta[p]);
    }
    return hipGetLastError();
}

}  // namespace dis
