// dis_launch_args.hip -- geometry, per-geometry constants and the kernel
// argument builders (dis_launch_args.h). Host code only, no HIP runtime call;
// a .hip file because dis_kernels.h includes the HIP headers. Compiled with
// -ffp-contract=off like everything else: make_geometry restates the
// reference's float arithmetic.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "dis_launch_args.h"

namespace dis {

bool make_geometry(const dis_params& p, int W, int H, Geometry* g)
{
    std::memset(g, 0, sizeof(*g));
    g->W = W;
    g->H = H;
    g->C = p.coarsest_scale;
    g->F = p.finest_scale;
    g->ps = p.patch_size;
    g->iters = p.iterations;
    g->norm = p.patch_normalization ? 1 : 0;
    // src/main.cpp:139-155
    const int sf = 1 << g->C;
    const int padw = (W % sf) ? sf - W % sf : 0;
    const int padh = (H % sf) ? sf - H % sf : 0;
    g->Wp = W + padw;
    g->Hp = H + padh;
    g->pad_left = padw / 2;
    g->pad_top = padh / 2;
    // src/optical_flow.cpp:38
    const int st = (int)std::floor((float)p.patch_size * (1.0f - p.patch_overlap));
    g->steps = st < 1 ? 1 : st;
    long long poff = 0, uoff = 0, doff = 0;
    for (int l = 0; l <= g->C; ++l) {
        LevelGeom& L = g->lv[l];
        const float sc = std::pow(2.0f, (float)-l);  // src/optical_flow.cpp:50-53
        L.W = (int)((float)g->Wp * sc);
        L.H = (int)((float)g->Hp * sc);
        if (L.W < 1 || L.H < 1) return false;
        L.steps = g->steps;
        // src/patch_grid.cpp:20-23
        L.npw = (int)std::ceil((float)L.W / (float)g->steps);
        L.nph = (int)std::ceil((float)L.H / (float)g->steps);
        L.offw = (L.W - (L.npw - 1) * g->steps) / 2;
        L.offh = (L.H - (L.nph - 1) * g->steps) / 2;
        L.n = L.npw * L.nph;
        // src/optical_flow.cpp:55-57
        L.tmp_lb = -(float)p.patch_size / 2;
        L.tmp_ub_w = (float)(L.W + p.patch_size / 2 - 2);
        L.tmp_ub_h = (float)(L.H + p.patch_size / 2 - 2);
        L.plane_off = poff;
        L.u_off = uoff;
        L.dense_off = doff;
        poff += (long long)L.W * L.H;
        uoff += L.n;
        doff += (long long)L.W * L.H;
    }
    g->plane_stride = (poff + 63) & ~63LL;
    g->u_stride = (uoff + 31) & ~31LL;
    g->dense_stride = (doff + 31) & ~31LL;
    return true;
}

float sqrt_threshold(float thr)
{
    float s = thr * thr;
    while (std::sqrt(s) > thr) s = std::nextafter(s, 0.0f);
    while (std::sqrt(std::nextafter(s, INFINITY)) <= thr) s = std::nextafter(s, INFINITY);
    return s;
}

int upsample_xmax(const Geometry& g)
{
    const int wF = g.lv[g.F].W;
    const double inv = 1.0 / (double)std::pow(2.0f, (float)g.F);
    for (int d = 0; d < g.Wp; ++d) {
        const float fx = (float)((d + 0.5) * inv - 0.5);
        int sx = (int)std::floor(fx);
        if (sx < 0) sx = 0;
        if (sx + 1 >= wF) return d;
    }
    return g.Wp;
}

LaunchConsts search_consts(const Geometry& g, int paper_mode)
{
    LaunchConsts k{};
    k.outlier = (float)g.ps / 2;
    k.thr_sq = sqrt_threshold(k.outlier);
    k.paper = paper_mode != 0 ? 1 : 0;
    return k;
}

LaunchConsts launch_consts(const Geometry& g, int paper_mode)
{
    LaunchConsts k = search_consts(g, paper_mode);
    k.xmax = upsample_xmax(g);
    k.sc = std::pow(2.0f, (float)g.F);
    return k;
}

int search8_lanes(int variant, long long patches)
{
    if (variant == 2) return 4;
    if (variant == 3 || variant == 9) return 2;
    if (variant == 4) return 8;
    if (variant == 5) return 1;
    if (variant == 6) return 64;  // one wave per patch (exact, non-paper levels)
    return patches <= kLpp8MaxPatches ? 8 : 2;
}

size_t fb_list_blocks(const LevelGeom& L) { return (size_t)((L.npw + 7) / 8) * ((L.nph + 7) / 8); }

bool frame_rows_aligned(const void* I0, const void* I1, size_t stride, size_t pair_stride, int n, int pad_left,
                        int bytes)
{
    return ((reinterpret_cast<uintptr_t>(I0) | reinterpret_cast<uintptr_t>(I1) | stride |
             (n > 1 ? pair_stride : 0) | (size_t)pad_left) & (size_t)(bytes - 1)) == 0;
}

bool flow_vec_store(const void* flow, int W, bool f16)
{
    return (reinterpret_cast<uintptr_t>(flow) & (f16 ? 7 : 15)) == 0 && (W & 1) == 0;
}

Planes context_planes(const Geometry& g, int p0, float* img0, float* img1, float* dx, float* dy, float2* pu,
                      float2* dense)
{
    Planes P{};
    P.img0 = img0 + (size_t)p0 * g.plane_stride;
    P.img1 = img1 + (size_t)p0 * g.plane_stride;
    P.dx = dx + (size_t)p0 * g.plane_stride;
    P.dy = dy + (size_t)p0 * g.plane_stride;
    P.pu = pu + (size_t)p0 * g.u_stride;
    P.dense = dense + (size_t)p0 * g.dense_stride;
    P.plane_stride = g.plane_stride;
    P.u_stride = g.u_stride;
    P.dense_stride = g.dense_stride;
    for (int l = 0; l <= g.C; ++l) P.plane_off[l] = g.lv[l].plane_off;
    return P;
}

Planes compat_planes(const Geometry& g, int pad, float* img1, float* dx, float* dy, float2* pu, float2* dense)
{
    Planes P{};
    P.img1 = img1;
    P.dx = dx;
    P.dy = dy;
    P.pu = pu;
    P.dense = dense;
    P.u_stride = g.u_stride;
    P.dense_stride = g.dense_stride;
    P.pad = pad;
    long long tot = 0;
    for (int l = 0; l <= g.C; ++l) {
        P.plane_off[l] = tot;
        tot += (long long)(g.lv[l].W + 2 * pad) * (g.lv[l].H + 2 * pad);
    }
    P.plane_stride = tot;
    return P;
}

PyramidArgs pyramid_args(const Geometry& g, const Planes& P, const uint8_t* I0, const uint8_t* I1, size_t stride,
                         size_t pair_stride, int n)
{
    PyramidArgs pa{};
    pa.I0 = I0;
    pa.I1 = I1;
    pa.stride = stride;
    pa.pair_stride = pair_stride;
    pa.W = g.W;
    pa.H = g.H;
    pa.Wp = g.Wp;
    pa.Hp = g.Hp;
    pa.pl = g.pad_left;
    pa.pt = g.pad_top;
    pa.img0 = P.img0;
    pa.img1 = P.img1;
    pa.plane_stride = P.plane_stride;
    pa.levels = std::min(g.C, 6);
    pa.write_l0 = g.F == 0 ? 1 : 0;
    pa.qword_ok = frame_rows_aligned(I0, I1, stride, pair_stride, n, g.pad_left, 16);
    for (int l = 0; l <= g.C; ++l) {
        pa.off[l] = P.plane_off[l];
        pa.w[l] = g.lv[l].W;
    }
    return pa;
}

SearchArgs search_args(const Geometry& g, int l, const Planes& P, const LaunchConsts& k)
{
    const LevelGeom& L = g.lv[l];
    SearchArgs a{};
    a.img0 = P.img0;
    a.img1 = P.img1;
    a.dx = P.dx;
    a.dy = P.dy;
    a.dense_coarse = (l < g.C) ? P.dense + g.lv[l + 1].dense_off : nullptr;
    a.u_out = P.pu + L.u_off;
    a.plane_stride = P.plane_stride;
    a.plane_off = P.plane_off[l];
    a.dense_stride = P.dense_stride;
    a.coarse_ld = L.W / 2;
    a.u_stride = P.u_stride;
    a.phys_pad = P.pad;
    a.W = L.W;
    a.H = L.H;
    a.steps = L.steps;
    a.npw = L.npw;
    a.nph = L.nph;
    a.offw = L.offw;
    a.offh = L.offh;
    a.n = L.n;
    a.tmp_lb = L.tmp_lb;
    a.tmp_ub_w = L.tmp_ub_w;
    a.tmp_ub_h = L.tmp_ub_h;
    a.outlier = k.outlier;
    a.iters = g.iters;
    a.norm = g.norm;
    a.paper = k.paper;
    return a;
}

Search8Args search8_args(const Geometry& g, int l, const Planes& P, const LaunchConsts& k)
{
    const LevelGeom& L = g.lv[l];
    Search8Args b{};
    b.img0 = P.img0;
    b.img1 = P.img1;
    if (P.pad) {  // the caller's padded planes: template gradients from them
        b.gdx_plane = P.dx;
        b.gdy_plane = P.dy;
        b.pad = P.pad;
    }
    b.u_coarse = (l < g.C) ? P.pu + g.lv[l + 1].u_off : nullptr;
    b.u_out = P.pu + L.u_off;
    b.plane_stride = P.plane_stride;
    b.plane_off = P.plane_off[l];
    b.u_stride = P.u_stride;
    b.W = L.W;
    b.H = L.H;
    b.steps = L.steps;
    b.npw = L.npw;
    b.nph = L.nph;
    b.offw = L.offw;
    b.offh = L.offh;
    if (l < g.C) {
        b.c_npw = g.lv[l + 1].npw;
        b.c_nph = g.lv[l + 1].nph;
        b.c_offw = g.lv[l + 1].offw;
        b.c_offh = g.lv[l + 1].offh;
    }
    b.coarse_ld = L.W / 2;
    b.tmp_lb = L.tmp_lb;
    b.tmp_ub_w = L.tmp_ub_w;
    b.tmp_ub_h = L.tmp_ub_h;
    b.thr_sq = k.thr_sq;
    b.iters = g.iters;
    b.norm = g.norm;
    b.paper = k.paper;
    return b;
}

DensifyArgs densify_args(const Geometry& g, int l, const Planes& P, const LaunchConsts& k)
{
    const LevelGeom& L = g.lv[l];
    DensifyArgs d{};
    if (!P.pad) {  // paper mode's residual weights read unpadded planes only
        d.img0 = P.img0 + P.plane_off[l];
        d.img1 = P.img1 + P.plane_off[l];
        d.plane_stride = P.plane_stride;
    }
    d.paper = k.paper;
    d.u = P.pu + L.u_off;
    d.dense = P.dense + L.dense_off;
    d.u_stride = P.u_stride;
    d.dense_stride = P.dense_stride;
    d.W = L.W;
    d.H = L.H;
    d.ps = g.ps;
    d.steps = L.steps;
    d.npw = L.npw;
    d.nph = L.nph;
    d.offw = L.offw;
    d.offh = L.offh;
    return d;
}

VarRefArgs varref_args(const Geometry& g, int l, const Planes& P)
{
    const LevelGeom& L = g.lv[l];
    VarRefArgs v{};
    v.img0 = P.img0 + P.plane_off[l];
    v.img1 = P.img1 + P.plane_off[l];
    v.plane_stride = P.plane_stride;
    v.flow = P.dense + L.dense_off;
    v.flow_stride = P.dense_stride;
    v.W = L.W;
    v.H = L.H;
    return v;
}

OutputArgs output_args(const Geometry& g, const Planes& P, const LaunchConsts& k, float2* flow, bool f16)
{
    const LevelGeom& LF = g.lv[g.F];
    OutputArgs o{};
    o.u = P.pu + LF.u_off;
    o.flow = flow;
    o.u_stride = P.u_stride;
    o.W = g.W;
    o.H = g.H;
    o.wF = LF.W;
    o.hF = LF.H;
    o.F = g.F;
    o.pad_left = g.pad_left;
    o.pad_top = g.pad_top;
    o.xmax = k.xmax;
    o.npw = LF.npw;
    o.nph = LF.nph;
    o.offw = LF.offw;
    o.offh = LF.offh;
    o.steps = LF.steps;
    o.hp = g.ps / 2;
    o.vec_store = flow_vec_store(flow, g.W, f16) ? 1 : 0;
    o.sc = k.sc;
    o.paper = k.paper;
    o.img0 = P.img0 + P.plane_off[g.F];
    o.img1 = P.img1 + P.plane_off[g.F];
    o.plane_stride = P.plane_stride;
    return o;
}

UpsampleArgs upsample_args(const Geometry& g, const Planes& P, const LaunchConsts& k, float2* flow)
{
    const LevelGeom& LF = g.lv[g.F];
    UpsampleArgs u{};
    u.dense = P.dense + LF.dense_off;
    u.flow = flow;
    u.dense_stride = P.dense_stride;
    u.W = g.W;
    u.H = g.H;
    u.wF = LF.W;
    u.hF = LF.H;
    u.F = g.F;
    u.pad_left = g.pad_left;
    u.pad_top = g.pad_top;
    u.sc = k.sc;
    u.inv_sc = 1.0 / (double)u.sc;
    u.xmax = k.xmax;
    return u;
}

}  // namespace dis
