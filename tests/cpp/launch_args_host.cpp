// launch_args_host.cpp -- the host arithmetic in front of the launches
// (csrc/dis_launch_args.hip: geometry, per-geometry constants, the kernel
// argument builders) on the CPU, compiled together with that file under
// -fsanitize=address,undefined by tests/test_init_host.py. Pointers are made
// up: nothing is dereferenced. What it checks is what the bit-exact GPU suite
// cannot see (fields that change only speed) or never looked at.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "dis_launch_args.h"

static int failures = 0;

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAIL %s:%d: %s\n", __func__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

template <class T>
static T* at(uintptr_t a)
{
    return reinterpret_cast<T*>(a);
}

static dis_params params(int C, int F, int ps, float overlap, int iters = 12)
{
    dis_params p{};
    p.coarsest_scale = C;
    p.finest_scale = F;
    p.patch_size = ps;
    p.patch_overlap = overlap;
    p.iterations = iters;
    p.patch_normalization = 1;
    return p;
}

static void sqrt_thresholds()
{
    const float want[8] = {1.00000012f, 4.00000048f, 9.0f, 16.0000019f, 25.0000019f, 36.0f, 49.0f, 64.0000076f};
    for (int ps = 2; ps <= 16; ps += 2) {
        const float thr = (float)ps / 2, s = dis::sqrt_threshold(thr);
        CHECK(sqrtf(s) <= thr);
        CHECK(sqrtf(nextafterf(s, INFINITY)) > thr);
        CHECK(s == want[ps / 2 - 1]);
    }
}

// 0 when wF == 1, Wp - 1 when F == 0, Wp - 2^(F-1) otherwise
static void xmax_closed_form()
{
    const int ks[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 33, 100, 255, 1000, 1023, 1025, 4097};
    int cases = 0;
    for (int F = 0; F <= 5; ++F)
        for (int C = F; C <= 9; ++C) {
            auto one = [&](int k) {
                const long long Wp = (long long)k << C;
                if (Wp > (1 << 20)) return;
                dis::Geometry g;
                const dis_params p = params(C, F, 8, 0.5f);
                if (!dis::make_geometry(p, (int)Wp, 1 << C, &g)) {
                    CHECK(!"make_geometry");
                    return;
                }
                CHECK(g.Wp == Wp && g.lv[F].W == (Wp >> F));
                const int wF = g.lv[F].W;
                const int want = wF == 1 ? 0 : F == 0 ? (int)Wp - 1 : (int)Wp - (1 << (F - 1));
                const int got = dis::upsample_xmax(g);
                if (got != want) {
                    std::printf("FAIL upsample_xmax F %d C %d Wp %lld: got %d, wanted %d\n", F, C, Wp, got, want);
                    ++failures;
                }
                ++cases;
            };
            for (int k : ks) one(k);
            one((1 << 20) >> C);  // Wp = 2^20
        }
    CHECK(cases > 700);
}

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

// patch counts, running offsets and rounded strides of one geometry
static void geometry_sums(const dis::Geometry& g)
{
    long long poff = 0, uoff = 0, doff = 0;
    for (int l = 0; l <= g.C; ++l) {
        const dis::LevelGeom& L = g.lv[l];
        CHECK(L.W == g.Wp >> l && L.H == g.Hp >> l);
        CHECK(L.npw == ceil_div(L.W, g.steps) && L.nph == ceil_div(L.H, g.steps));
        CHECK(L.n == ceil_div(L.W, g.steps) * ceil_div(L.H, g.steps));
        CHECK(L.steps == g.steps);
        CHECK(L.plane_off == poff && L.u_off == uoff && L.dense_off == doff);
        CHECK(dis::fb_list_blocks(L) == (size_t)ceil_div(L.npw, 8) * ceil_div(L.nph, 8));
        poff += (long long)L.W * L.H;
        uoff += L.n;
        doff += (long long)L.W * L.H;
    }
    CHECK(g.plane_stride == (poff + 63) / 64 * 64);
    CHECK(g.u_stride == (uoff + 31) / 32 * 32);
    CHECK(g.dense_stride == (doff + 31) / 32 * 32);
}

struct Bases {
    float *img0, *img1, *dx, *dy;
    float2 *pu, *dense;
};
static const Bases kB = {at<float>(0x10000000), at<float>(0x20000000), at<float>(0x30000000), at<float>(0x40000000),
                         at<float2>(0x50000000), at<float2>(0x60000000)};

// every builder at every level against planes P; `pad` 0 is the context form
static void builders(const dis::Geometry& g, const dis::Planes& P, const long long* poff, int pad)
{
    for (int paper = 0; paper <= (pad ? 0 : 1); ++paper) {
        // the compat path makes the searches' part alone: it has no output stage
        const dis::LaunchConsts k = pad ? dis::search_consts(g, paper) : dis::launch_consts(g, paper);
        CHECK(k.outlier == (float)g.ps / 2 && k.thr_sq == dis::sqrt_threshold((float)g.ps / 2) && k.paper == paper);
        if (pad)
            CHECK(k.xmax == 0 && k.sc == 0.0f);
        else
            CHECK(k.xmax == dis::upsample_xmax(g) && k.sc == (float)(1 << g.F));
        for (int l = g.F; l <= g.C; ++l) {
            const dis::LevelGeom& L = g.lv[l];
            const dis::LevelGeom* Lc = l < g.C ? &g.lv[l + 1] : nullptr;
            const dis::Search8Args b = dis::search8_args(g, l, P, k);
            CHECK(b.img0 == P.img0 && b.img1 == P.img1);
            CHECK(b.plane_stride == P.plane_stride && b.plane_off == poff[l] && b.u_stride == g.u_stride);
            CHECK(b.u_out == P.pu + L.u_off);
            CHECK(b.u_coarse == (Lc ? P.pu + Lc->u_off : nullptr));
            CHECK(b.W == L.W && b.H == L.H && b.steps == L.steps && b.npw == L.npw && b.nph == L.nph);
            CHECK(b.offw == L.offw && b.offh == L.offh);
            CHECK(b.c_npw == (Lc ? Lc->npw : 0) && b.c_nph == (Lc ? Lc->nph : 0));
            CHECK(b.c_offw == (Lc ? Lc->offw : 0) && b.c_offh == (Lc ? Lc->offh : 0));
            CHECK(b.tmp_lb == L.tmp_lb && b.tmp_ub_w == L.tmp_ub_w && b.tmp_ub_h == L.tmp_ub_h);
            CHECK(b.thr_sq == k.thr_sq && b.iters == g.iters && b.norm == g.norm && b.paper == paper);
            CHECK(b.coarse_ld == L.W / 2 && b.dense_coarse == nullptr && b.dense_stride == 0);
            CHECK(b.pad == pad && b.gdx_plane == (pad ? P.dx : nullptr) && b.gdy_plane == (pad ? P.dy : nullptr));
            // the caller's: lane layout, fallback list, variant and precision switches, paper's coarse planes
            CHECK(b.lanes_per_patch == 0 && b.tile_stride == 0 && b.quad == 0 && b.tile_cap == 0 && b.fma == 0);
            CHECK(b.fb_count == nullptr && b.fb_list == nullptr && b.c_plane_off == 0 && b.c_W == 0 && b.c_H == 0);

            const dis::SearchArgs a = dis::search_args(g, l, P, k);
            CHECK(a.img0 == P.img0 && a.img1 == P.img1 && a.dx == P.dx && a.dy == P.dy);
            CHECK(a.dense_coarse == (Lc ? P.dense + Lc->dense_off : nullptr) && a.coarse_ld == L.W / 2);
            CHECK(a.u_out == P.pu + L.u_off);
            CHECK(a.plane_stride == P.plane_stride && a.plane_off == poff[l] && a.phys_pad == pad);
            CHECK(a.dense_stride == g.dense_stride && a.u_stride == g.u_stride);
            CHECK(a.W == L.W && a.H == L.H && a.steps == L.steps && a.npw == L.npw && a.nph == L.nph);
            CHECK(a.offw == L.offw && a.offh == L.offh && a.n == L.n);
            CHECK(a.tmp_lb == L.tmp_lb && a.tmp_ub_w == L.tmp_ub_w && a.tmp_ub_h == L.tmp_ub_h);
            CHECK(a.outlier == k.outlier && a.iters == g.iters && a.norm == g.norm && a.paper == paper);

            const dis::DensifyArgs d = dis::densify_args(g, l, P, k);
            CHECK(d.u == P.pu + L.u_off && d.dense == P.dense + L.dense_off);
            CHECK(d.u_stride == g.u_stride && d.dense_stride == g.dense_stride);
            CHECK(d.W == L.W && d.H == L.H && d.ps == g.ps && d.steps == L.steps && d.npw == L.npw && d.nph == L.nph);
            CHECK(d.offw == L.offw && d.offh == L.offh && d.paper == paper);
            if (pad) {
                CHECK(d.img0 == nullptr && d.img1 == nullptr && d.plane_stride == 0);
                continue;  // the rest never runs on padded planes
            }
            CHECK(d.img0 == P.img0 + poff[l] && d.img1 == P.img1 + poff[l] && d.plane_stride == P.plane_stride);

            const dis::VarRefArgs v = dis::varref_args(g, l, P);
            CHECK(v.img0 == P.img0 + poff[l] && v.img1 == P.img1 + poff[l] && v.plane_stride == P.plane_stride);
            CHECK(v.flow == P.dense + L.dense_off && v.flow_stride == g.dense_stride && v.W == L.W && v.H == L.H);
            CHECK(v.ws == nullptr && v.ws_plane == 0 && v.ws_stride == 0 && v.iters == 0);  // the caller's
        }
        if (pad) continue;
        const dis::LevelGeom& LF = g.lv[g.F];
        float2* const flow = at<float2>(0x70000000);
        const dis::OutputArgs o = dis::output_args(g, P, k, flow, false);
        CHECK(o.u == P.pu + LF.u_off && o.flow == flow && o.u_stride == g.u_stride);
        CHECK(o.W == g.W && o.H == g.H && o.wF == LF.W && o.hF == LF.H && o.F == g.F);
        CHECK(o.pad_left == g.pad_left && o.pad_top == g.pad_top && o.xmax == k.xmax && o.sc == k.sc);
        CHECK(o.npw == LF.npw && o.nph == LF.nph && o.offw == LF.offw && o.offh == LF.offh && o.steps == LF.steps);
        CHECK(o.hp == g.ps / 2 && o.paper == paper);
        CHECK(o.img0 == P.img0 + poff[g.F] && o.img1 == P.img1 + poff[g.F] && o.plane_stride == P.plane_stride);
        const dis::UpsampleArgs u = dis::upsample_args(g, P, k, flow);
        CHECK(u.dense == P.dense + LF.dense_off && u.flow == flow && u.dense_stride == g.dense_stride);
        CHECK(u.W == g.W && u.H == g.H && u.wF == LF.W && u.hF == LF.H && u.F == g.F);
        CHECK(u.pad_left == g.pad_left && u.pad_top == g.pad_top && u.xmax == k.xmax);
        CHECK(u.sc == k.sc && u.inv_sc == 1.0 / (double)(1 << g.F));
        const uint8_t* const I0 = at<const uint8_t>(0x80000000);
        const uint8_t* const I1 = at<const uint8_t>(0x90000000);
        const dis::PyramidArgs pa = dis::pyramid_args(g, P, I0, I1, 2048, 2048 * 1100, 4);
        CHECK(pa.I0 == I0 && pa.I1 == I1 && pa.stride == 2048 && pa.pair_stride == 2048 * 1100);
        CHECK(pa.W == g.W && pa.H == g.H && pa.Wp == g.Wp && pa.Hp == g.Hp && pa.pl == g.pad_left && pa.pt == g.pad_top);
        CHECK(pa.img0 == P.img0 && pa.img1 == P.img1 && pa.plane_stride == P.plane_stride);
        CHECK(pa.levels == (g.C < 6 ? g.C : 6) && pa.write_l0 == (g.F == 0));
        CHECK(pa.zero == nullptr && pa.nzero == 0 && pa.vec_st == 0);  // the caller's, the launcher's
        for (int l = 0; l <= g.C; ++l) CHECK(pa.off[l] == poff[l] && pa.w[l] == g.lv[l].W);
    }
}

static void one_geometry(int W, int H, const dis_params& p)
{
    dis::Geometry g;
    if (!dis::make_geometry(p, W, H, &g)) {
        CHECK(!"make_geometry");
        return;
    }
    geometry_sums(g);
    // the context form: pairs 3.. of a workspace
    const int p0 = 3;
    const dis::Planes P = dis::context_planes(g, p0, kB.img0, kB.img1, kB.dx, kB.dy, kB.pu, kB.dense);
    CHECK(P.img0 == kB.img0 + p0 * g.plane_stride && P.img1 == kB.img1 + p0 * g.plane_stride);
    CHECK(P.dx == kB.dx + p0 * g.plane_stride && P.dy == kB.dy + p0 * g.plane_stride);
    CHECK(P.pu == kB.pu + p0 * g.u_stride && P.dense == kB.dense + p0 * g.dense_stride);
    CHECK(P.plane_stride == g.plane_stride && P.u_stride == g.u_stride && P.dense_stride == g.dense_stride);
    CHECK(P.pad == 0);
    long long poff[dis::kMaxLevels] = {};
    for (int l = 0; l <= g.C; ++l) poff[l] = g.lv[l].plane_off;
    builders(g, P, poff, 0);
    // the compat form: one pair, planes padded by 8 pixels on every side
    const int pad = 8;
    const dis::Planes Q = dis::compat_planes(g, pad, kB.img1, kB.dx, kB.dy, kB.pu, kB.dense);
    long long tot = 0;
    for (int l = 0; l <= g.C; ++l) {
        poff[l] = tot;
        tot += (long long)(g.lv[l].W + 2 * pad) * (g.lv[l].H + 2 * pad);
        CHECK(Q.plane_off[l] == poff[l]);
    }
    CHECK(Q.plane_stride == tot && Q.u_stride == g.u_stride && Q.dense_stride == g.dense_stride && Q.pad == pad);
    CHECK(Q.img0 == nullptr && Q.img1 == kB.img1 && Q.dx == kB.dx && Q.dy == kB.dy);
    CHECK(Q.pu == kB.pu && Q.dense == kB.dense);
    builders(g, Q, poff, pad);
}

static void geometries()
{
    dis::Geometry g;
    const dis_params medium = params(6, 1, 8, 0.625f, 25);
    CHECK(dis::make_geometry(medium, 1920, 1080, &g));
    CHECK(g.Wp == 1920 && g.Hp == 1088 && g.pad_left == 0 && g.pad_top == 4 && g.steps == 3);
    long long patches = 0;
    for (int l = g.F; l <= g.C; ++l) patches += g.lv[l].n;
    CHECK(patches == 77700);
    CHECK(g.lv[1].n == 58240);
    one_geometry(1920, 1080, medium);
    one_geometry(200, 136, params(3, 1, 8, 0.5f));
    const dis_params ragged = params(4, 0, 8, 0.75f);
    CHECK(dis::make_geometry(ragged, 161, 121, &g));
    CHECK(g.Wp == 176 && g.Hp == 128 && g.pad_left == 7 && g.pad_top == 3 && g.steps == 2);
    one_geometry(161, 121, ragged);
}

// fields that change no result, only which loads and stores a kernel uses
static void speed_only_fields()
{
    // base, stride, pair_stride, n, pad_left -> rows loadable 4 / 16 bytes at a time (16: qword_ok)
    const struct {
        uintptr_t i0, i1;
        size_t stride, pair_stride;
        int n, pad_left, dword, qword;
    } rows[] = {
        {0x1000, 0x2000, 1920, 1920 * 1080, 2, 0, 1, 1},
        {0x1000, 0x2000, 1920, 1920 * 1080, 2, 16, 1, 1},
        {0x1004, 0x2000, 1920, 1920 * 1080, 2, 0, 1, 0},   // a 4-aligned base
        {0x1000, 0x2008, 1920, 1920 * 1080, 2, 0, 1, 0},
        {0x1000, 0x2000, 1924, 1920 * 1080, 2, 0, 1, 0},   // a 4-aligned stride
        {0x1000, 0x2000, 1920, 1920 * 1080 + 4, 2, 0, 1, 0},
        {0x1000, 0x2000, 1920, 1920 * 1080, 2, 4, 1, 0},   // a 4-aligned pad_left
        {0x1001, 0x2000, 1920, 1920 * 1080, 2, 0, 0, 0},   // odd
        {0x1000, 0x2003, 1920, 1920 * 1080, 2, 0, 0, 0},
        {0x1000, 0x2000, 1921, 1920 * 1080, 2, 0, 0, 0},
        {0x1000, 0x2000, 1920, 1920 * 1080 + 1, 2, 0, 0, 0},
        {0x1000, 0x2000, 1920, 1920 * 1080, 2, 7, 0, 0},
        {0x1000, 0x2000, 1920, 1920 * 1080 + 1, 1, 0, 1, 1},  // one pair: pair_stride is never applied
        {0x1000, 0x2000, 1920, 4, 1, 0, 1, 1},
    };
    dis::Geometry g;
    for (const auto& r : rows) {
        const uint8_t* const I0 = at<const uint8_t>(r.i0);
        const uint8_t* const I1 = at<const uint8_t>(r.i1);
        CHECK(dis::frame_rows_aligned(I0, I1, r.stride, r.pair_stride, r.n, r.pad_left, 4) == (r.dword != 0));
        CHECK(dis::frame_rows_aligned(I0, I1, r.stride, r.pair_stride, r.n, r.pad_left, 16) == (r.qword != 0));
        // through the builder: a width whose padding to 2^6 gives that pad_left
        const int W = 1920 - 2 * r.pad_left - (r.pad_left == 7 ? 1 : 0);
        CHECK(dis::make_geometry(params(6, 1, 8, 0.625f), W, 1080, &g));
        CHECK(g.pad_left == r.pad_left);
        const dis::Planes P = dis::context_planes(g, 0, kB.img0, kB.img1, kB.dx, kB.dy, kB.pu, kB.dense);
        const dis::PyramidArgs pa = dis::pyramid_args(g, P, I0, I1, r.stride, r.pair_stride, r.n);
        CHECK(pa.qword_ok == r.qword);
    }
    // two pixels per store: f32 needs a 16-byte base, f16 an 8-byte one; W even
    const struct {
        uintptr_t flow;
        int W, f16, want;
    } st[] = {{0x7000, 200, 0, 1}, {0x7008, 200, 0, 0}, {0x7000, 201, 0, 0}, {0x7008, 201, 0, 0},
              {0x7008, 200, 1, 1}, {0x7004, 200, 1, 0}, {0x7008, 201, 1, 0}, {0x7004, 201, 1, 0},
              {0x7000, 200, 1, 1}};
    for (const auto& s : st) {
        CHECK(dis::flow_vec_store(at<void>(s.flow), s.W, s.f16 != 0) == (s.want != 0));
        CHECK(dis::make_geometry(params(3, 1, 8, 0.5f), s.W, 136, &g));
        const dis::Planes P = dis::context_planes(g, 0, kB.img0, kB.img1, kB.dx, kB.dy, kB.pu, kB.dense);
        const dis::LaunchConsts k = dis::launch_consts(g, 0);
        CHECK(dis::output_args(g, P, k, at<float2>(s.flow), s.f16 != 0).vec_store == s.want);
    }
    // lanes per patch: 8 up to kLpp8MaxPatches patches x pairs, 2 above; the forced variants
    CHECK(dis::kLpp8MaxPatches == 16384);
    CHECK(dis::search8_lanes(0, 16384) == 8 && dis::search8_lanes(0, 16385) == 2);
    CHECK(dis::search8_lanes(0, 1) == 8 && dis::search8_lanes(0, 58240LL * 32) == 2);
    for (long long n : {1LL, 16384LL, 16385LL}) {
        CHECK(dis::search8_lanes(2, n) == 4 && dis::search8_lanes(3, n) == 2 && dis::search8_lanes(4, n) == 8);
        CHECK(dis::search8_lanes(6, n) == 64 && dis::search8_lanes(9, n) == 2);
    }
}

int main()
{
    sqrt_thresholds();
    xmax_closed_form();
    geometries();
    speed_only_fields();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
