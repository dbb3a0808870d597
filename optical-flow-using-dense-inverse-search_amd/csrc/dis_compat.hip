// dis_compat.hip -- the compat path of the C-ABI: dis_flow_from_pyramids,
// OpticalFlowClass(...) semantics over caller-padded host pyramids, on a
// per-device workspace of its own (no context). The kernel arguments come from
// the builders the context's launch sequence uses (dis_launch_args.h).
#include <map>
#include <mutex>

#include "dis_host.h"
#include "dis_launch_args.h"

namespace {

// Compat path workspace: one per device for the process, grown on demand.
struct CompatWs {
    std::mutex mu;  // one call at a time on this device's workspace and stream
    float *dx = nullptr, *dy = nullptr, *i1 = nullptr;
    float2 *pu = nullptr, *dense = nullptr;
    int* fb = nullptr;
    size_t planes = 0, u = 0, d = 0, nfb = 0;
    hipStream_t stream = nullptr;
    hipStream_t up = nullptr;                  // plane uploads, level by level
    hipEvent_t level_up[dis::kMaxLevels] = {};  // level l's planes are on the device
    bool reserve(size_t p, size_t nu, size_t nd, size_t nf)
    {
        if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return false;
        if (!up && hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) return false;
        for (hipEvent_t& e : level_up)
            if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
        if (p > planes) {
            hipFree(dx);
            hipFree(dy);
            hipFree(i1);
            dx = dy = i1 = nullptr;
            planes = 0;
            if (hipMalloc(&dx, sizeof(float) * p) != hipSuccess || hipMalloc(&dy, sizeof(float) * p) != hipSuccess ||
                hipMalloc(&i1, sizeof(float) * p) != hipSuccess)
                return false;
            planes = p;
        }
        if (nu > u) {
            hipFree(pu);
            pu = nullptr;
            u = 0;
            if (hipMalloc(&pu, sizeof(float2) * nu) != hipSuccess) return false;
            u = nu;
        }
        if (nd > d) {
            hipFree(dense);
            dense = nullptr;
            d = 0;
            if (hipMalloc(&dense, sizeof(float2) * nd) != hipSuccess) return false;
            d = nd;
        }
        if (nf > nfb) {
            hipFree(fb);
            fb = nullptr;
            nfb = 0;
            if (hipMalloc(&fb, sizeof(int) * nf) != hipSuccess) return false;
            nfb = nf;
        }
        return true;
    }
};
std::mutex compat_mu;  // guards the map only: calls on different devices run in parallel
CompatWs& compat_ws(int device)
{
    static std::map<int, CompatWs> ws;  // process lifetime (freed by the driver at exit); nodes never move
    std::lock_guard<std::mutex> lock(compat_mu);
    return ws[device];
}

}  // namespace

extern "C" dis_status dis_flow_from_pyramids(const float* const* img_first, const float* const* img_first_dx,
                                             const float* const* img_first_dy, const float* const* img_second,
                                             const float* const* img_second_dx, const float* const* img_second_dy,
                                             int img_padding, float* outflow, int width, int height, int coarsest,
                                             int finest, int iterations, int patch_size, float patch_overlap,
                                             int patch_normalization, int device)
{
    (void)img_first;      // the template T is never used by the reference (Q2)
    (void)img_second_dx;  // frame-2 gradients are never read (Q15)
    (void)img_second_dy;
    if (!img_first_dx || !img_first_dy || !img_second || !outflow)
        return fail(DIS_ERR_INVALID_ARGUMENT, "null pyramid or output pointer");
    dis_params p{};
    p.coarsest_scale = coarsest;
    p.finest_scale = finest;
    p.patch_size = patch_size;
    p.iterations = iterations;
    p.patch_overlap = patch_overlap;
    p.patch_normalization = patch_normalization ? 1 : 0;
    dis_status st = dis_validate_params(&p, width, height);
    if (st != DIS_OK) return st;
    if ((width % (1 << coarsest)) || (height % (1 << coarsest)))
        return fail(DIS_ERR_INVALID_ARGUMENT, "width/height must be multiples of 2^coarsest");
    if (img_padding < patch_size)
        return fail(DIS_ERR_INVALID_ARGUMENT, "img_padding must be >= patch_size");
    for (int l = finest; l <= coarsest; ++l)
        if (!img_first_dx[l] || !img_first_dy[l] || !img_second[l])
            return fail(DIS_ERR_INVALID_ARGUMENT, "null plane in pyramid");
    dis::Geometry g;
    if (!dis::make_geometry(p, width, height, &g)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad geometry");
    const dis::LaunchConsts k = dis::search_consts(g, 0);
    if (dis_status ds = dis::use_device(device)) return ds;
    // per-device workspace, grown on demand and kept for the next call (the
    // reference constructs one OpticalFlowClass per frame pair: a malloc/free
    // per call would dominate)
    size_t fb_n = dis::kMaxLevels;
    for (int l = g.F; l <= g.C; ++l) fb_n += dis::fb_list_blocks(g.lv[l]);
    CompatWs& w = compat_ws(device);
    std::lock_guard<std::mutex> lock(w.mu);
    // physically padded plane stacks
    dis::Planes P = dis::compat_planes(g, img_padding, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!w.reserve(P.plane_stride, g.u_stride, g.dense_stride, fb_n))
        return fail(DIS_ERR_OUT_OF_MEMORY, "device allocation failed");
    P = dis::compat_planes(g, img_padding, w.i1, w.dx, w.dy, w.pu, w.dense);
    hipStream_t s = w.stream;
    const bool fast = g.ps == 8;
    // The planes go up level by level, coarsest first, on a stream of their
    // own; level l's search waits only for level l's planes. A pageable upload
    // returns when it is done, so the finer (larger) levels' uploads run while
    // the coarser levels search.
    auto upload = [&](int l) {
        const size_t bytes = sizeof(float) * (size_t)(g.lv[l].W + 2 * img_padding) * (g.lv[l].H + 2 * img_padding);
        const long long off = P.plane_off[l];
        if (hipMemcpyAsync(w.dx + off, img_first_dx[l], bytes, hipMemcpyHostToDevice, w.up) != hipSuccess ||
            hipMemcpyAsync(w.dy + off, img_first_dy[l], bytes, hipMemcpyHostToDevice, w.up) != hipSuccess ||
            hipMemcpyAsync(w.i1 + off, img_second[l], bytes, hipMemcpyHostToDevice, w.up) != hipSuccess ||
            hipEventRecord(w.level_up[l], w.up) != hipSuccess || hipStreamWaitEvent(s, w.level_up[l], 0) != hipSuccess)
            return fail(DIS_ERR_DEVICE, "pyramid upload failed");
        return DIS_OK;
    };
    // (the previous call's searches have read the workspace: `up` follows `s`)
    DIS_HIP(hipEventRecord(w.level_up[g.C], s));
    DIS_HIP(hipStreamWaitEvent(w.up, w.level_up[g.C], 0));
    if (fast) DIS_HIP(hipMemsetAsync(w.fb, 0, sizeof(int) * dis::kMaxLevels, s));
    size_t fb_off = dis::kMaxLevels;
    for (int l = g.C; l >= g.F; --l) {
        const dis::LevelGeom& L = g.lv[l];
        if (dis_status us = upload(l); us != DIS_OK) return us;
        if (fast) {  // the patch_size-8 search on the caller's planes (Search8Args.gdx_plane)
            dis::Search8Args b = dis::search8_args(g, l, P, k);
            dis::set_search8_lanes(&b, dis::search8_lanes(0, (long long)L.npw * L.nph));
            b.fb_count = w.fb + l;
            b.fb_list = w.fb + fb_off;
            fb_off += dis::fb_list_blocks(L);
            if (dis::launch_search8(b, 1, s) != hipSuccess) return fail(DIS_ERR_DEVICE, "search launch failed");
            continue;
        }
        if (dis::launch_search_generic(dis::search_args(g, l, P, k), g.ps, 1, s) != hipSuccess)
            return fail(DIS_ERR_DEVICE, "search launch failed");
        if (l > g.F && dis::launch_densify(dis::densify_args(g, l, P, k), 1, s) != hipSuccess)
            return fail(DIS_ERR_DEVICE, "densify launch failed");
    }
    // the finest level's dense flow (src/patch_grid.cpp:121-182) is the output
    if (dis::launch_densify(dis::densify_args(g, g.F, P, k), 1, s) != hipSuccess)
        return fail(DIS_ERR_DEVICE, "densify launch failed");
    const dis::LevelGeom& LF = g.lv[g.F];
    if (hipMemcpyAsync(outflow, w.dense + LF.dense_off, sizeof(float2) * LF.W * LF.H, hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return fail(DIS_ERR_DEVICE, "result download failed");
    return DIS_OK;
}
