// dis_flowops.hip -- the entry points of the C-ABI that need no context. Each
// is the pure argument rules (dis_args.h) and its own value checks, all before
// the first HIP call; then the device; then the launch, staged (dis_stage.h)
// when the pointers are the host's.
#include <cmath>
#include <cstring>

#include "dis_args.h"
#include "dis_kernels.h"
#include "dis_stage.h"

namespace {

bool bad_mem(dis_mem where) { return where != DIS_MEM_HOST && where != DIS_MEM_DEVICE; }
bool bad_format(int f) { return f != DIS_FLOW_F32 && f != DIS_FLOW_F16; }
uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

}  // namespace

extern "C" {

dis_status dis_flow_color(const float* flow, int n, int width, int height, float maxmotion, uint8_t* bgr,
                          dis_mem where, void* stream, int device)
{
    if (!flow || !bgr) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_dims(n, width, height));
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t px = (size_t)width * height * n;
    const size_t ws_bytes = sizeof(unsigned int) * dis::flow_color_ws_words(n);
    if (where == DIS_MEM_DEVICE) {
        unsigned int* maxbits = nullptr;
        DIS_HIP(hipMallocAsync(reinterpret_cast<void**>(&maxbits), ws_bytes, s));
        const hipError_t e = dis::launch_flow_color(flow, n, width, height, maxmotion, bgr, maxbits, s);
        DIS_HIP(hipFreeAsync(maxbits, s));
        DIS_HIP(e);
        return DIS_OK;
    }
    dis::HostStage st(s);
    const float* dflow = st.in(flow, sizeof(float) * 2 * px);
    uint8_t* dbgr = st.out(bgr, 3 * px);
    unsigned int* maxbits = static_cast<unsigned int*>(st.scratch(ws_bytes));
    return st.finish([&] { return dis::launch_flow_color(dflow, n, width, height, maxmotion, dbgr, maxbits, s); },
                     "flow colour coding");
}

dis_status dis_flow_convert(const void* src, int src_format, void* dst, int dst_format, size_t count, dis_mem where,
                            void* stream, int device)
{
    if (!src || !dst) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    if (bad_format(src_format) || bad_format(dst_format))
        return fail(DIS_ERR_INVALID_ARGUMENT, "formats must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    const size_t ssz = src_format == DIS_FLOW_F16 ? 2 : 4, dsz = dst_format == DIS_FLOW_F16 ? 2 : 4;
    if (count > (size_t(1) << 40)) return fail(DIS_ERR_INVALID_ARGUMENT, "count too large");
    const dis::NamedRange r[2] = {{addr(src), count * ssz, "src"}, {addr(dst), count * dsz, "dst"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(r, 1, 2, &why));
    if (where == DIS_MEM_DEVICE && ((r[0].p & (ssz - 1)) || (r[1].p & (dsz - 1))))
        return fail(DIS_ERR_INVALID_ARGUMENT, "device pointers must be aligned to their element (4 / 2 bytes)");
    if (!count) return DIS_OK;
    if (where == DIS_MEM_HOST && src_format == dst_format) {  // a host copy needs no device
        std::memcpy(dst, src, r[0].bytes);
        return DIS_OK;
    }
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (where == DIS_MEM_DEVICE) {
        if (src_format == dst_format)
            DIS_HIP(hipMemcpyAsync(dst, src, r[0].bytes, hipMemcpyDeviceToDevice, s));
        else
            DIS_HIP(dis::launch_flow_convert(src, src_format, dst, count, s));
        return DIS_OK;
    }
    dis::HostStage st(s);
    const void* dsrc = st.in(src, r[0].bytes);
    void* ddst = st.out(dst, r[1].bytes);
    return st.finish([&] { return dis::launch_flow_convert(dsrc, src_format, ddst, count, s); }, "flow conversion");
}

dis_status dis_flow_consistency(const float* fw, const float* bw, int n, int width, int height, float alpha1,
                                float alpha2, uint8_t* mask, float* err, dis_mem where, void* stream, int device)
{
    if (!fw || !bw || !mask) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_dims(n, width, height, dis::kMaxExactSide));
    if (!std::isfinite(alpha1) || !std::isfinite(alpha2) || alpha1 < 0.0f || alpha2 < 0.0f)
        return fail(DIS_ERR_INVALID_ARGUMENT, "alpha1 and alpha2 must be finite and >= 0");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    // n * H rows are folded into a one-dimensional grid: its size is the only limit on n
    if (dis::flow_consistency_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large for one launch");
    if (where == DIS_MEM_DEVICE && (((addr(fw) | addr(bw)) & 7) || (addr(err) & 3)))
        return fail(DIS_ERR_INVALID_ARGUMENT, "fw and bw must be 8-byte aligned, err 4-byte aligned");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t px = (size_t)width * height * n;
    dis::HostStage st(s, where == DIS_MEM_HOST);
    const float* dfw = st.in(fw, sizeof(float) * 2 * px);
    const float* dbw = st.in(bw, sizeof(float) * 2 * px);
    uint8_t* dmask = st.out(mask, px);
    float* derr = st.out(err, sizeof(float) * px);
    return st.finish(
        [&] { return dis::launch_flow_consistency(dfw, dbw, n, width, height, alpha1, alpha2, dmask, derr, s); },
        "flow consistency check");
}

dis_status dis_flow_warp_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                            const void* flow, int flow_format, int n, int width, int height, float scale, int border,
                            uint8_t* dst, uint8_t* valid, dis_mem where, void* stream, int device)
{
    if (!src || !flow || !dst) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_dims(n, width, height, dis::kMaxExactSide));
    if (channels != 1 && channels != 3 && channels != 4) return fail(DIS_ERR_INVALID_ARGUMENT, "channels must be 1, 3 or 4");
    if (bad_format(flow_format)) return fail(DIS_ERR_INVALID_ARGUMENT, "flow_format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (border != DIS_BORDER_REPLICATE && border != DIS_BORDER_ZERO)
        return fail(DIS_ERR_INVALID_ARGUMENT, "border must be DIS_BORDER_REPLICATE or DIS_BORDER_ZERO");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    if (!std::isfinite(scale) || std::fabs(scale) > 1024.0f)
        return fail(DIS_ERR_INVALID_ARGUMENT, "scale must be finite with |scale| <= 1024");
    // n * H rows are folded into a one-dimensional grid: its size is the only limit on n
    // (it also keeps every byte count below far under 2^63)
    if (dis::flow_warp_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large for one launch");
    dis::ImageStack im;
    DIS_ARG(dis::check_image_stack(width, height, channels, n, src_stride, src_image_stride, &im));
    const size_t px = (size_t)width * height * n;
    const size_t fsz = flow_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    const dis::NamedRange r[4] = {{addr(src), im.bytes, "src"}, {addr(flow), px * fsz, "flow"},
                                  {addr(dst), px * channels, "dst"}, {addr(valid), valid ? px : 0, "valid"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(r, 2, 4, &why));
    if (where == DIS_MEM_DEVICE && (addr(flow) & (fsz - 1)))
        return fail(DIS_ERR_INVALID_ARGUMENT, "flow must be aligned to one (u,v) pair (8 bytes f32, 4 bytes f16)");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int f16 = flow_format == DIS_FLOW_F16, zero = border == DIS_BORDER_ZERO;
    // a host source is staged as it lies (rows and images keep their strides)
    dis::HostStage st(s, where == DIS_MEM_HOST);
    const uint8_t* dsrc = st.in(src, im.bytes);
    const void* dflow = st.in(flow, px * fsz);
    uint8_t* ddst = st.out(dst, px * channels);
    uint8_t* dvalid = st.out(valid, px);
    return st.finish([&] { return dis::launch_flow_warp(dsrc, im.stride, im.image_stride, channels, dflow, f16, n, width,
                                                        height, scale, zero, ddst, dvalid, s); }, "flow warp");
}

dis_status dis_denoise_weights(float sigma, float table[256])
{
    if (!table) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    if (!std::isfinite(sigma) || !(sigma > 0.0f)) return fail(DIS_ERR_INVALID_ARGUMENT, "sigma must be finite and > 0");
    const double s2 = 2.0 * (double)sigma * (double)sigma;
    for (int d = 0; d < 256; ++d) table[d] = (float)std::exp(-((double)d * d) / s2);
    return DIS_OK;
}

dis_status dis_temporal_denoise_u8(const uint8_t* cur, const uint8_t* const* neighbours, size_t stride,
                                   size_t image_stride, int channels, const void* const* flows, int flow_format,
                                   const uint8_t* const* masks, int k_neighbours, int n, int width, int height,
                                   const float* weights, uint8_t* dst, uint8_t* support, dis_mem where, void* stream,
                                   int device)
{
    if (!cur || !neighbours || !flows || !weights || !dst) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    if (bad_format(flow_format)) return fail(DIS_ERR_INVALID_ARGUMENT, "flow_format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    DIS_ARG(dis::check_denoise_sizes(k_neighbours, n, width, height, channels));  // sizes, channels, K and the grid
    dis::ImageStack im;
    DIS_ARG(dis::check_image_stack(width, height, channels, n, stride, image_stride, &im));
    for (int d = 0; d < 256; ++d)
        if (!dis::denoise_weight_ok(weights[d])) return fail(DIS_ERR_INVALID_ARGUMENT, "weights must lie in [0, 1]");
    const bool dev = where == DIS_MEM_DEVICE;
    const int K = k_neighbours;
    const size_t px = (size_t)width * height * n;
    const size_t fsz = flow_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    uintptr_t nb[dis::kDenoiseMaxNeighbours], fl[dis::kDenoiseMaxNeighbours], mk[dis::kDenoiseMaxNeighbours];
    for (int k = 0; k < K; ++k) nb[k] = addr(neighbours[k]), fl[k] = addr(flows[k]), mk[k] = masks ? addr(masks[k]) : 0;
    dis::PairMessage why;
    DIS_ARG(dis::check_denoise_buffers(addr(cur), nb, fl, masks ? mk : nullptr, K, im.bytes, px * fsz, px, addr(dst),
                                       px * channels, addr(support), dev ? fsz : 0, &why));
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // host frames are staged as they lie (rows and images keep their strides)
    dis::HostStage st(s, !dev);
    const uint8_t* dcur = st.in(cur, im.bytes);
    const uint8_t* dnb[dis::kDenoiseMaxNeighbours];
    const void* dfl[dis::kDenoiseMaxNeighbours];
    const uint8_t* dmk[dis::kDenoiseMaxNeighbours];
    for (int k = 0; k < K; ++k) {
        dnb[k] = st.in(neighbours[k], im.bytes);
        dfl[k] = st.in(flows[k], px * fsz);
        dmk[k] = st.in(masks ? masks[k] : nullptr, px);
    }
    uint8_t* ddst = st.out(dst, px * channels);
    uint8_t* dsup = st.out(support, px);
    return st.finish([&] { return dis::launch_temporal_denoise(dcur, dnb, im.stride, im.image_stride, channels, dfl,
                                                               flow_format == DIS_FLOW_F16, dmk, K, n, width, height,
                                                               weights, ddst, dsup, s); }, "temporal denoising");
}

dis_status dis_flow_compose(const void* a, int a_format, const void* b, int b_format, int n, int width, int height,
                            const uint8_t* valid_a, const uint8_t* mask_b, void* out, int out_format,
                            uint8_t* valid_out, dis_mem where, void* stream, int device)
{
    if (!a || !b || !out) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_dims(n, width, height, dis::kMaxExactSide));
    if (bad_format(a_format) || bad_format(b_format) || bad_format(out_format))
        return fail(DIS_ERR_INVALID_ARGUMENT, "formats must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    // n * H rows are folded into a one-dimensional grid: its size is the only limit on n
    // (it also keeps every byte count below far under 2^63)
    if (dis::flow_compose_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large for one launch");
    const size_t px = (size_t)width * height * n;
    const size_t asz = a_format == DIS_FLOW_F16 ? 4 : 8, bsz = b_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    const size_t osz = out_format == DIS_FLOW_F16 ? 4 : 8;
    const dis::NamedRange r[6] = {{addr(a), px * asz, "a"}, {addr(b), px * bsz, "b"},
                                  {addr(valid_a), valid_a ? px : 0, "valid_a"}, {addr(mask_b), mask_b ? px : 0, "mask_b"},
                                  {addr(out), px * osz, "out"}, {addr(valid_out), valid_out ? px : 0, "valid_out"}};
    // in place: out may be a itself when their formats are equal, valid_out may be valid_a itself
    const dis::MayAlias may[2] = {{5, 2}, {4, 0}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint_or_same(r, 4, 6, may, a_format == out_format ? 2 : 1, &why));
    if (where == DIS_MEM_DEVICE && ((addr(a) & (asz - 1)) || (addr(b) & (bsz - 1)) || (addr(out) & (osz - 1))))
        return fail(DIS_ERR_INVALID_ARGUMENT,
                    "a, b and out must be aligned to one (u,v) pair of their format (8 bytes f32, 4 bytes f16)");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dis::HostStage st(s, where == DIS_MEM_HOST);
    const void* da = st.in(a, px * asz);
    const void* db = st.in(b, px * bsz);
    const uint8_t* dva = st.in(valid_a, px);
    const uint8_t* dmb = st.in(mask_b, px);
    void* dout = st.out(out, px * osz);
    uint8_t* dvo = st.out(valid_out, px);
    return st.finish([&] { return dis::launch_flow_compose(da, a_format == DIS_FLOW_F16, db, b_format == DIS_FLOW_F16, n,
                                                           width, height, dva, dmb, dout, out_format == DIS_FLOW_F16,
                                                           dvo, s); }, "flow composition");
}

dis_status dis_flow_fill_workspace(int n, int width, int height, size_t* bytes)
{
    if (!bytes) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_fill_workspace(n, width, height, bytes));
    return DIS_OK;
}

dis_status dis_flow_fill(const void* flow, int flow_format, const uint8_t* mask, int n, int width, int height, void* out,
                         int out_format, uint8_t* level, void* workspace, dis_mem where, void* stream, int device)
{
    if (!flow || !out) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    size_t ws_bytes = 0;
    DIS_ARG(dis::check_fill_workspace(n, width, height, &ws_bytes));  // sizes and the grid limit
    if (bad_format(flow_format) || bad_format(out_format))
        return fail(DIS_ERR_INVALID_ARGUMENT, "formats must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    const bool dev = where == DIS_MEM_DEVICE;
    if (dev && ws_bytes && !workspace) return fail(DIS_ERR_INVALID_ARGUMENT, "device pointers need a workspace");
    if (dev && ws_bytes && (addr(workspace) & 7)) return fail(DIS_ERR_INVALID_ARGUMENT, "workspace must be 8-byte aligned");
    const size_t px = (size_t)width * height * n;
    const size_t fsz = flow_format == DIS_FLOW_F16 ? 4 : 8, osz = out_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    // (a null mask, a null level and a host call's workspace take no part)
    const dis::NamedRange r[5] = {{addr(flow), px * fsz, "flow"}, {addr(mask), mask ? px : 0, "mask"},
                                  {addr(out), px * osz, "out"}, {addr(level), level ? px : 0, "level"},
                                  {addr(workspace), dev ? ws_bytes : 0, "workspace"}};
    const dis::MayAlias may[1] = {{2, 0}};  // in place: out may be flow itself when their formats are equal
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint_or_same(r, 2, 5, may, flow_format == out_format ? 1 : 0, &why));
    if (dev && ((addr(flow) & (fsz - 1)) || (addr(out) & (osz - 1))))
        return fail(DIS_ERR_INVALID_ARGUMENT,
                    "flow and out must be aligned to one (u,v) pair of their format (8 bytes f32, 4 bytes f16)");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dis::HostStage st(s, !dev);
    const void* dflow = st.in(flow, px * fsz);
    const uint8_t* dmask = st.in(mask, px);
    void* dout = st.out(out, px * osz);
    uint8_t* dlevel = st.out(level, px);
    void* dws = dev ? workspace : st.scratch(ws_bytes);
    return st.finish([&] { return dis::launch_flow_fill(dflow, flow_format == DIS_FLOW_F16, dmask, n, width, height, dout,
                                                        out_format == DIS_FLOW_F16, dlevel, dws, s); }, "flow fill");
}

dis_status dis_flow_fit_motion_workspace(int n, int width, int height, size_t* bytes)
{
    if (!bytes) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_motion_workspace(n, width, height, bytes));
    return DIS_OK;
}

dis_status dis_flow_fit_motion(const void* flow, int flow_format, const uint8_t* mask, int n, int width, int height,
                               int model, int iterations, float threshold, float* params, uint32_t* info,
                               uint8_t* inliers, void* workspace, dis_mem where, void* stream, int device)
{
    if (!flow || !params) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    size_t ws_bytes = 0;
    DIS_ARG(dis::check_motion_workspace(n, width, height, &ws_bytes));  // sizes and the grid limit
    if (bad_format(flow_format)) return fail(DIS_ERR_INVALID_ARGUMENT, "flow_format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (model != DIS_MOTION_TRANSLATION && model != DIS_MOTION_SIMILARITY && model != DIS_MOTION_AFFINE)
        return fail(DIS_ERR_INVALID_ARGUMENT, "model must be a dis_motion_model");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    if (iterations < 0 || iterations > 16) return fail(DIS_ERR_INVALID_ARGUMENT, "iterations must be in [0, 16]");
    if (!std::isfinite(threshold) || threshold < 0.0f)
        return fail(DIS_ERR_INVALID_ARGUMENT, "threshold must be finite and >= 0");
    const bool dev = where == DIS_MEM_DEVICE;
    if (dev && !workspace) return fail(DIS_ERR_INVALID_ARGUMENT, "device pointers need a workspace");
    if (dev && (addr(workspace) & 7)) return fail(DIS_ERR_INVALID_ARGUMENT, "workspace must be 8-byte aligned");
    const size_t px = (size_t)width * height * n;
    const size_t fsz = flow_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    // (a null mask, info or inliers and a host call's workspace take no part)
    const dis::NamedRange r[6] = {{addr(flow), px * fsz, "flow"}, {addr(mask), mask ? px : 0, "mask"},
                                  {addr(params), sizeof(float) * 6 * n, "params"},
                                  {addr(info), info ? sizeof(uint32_t) * 4 * n : 0, "info"},
                                  {addr(inliers), inliers ? px : 0, "inliers"},
                                  {addr(workspace), dev ? ws_bytes : 0, "workspace"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(r, 2, 6, &why));
    if (dev && (addr(flow) & (fsz - 1)))
        return fail(DIS_ERR_INVALID_ARGUMENT, "flow must be aligned to one (u,v) pair (8 bytes f32, 4 bytes f16)");
    if (dev && ((addr(params) | addr(info)) & 3))
        return fail(DIS_ERR_INVALID_ARGUMENT, "params and info must be 4-byte aligned");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dis::HostStage st(s, !dev);
    const void* dflow = st.in(flow, px * fsz);
    const uint8_t* dmask = st.in(mask, px);
    float* dparams = st.out(params, sizeof(float) * 6 * n);
    uint32_t* dinfo = st.out(info, sizeof(uint32_t) * 4 * n);
    uint8_t* dinliers = st.out(inliers, px);
    void* dws = dev ? workspace : st.scratch(ws_bytes);
    return st.finish([&] { return dis::launch_fit_motion(dflow, flow_format == DIS_FLOW_F16, dmask, n, width, height, model,
                                                         iterations, threshold, dparams, dinfo, dinliers, dws, s); },
                     "motion fit");
}

dis_status dis_motion_to_flow(const float* params, int n, int width, int height, void* out, int out_format, dis_mem where,
                              void* stream, int device)
{
    if (!params || !out) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_motion_flow(n, width, height));
    if (bad_format(out_format)) return fail(DIS_ERR_INVALID_ARGUMENT, "out_format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    const size_t px = (size_t)width * height * n;
    const size_t osz = out_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    const dis::NamedRange r[2] = {{addr(params), sizeof(float) * 6 * n, "params"}, {addr(out), px * osz, "out"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(r, 1, 2, &why));
    if (where == DIS_MEM_DEVICE && ((addr(out) & (osz - 1)) || (addr(params) & 3)))
        return fail(DIS_ERR_INVALID_ARGUMENT,
                    "out must be aligned to one (u,v) pair (8 bytes f32, 4 bytes f16), params to 4 bytes");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dis::HostStage st(s, where == DIS_MEM_HOST);
    const float* dparams = st.in(params, sizeof(float) * 6 * n);
    void* dout = st.out(out, px * osz);
    return st.finish([&] { return dis::launch_motion_flow(dparams, n, width, height, dout, out_format == DIS_FLOW_F16, s); },
                     "motion field");
}

dis_status dis_warp_motion_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                              const float* params, int n, int width, int height, int border, uint8_t* dst, uint8_t* valid,
                              dis_mem where, void* stream, int device)
{
    if (!src || !params || !dst) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_warp_motion_sizes(n, width, height, channels));  // sizes, channels and the grid
    if (border != DIS_BORDER_REPLICATE && border != DIS_BORDER_ZERO)
        return fail(DIS_ERR_INVALID_ARGUMENT, "border must be DIS_BORDER_REPLICATE or DIS_BORDER_ZERO");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    dis::ImageStack im;
    DIS_ARG(dis::check_image_stack(width, height, channels, n, src_stride, src_image_stride, &im));
    const bool dev = where == DIS_MEM_DEVICE;
    const size_t px = (size_t)width * height * n;
    dis::PairMessage why;
    DIS_ARG(dis::check_warp_motion_buffers(addr(src), im.bytes, addr(params), n, addr(dst), px * channels, addr(valid), px,
                                           dev ? 4 : 0, &why));
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int zero = border == DIS_BORDER_ZERO;
    // a host source is staged as it lies (rows and images keep their strides)
    dis::HostStage st(s, !dev);
    const uint8_t* dsrc = st.in(src, im.bytes);
    const float* dparams = st.in(params, sizeof(float) * 6 * n);
    uint8_t* ddst = st.out(dst, px * channels);
    uint8_t* dvalid = st.out(valid, px);
    return st.finish([&] { return dis::launch_warp_motion(dsrc, im.stride, im.image_stride, channels, dparams, n, width,
                                                          height, zero, ddst, dvalid, s); }, "motion warp");
}

dis_status dis_flow_fit_homography_workspace(int n, int width, int height, size_t* bytes)
{
    if (!bytes) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_homography_workspace(n, width, height, bytes));
    return DIS_OK;
}

dis_status dis_flow_fit_homography(const void* flow, int flow_format, const uint8_t* mask, int n, int width, int height,
                                   int iterations, float threshold, float* params, uint32_t* info, uint8_t* inliers,
                                   void* workspace, dis_mem where, void* stream, int device)
{
    if (!flow || !params) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    size_t ws_bytes = 0;
    DIS_ARG(dis::check_homography_workspace(n, width, height, &ws_bytes));  // sizes and the grid limit
    if (bad_format(flow_format)) return fail(DIS_ERR_INVALID_ARGUMENT, "flow_format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    if (iterations < 0 || iterations > 16) return fail(DIS_ERR_INVALID_ARGUMENT, "iterations must be in [0, 16]");
    if (!std::isfinite(threshold) || threshold < 0.0f)
        return fail(DIS_ERR_INVALID_ARGUMENT, "threshold must be finite and >= 0");
    const bool dev = where == DIS_MEM_DEVICE;
    if (dev && !workspace) return fail(DIS_ERR_INVALID_ARGUMENT, "device pointers need a workspace");
    if (dev && (addr(workspace) & 7)) return fail(DIS_ERR_INVALID_ARGUMENT, "workspace must be 8-byte aligned");
    const size_t px = (size_t)width * height * n;
    const size_t fsz = flow_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    // (a null mask, info or inliers and a host call's workspace take no part)
    const dis::NamedRange r[6] = {{addr(flow), px * fsz, "flow"}, {addr(mask), mask ? px : 0, "mask"},
                                  {addr(params), sizeof(float) * 8 * n, "params"},
                                  {addr(info), info ? sizeof(uint32_t) * 4 * n : 0, "info"},
                                  {addr(inliers), inliers ? px : 0, "inliers"},
                                  {addr(workspace), dev ? ws_bytes : 0, "workspace"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(r, 2, 6, &why));
    if (dev && (addr(flow) & (fsz - 1)))
        return fail(DIS_ERR_INVALID_ARGUMENT, "flow must be aligned to one (u,v) pair (8 bytes f32, 4 bytes f16)");
    if (dev && ((addr(params) | addr(info)) & 3))
        return fail(DIS_ERR_INVALID_ARGUMENT, "params and info must be 4-byte aligned");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dis::HostStage st(s, !dev);
    const void* dflow = st.in(flow, px * fsz);
    const uint8_t* dmask = st.in(mask, px);
    float* dparams = st.out(params, sizeof(float) * 8 * n);
    uint32_t* dinfo = st.out(info, sizeof(uint32_t) * 4 * n);
    uint8_t* dinliers = st.out(inliers, px);
    void* dws = dev ? workspace : st.scratch(ws_bytes);
    return st.finish([&] { return dis::launch_fit_homography(dflow, flow_format == DIS_FLOW_F16, dmask, n, width, height,
                                                             iterations, threshold, dparams, dinfo, dinliers, dws, s); },
                     "homography fit");
}

dis_status dis_homography_to_flow(const float* params, int n, int width, int height, void* out, int out_format,
                                  dis_mem where, void* stream, int device)
{
    if (!params || !out) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_motion_flow(n, width, height));
    if (bad_format(out_format)) return fail(DIS_ERR_INVALID_ARGUMENT, "out_format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    const size_t px = (size_t)width * height * n;
    const size_t osz = out_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    const dis::NamedRange r[2] = {{addr(params), sizeof(float) * 8 * n, "params"}, {addr(out), px * osz, "out"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(r, 1, 2, &why));
    if (where == DIS_MEM_DEVICE && ((addr(out) & (osz - 1)) || (addr(params) & 3)))
        return fail(DIS_ERR_INVALID_ARGUMENT,
                    "out must be aligned to one (u,v) pair (8 bytes f32, 4 bytes f16), params to 4 bytes");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dis::HostStage st(s, where == DIS_MEM_HOST);
    const float* dparams = st.in(params, sizeof(float) * 8 * n);
    void* dout = st.out(out, px * osz);
    return st.finish([&] { return dis::launch_homography_flow(dparams, n, width, height, dout, out_format == DIS_FLOW_F16,
                                                              s); }, "homography field");
}

dis_status dis_warp_homography_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                                  const float* params, int n, int width, int height, int border, uint8_t* dst,
                                  uint8_t* valid, dis_mem where, void* stream, int device)
{
    if (!src || !params || !dst) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_warp_motion_sizes(n, width, height, channels));  // sizes, channels and the grid
    if (border != DIS_BORDER_REPLICATE && border != DIS_BORDER_ZERO)
        return fail(DIS_ERR_INVALID_ARGUMENT, "border must be DIS_BORDER_REPLICATE or DIS_BORDER_ZERO");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    dis::ImageStack im;
    DIS_ARG(dis::check_image_stack(width, height, channels, n, src_stride, src_image_stride, &im));
    const bool dev = where == DIS_MEM_DEVICE;
    const size_t px = (size_t)width * height * n;
    dis::PairMessage why;
    DIS_ARG(dis::check_warp_homography_buffers(addr(src), im.bytes, addr(params), n, addr(dst), px * channels, addr(valid),
                                               px, dev ? 4 : 0, &why));
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int zero = border == DIS_BORDER_ZERO;
    // a host source is staged as it lies (rows and images keep their strides)
    dis::HostStage st(s, !dev);
    const uint8_t* dsrc = st.in(src, im.bytes);
    const float* dparams = st.in(params, sizeof(float) * 8 * n);
    uint8_t* ddst = st.out(dst, px * channels);
    uint8_t* dvalid = st.out(valid, px);
    return st.finish([&] { return dis::launch_warp_homography(dsrc, im.stride, im.image_stride, channels, dparams, n, width,
                                                              height, zero, ddst, dvalid, s); }, "homography warp");
}

dis_status dis_flow_advect_points(const void* flow, int flow_format, int n, int width, int height, const float* points,
                                  int count, float* points_out, uint8_t* status, dis_mem where, void* stream, int device)
{
    if (!flow || !points || !points_out) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_dims(n, width, height, dis::kMaxExactSide));
    if (bad_format(flow_format)) return fail(DIS_ERR_INVALID_ARGUMENT, "flow_format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    size_t pts = 0;
    DIS_ARG(dis::check_points(n, count, &pts));
    // the field's size is bounded as dis_flow_compose's (every byte count far under 2^63), the points by their own grid
    if (dis::flow_compose_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large");
    if (dis::flow_advect_blocks(n, count) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * count too large for one launch");
    const size_t px = (size_t)width * height * n;
    const size_t fsz = flow_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    const dis::NamedRange r[4] = {{addr(flow), px * fsz, "flow"}, {addr(points), pts * 8, "points"},
                                  {addr(points_out), pts * 8, "points_out"}, {addr(status), status ? pts : 0, "status"}};
    const dis::MayAlias may[1] = {{2, 1}};  // in place: points_out may be points itself
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint_or_same(r, 2, 4, may, 1, &why));
    if (where == DIS_MEM_DEVICE && ((addr(flow) & (fsz - 1)) || ((addr(points) | addr(points_out)) & 7)))
        return fail(DIS_ERR_INVALID_ARGUMENT,
                    "flow must be aligned to one (u,v) pair (8 bytes f32, 4 bytes f16), points and points_out to 8 bytes");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dis::HostStage st(s, where == DIS_MEM_HOST);
    const void* dflow = st.in(flow, px * fsz);
    const float* dpts = st.in(points, pts * 8);
    float* dout = st.out(points_out, pts * 8);
    uint8_t* dstatus = st.out(status, pts);
    return st.finish([&] { return dis::launch_flow_advect(dflow, flow_format == DIS_FLOW_F16, n, width, height, dpts,
                                                          count, dout, dstatus, s); }, "point advection");
}

dis_status dis_frames_to_gray_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int frame_format, int n,
                                 int width, int height, uint8_t* dst, size_t dst_stride, size_t dst_image_stride,
                                 dis_mem where, void* stream, int device)
{
    if (!src || !dst) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_dims(n, width, height));
    const int channels = dis::frame_format_channels(frame_format);
    if (!channels) return fail(DIS_ERR_INVALID_ARGUMENT, "frame_format must be a dis_frame_format");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    // n * H rows are folded into a one-dimensional grid: its size is the only limit on n
    if (dis::frames_to_gray_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large for one launch");
    dis::ImageStack im, om;
    DIS_ARG(dis::check_image_stack(width, height, channels, n, src_stride, src_image_stride, &im));
    DIS_ARG(dis::check_image_stack(width, height, 1, n, dst_stride, dst_image_stride, &om));
    const dis::NamedRange r[2] = {{addr(src), im.bytes, "src"}, {addr(dst), om.bytes, "dst"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(r, 1, 2, &why));
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (where == DIS_MEM_DEVICE) {
        DIS_HIP(dis::launch_frames_to_gray(src, nullptr, im.stride, im.image_stride, frame_format, n, width, height, dst,
                                           nullptr, om.stride, om.image_stride, s));
        return DIS_OK;
    }
    // a host source is staged as it lies; the gray images are made tight on the
    // device and come down row by row, so the caller's padding keeps its bytes
    dis::HostStage st(s);
    const uint8_t* dsrc = st.in(src, im.bytes);
    const size_t tight = (size_t)width * height;
    uint8_t* dgray = static_cast<uint8_t*>(st.scratch(tight * n));
    return st.finish(
        [&] {
            hipError_t e = dis::launch_frames_to_gray(dsrc, nullptr, im.stride, im.image_stride, frame_format, n, width,
                                                      height, dgray, nullptr, (size_t)width, tight, s);
            for (int k = 0; e == hipSuccess && k < n; ++k)
                e = hipMemcpy2DAsync(dst + k * om.image_stride, om.stride, dgray + k * tight, (size_t)width,
                                     (size_t)width, (size_t)height, hipMemcpyDeviceToHost, s);
            return e;
        },
        "frame conversion");
}

dis_status dis_flow_interp_workspace(int n, int width, int height, size_t* bytes)
{
    if (!bytes) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_dims(n, width, height, dis::kMaxExactSide, dis::kMaxKeyPixels));
    if (dis::flow_interp_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large for one launch");
    *bytes = sizeof(uint64_t) * (size_t)width * height * n;
    return DIS_OK;
}

dis_status dis_flow_interp_u8(const uint8_t* I0, const uint8_t* I1, size_t stride_in, size_t image_stride_in, int channels,
                              const void* fw, const void* bw, int flow_format, int n, int width, int height, float t,
                              uint8_t* dst, uint8_t* fill, void* workspace, dis_mem where, void* stream, int device)
{
    if (!I0 || !I1 || !fw || !dst) return fail(DIS_ERR_INVALID_ARGUMENT, "null pointer");
    DIS_ARG(dis::check_dims(n, width, height, dis::kMaxExactSide, dis::kMaxKeyPixels));
    if (channels != 1 && channels != 3 && channels != 4) return fail(DIS_ERR_INVALID_ARGUMENT, "channels must be 1, 3 or 4");
    if (bad_format(flow_format)) return fail(DIS_ERR_INVALID_ARGUMENT, "flow_format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    if (bad_mem(where)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    if (!(t >= 0.0f && t <= 1.0f)) return fail(DIS_ERR_INVALID_ARGUMENT, "t must lie in [0, 1]");  // also NaN
    // the splat folds n * W * H pixels into a one-dimensional grid: its size is the only limit on n
    // (it also keeps every byte count below far under 2^63)
    if (dis::flow_interp_blocks(n, width, height) < 0)
        return fail(DIS_ERR_INVALID_ARGUMENT, "n * width * height too large for one launch");
    dis::ImageStack im;
    DIS_ARG(dis::check_image_stack(width, height, channels, n, stride_in, image_stride_in, &im));
    const bool dev = where == DIS_MEM_DEVICE;
    if (dev && !workspace) return fail(DIS_ERR_INVALID_ARGUMENT, "device pointers need a workspace");
    if (dev && (addr(workspace) & 7)) return fail(DIS_ERR_INVALID_ARGUMENT, "workspace must be 8-byte aligned");
    const size_t px = (size_t)width * height * n;
    const size_t fsz = flow_format == DIS_FLOW_F16 ? 4 : 8;  // bytes of one (u,v) pair
    // (a null bw, a null fill and a host call's workspace take no part)
    const dis::NamedRange r[7] = {{addr(I0), im.bytes, "I0"}, {addr(I1), im.bytes, "I1"}, {addr(fw), px * fsz, "fw"},
                                  {addr(bw), bw ? px * fsz : 0, "bw"}, {addr(dst), px * channels, "dst"},
                                  {addr(fill), fill ? px : 0, "fill"},
                                  {addr(workspace), dev ? px * sizeof(uint64_t) : 0, "workspace"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(r, 4, 7, &why));
    if (dev && ((addr(fw) | addr(bw)) & (fsz - 1)))
        return fail(DIS_ERR_INVALID_ARGUMENT, "fw and bw must be aligned to one (u,v) pair (8 bytes f32, 4 bytes f16)");
    if (dis_status st = dis::use_device(device)) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int f16 = flow_format == DIS_FLOW_F16;
    // host frames are staged as they lie (rows and images keep their strides)
    dis::HostStage st(s, !dev);
    const uint8_t* d0 = st.in(I0, im.bytes);
    const uint8_t* d1 = st.in(I1, im.bytes);
    const void* dfw = st.in(fw, px * fsz);
    const void* dbw = st.in(bw, px * fsz);
    uint8_t* ddst = st.out(dst, px * channels);
    uint8_t* dfill = st.out(fill, px);
    void* dws = dev ? workspace : st.scratch(px * sizeof(uint64_t));
    return st.finish([&] { return dis::launch_flow_interp(d0, d1, im.stride, im.image_stride, channels, dfw, dbw, f16, n,
                                                          width, height, t, ddst, dfill, dws, s); }, "flow interpolation");
}

}  // extern "C"
