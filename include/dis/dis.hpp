// dis.hpp -- C++ host facade of the MI355X DIS engine, header-only over the
// C-ABI (include/dis_abi.h).
//
//   dis::DenseInverseSearch   calc(I0, I1, flow) for u8 frames; presets
//                             (the per-pair body of src/main.cpp:135-198);
//                             calc(I0, I1, flow_fw, flow_bw) for both directions
//   dis::flowConsistency      forward-backward consistency mask of two fields
//   dis::FlowFormat, dis::half_bits, dis::flowConvert
//                             f16 flow output (set_flow_format) and the
//                             conversion between the two formats
//   dis::FrameFormat, dis::framesToGray
//                             colour frames in (set_frame_format: BGR / RGB(A)
//                             u8 reduced to gray on the GPU) and that
//                             conversion alone
//   dis::Yuv420, dis::yuv420ToFrames, dis::framesToYuv420
//                             4:2:0 video surfaces (NV12, NV21, I420, YV12) to
//                             frames and back, in exact integer arithmetic
//   dis::Border, dis::flowWarp
//                             u8 images warped back by a flow field (f32 or f16)
//   dis::flowInterp, dis::flowInterpWorkspace
//                             the frame at time t between two u8 images
//   dis::flowCompose, dis::advectPoints
//                             pair flows chained over a video: the flow from
//                             frame 0 to frame k+1, and points followed
//   dis::temporalDenoise, dis::denoiseWeights
//                             a frame denoised from its neighbours, each warped
//                             to it by its flow and weighted by the difference
//   OpticalFlow::OpticalFlowClass
//                             drop-in for the reference constructor with the
//                             identical signature (include/optical_flow.hpp:43-54,
//                             src/optical_flow.cpp:19-91): padded host pyramids
//                             in, finest-level flow out, computed on the GPU.
//
// Errors surface as dis::Error (status + the ABI's last-error text); the
// reference had no error reporting at all (bad input was UB).
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../dis_abi.h"

namespace dis {

enum class Preset {
    ULTRAFAST = DIS_PRESET_ULTRAFAST,
    FAST = DIS_PRESET_FAST,
    MEDIUM = DIS_PRESET_MEDIUM,
    SLOW = DIS_PRESET_SLOW,
    REFERENCE = DIS_PRESET_REFERENCE,
};

// the two forms of a warm start's `init` argument (dis_init_kind)
enum class InitKind { COARSE = DIS_INIT_COARSE, FULLRES = DIS_INIT_FULLRES };

// the format of every full-resolution flow an engine writes and reads
// (dis_flow_format); an F16 flow is an array of IEEE binary16 bit patterns
enum class FlowFormat { F32 = DIS_FLOW_F32, F16 = DIS_FLOW_F16 };
using half_bits = uint16_t;

// what the frames of an engine's calc calls hold (dis_frame_format): gray
// bytes, or 3 / 4 interleaved samples per pixel that the engine reduces to gray
enum class FrameFormat {
    GRAY8 = DIS_FRAME_GRAY8,
    BGR8 = DIS_FRAME_BGR8,
    RGB8 = DIS_FRAME_RGB8,
    BGRA8 = DIS_FRAME_BGRA8,
    RGBA8 = DIS_FRAME_RGBA8,
};
inline int channels(FrameFormat f) { return f == FrameFormat::GRAY8 ? 1 : (f == FrameFormat::BGR8 || f == FrameFormat::RGB8) ? 3 : 4; }

// what flowWarp does with a target outside the frame (dis_border)
enum class Border { REPLICATE = DIS_BORDER_REPLICATE, ZERO = DIS_BORDER_ZERO };

// the parametric model dis::fitMotion fits (dis_motion_model)
enum class MotionModel {
    TRANSLATION = DIS_MOTION_TRANSLATION,
    SIMILARITY = DIS_MOTION_SIMILARITY,
    AFFINE = DIS_MOTION_AFFINE
};

class Error : public std::runtime_error {
public:
    Error(dis_status s, const std::string& what) : std::runtime_error(what), status_(s) {}
    dis_status status() const { return status_; }

private:
    dis_status status_;
};

inline void check(dis_status s)
{
    if (s != DIS_OK) throw Error(s, std::string("dis: ") + dis_last_error());
}

inline dis_params preset_params(Preset p, int width, int height)
{
    dis_params out{};
    check(dis_preset_params(static_cast<dis_preset>(p), width, height, &out));
    return out;
}

class DenseInverseSearch {
public:
    DenseInverseSearch(const dis_params& params, int width, int height, int max_batch = 1, int device = 0)
        : params_(params), width_(width), height_(height)
    {
        check(dis_create(&ctx_, &params_, width, height, max_batch, device));
    }
    DenseInverseSearch(Preset preset, int width, int height, int max_batch = 1, int device = 0)
        : DenseInverseSearch(preset_params(preset, width, height), width, height, max_batch, device)
    {
    }
    static std::unique_ptr<DenseInverseSearch> create(Preset preset, int width, int height, int max_batch = 1,
                                                      int device = 0)
    {
        return std::unique_ptr<DenseInverseSearch>(new DenseInverseSearch(preset, width, height, max_batch, device));
    }
    ~DenseInverseSearch() { dis_destroy(ctx_); }
    DenseInverseSearch(const DenseInverseSearch&) = delete;
    DenseInverseSearch& operator=(const DenseInverseSearch&) = delete;
    DenseInverseSearch(DenseInverseSearch&& o) noexcept
        : ctx_(std::exchange(o.ctx_, nullptr)), params_(o.params_), width_(o.width_), height_(o.height_),
          format_(o.format_), frame_format_(o.frame_format_)
    {
    }

    // Flow format (dis_set_flow_format), F32 by default. The float* flow
    // overloads below throw while it is F16, the half_bits* ones unless it is:
    // a buffer of the wrong element size is never handed to the engine.
    void set_flow_format(FlowFormat f)
    {
        check(dis_set_flow_format(ctx_, static_cast<int>(f)));
        format_ = f;
    }
    FlowFormat flow_format() const { return format_; }

    // Frame format (dis_set_frame_format), GRAY8 by default. With another one
    // the I0 / I1 of every calc below are W x H x channels interleaved bytes
    // (strides stay in bytes, 0 = W * channels): the same overloads carry them,
    // and the flow is bit for bit the gray engine's on framesToGray of them.
    void set_frame_format(FrameFormat f)
    {
        check(dis_set_frame_format(ctx_, static_cast<int>(f)));
        frame_format_ = f;
    }
    FrameFormat frame_format() const { return frame_format_; }

    // Host u8 frames (row stride in bytes, 0 = width) -> host W*H*2 flow (u,v).
    void calc(const uint8_t* I0, const uint8_t* I1, float* flow, size_t stride = 0)
    {
        need(FlowFormat::F32);
        check(dis_calc_u8(ctx_, I0, I1, stride, flow, DIS_MEM_HOST, nullptr));
    }
    std::vector<float> calc(const std::vector<uint8_t>& I0, const std::vector<uint8_t>& I1)
    {
        if (I0.size() != (size_t)width_ * height_ * channels(frame_format_) || I1.size() != I0.size())
            throw Error(DIS_ERR_INVALID_ARGUMENT, "dis: frame size does not match the context");
        std::vector<float> flow((size_t)width_ * height_ * 2);
        calc(I0.data(), I1.data(), flow.data());
        return flow;
    }
    // ... -> host W*H*2 f16 flow (an F16 engine)
    void calc(const uint8_t* I0, const uint8_t* I1, half_bits* flow, size_t stride = 0)
    {
        need(FlowFormat::F16);
        check(dis_calc_u8(ctx_, I0, I1, stride, as_flow(flow), DIS_MEM_HOST, nullptr));
    }
    // Device-resident frames/flow; asynchronous on `stream` (hipStream_t).
    void calc_device(const uint8_t* dI0, const uint8_t* dI1, float* dflow, void* stream = nullptr, size_t stride = 0)
    {
        need(FlowFormat::F32);
        check(dis_calc_u8(ctx_, dI0, dI1, stride, dflow, DIS_MEM_DEVICE, stream));
    }
    // (an F16 engine: dflow 4-byte aligned)
    void calc_device(const uint8_t* dI0, const uint8_t* dI1, half_bits* dflow, void* stream = nullptr,
                     size_t stride = 0)
    {
        need(FlowFormat::F16);
        check(dis_calc_u8(ctx_, dI0, dI1, stride, as_flow(dflow), DIS_MEM_DEVICE, stream));
    }
    // n pairs: frames at I0 + k*pair_stride, flows at flow + k*W*H*2.
    void calc_batch(int n, const uint8_t* I0, const uint8_t* I1, float* flow, dis_mem where = DIS_MEM_HOST,
                    void* stream = nullptr, size_t stride = 0, size_t pair_stride = 0)
    {
        need(FlowFormat::F32);
        check(dis_calc_batch_u8(ctx_, n, I0, I1, stride, pair_stride, flow, where, stream));
    }
    void calc_batch(int n, const uint8_t* I0, const uint8_t* I1, half_bits* flow, dis_mem where = DIS_MEM_HOST,
                    void* stream = nullptr, size_t stride = 0, size_t pair_stride = 0)
    {
        need(FlowFormat::F16);
        check(dis_calc_batch_u8(ctx_, n, I0, I1, stride, pair_stride, as_flow(flow), where, stream));
    }
    // Both directions in one call (dis_calc_bidir_batch_u8): flow_fw is what
    // calc(I0, I1, .) gives, flow_bw what calc(I1, I0, .) gives, bit for bit;
    // each frame's pyramid is built once.
    void calc(const uint8_t* I0, const uint8_t* I1, float* flow_fw, float* flow_bw, size_t stride = 0)
    {
        need(FlowFormat::F32);
        check(dis_calc_bidir_batch_u8(ctx_, 1, I0, I1, stride, 0, flow_fw, flow_bw, DIS_MEM_HOST, nullptr));
    }
    void calc_bidir_batch(int n, const uint8_t* I0, const uint8_t* I1, float* flow_fw, float* flow_bw,
                          dis_mem where = DIS_MEM_HOST, void* stream = nullptr, size_t stride = 0,
                          size_t pair_stride = 0)
    {
        need(FlowFormat::F32);
        check(dis_calc_bidir_batch_u8(ctx_, n, I0, I1, stride, pair_stride, flow_fw, flow_bw, where, stream));
    }
    void calc_bidir_batch(int n, const uint8_t* I0, const uint8_t* I1, half_bits* flow_fw, half_bits* flow_bw,
                          dis_mem where = DIS_MEM_HOST, void* stream = nullptr, size_t stride = 0,
                          size_t pair_stride = 0)
    {
        need(FlowFormat::F16);
        check(dis_calc_bidir_batch_u8(ctx_, n, I0, I1, stride, pair_stride, as_flow(flow_fw), as_flow(flow_bw), where,
                                      stream));
    }
    // Warm start (dis_calc_batch_init_u8): the coarsest level starts from
    // `init` -- a full-resolution W*H*2 flow such as the previous pair's result
    // (InitKind::FULLRES; it may be `flow` itself) or an init plane of
    // initPlaneSize() vectors (InitKind::COARSE). init == nullptr is the plain
    // calc. (float flows: an F32 engine; an F16 engine's warm start goes
    // through the C-ABI with its format-typed pointers.)
    void calc(const uint8_t* I0, const uint8_t* I1, float* flow, const float* init, InitKind kind, size_t stride = 0)
    {
        need(FlowFormat::F32);
        check(dis_calc_batch_init_u8(ctx_, 1, I0, I1, stride, 0, init, static_cast<int>(kind), flow, DIS_MEM_HOST,
                                     nullptr));
    }
    void calc_batch_init(int n, const uint8_t* I0, const uint8_t* I1, const float* init, InitKind kind, float* flow,
                         dis_mem where = DIS_MEM_HOST, void* stream = nullptr, size_t stride = 0,
                         size_t pair_stride = 0)
    {
        need(FlowFormat::F32);
        check(dis_calc_batch_init_u8(ctx_, n, I0, I1, stride, pair_stride, init, static_cast<int>(kind), flow, where,
                                     stream));
    }
    // (iw, ih) of one pair's init plane
    std::pair<int, int> initPlaneSize() const
    {
        int iw = 0, ih = 0;
        check(dis_init_plane_size(ctx_, &iw, &ih));
        return {iw, ih};
    }
    // the reduction alone: n full-resolution flows -> n init planes
    void flow_to_init(int n, const float* flow, float* init_planes, dis_mem where = DIS_MEM_HOST,
                      void* stream = nullptr)
    {
        need(FlowFormat::F32);
        check(dis_flow_to_init(ctx_, n, flow, init_planes, where, stream));
    }
    void set_concurrency(int streams) { check(dis_set_concurrency(ctx_, streams)); }
    // DIS_PRECISION_EXACT (default) or DIS_PRECISION_FMA (dis_abi.h)
    void set_precision(int mode) { check(dis_set_precision(ctx_, mode)); }
    void set_graphs(bool on) { check(dis_set_graphs(ctx_, on ? 1 : 0)); }
    // host-memory batches: pairs per overlapped chunk (0 = auto), ABI v8
    void set_host_pipeline(int chunk_pairs) { check(dis_set_host_pipeline(ctx_, chunk_pairs)); }

    const dis_params& params() const { return params_; }
    int width() const { return width_; }
    int height() const { return height_; }
    dis_ctx* handle() const { return ctx_; }

private:
    void need(FlowFormat f) const
    {
        if (format_ != f)
            throw Error(DIS_ERR_INVALID_ARGUMENT, f == FlowFormat::F16
                                                      ? "dis: half_bits flow on an engine whose flow format is F32"
                                                      : "dis: float flow on an engine whose flow format is F16");
    }
    // the ABI's flow parameters are format-typed float*
    static float* as_flow(half_bits* p) { return reinterpret_cast<float*>(p); }

    dis_ctx* ctx_ = nullptr;
    dis_params params_;
    int width_, height_;
    FlowFormat format_ = FlowFormat::F32;
    FrameFormat frame_format_ = FrameFormat::GRAY8;
};

// Middlebury colour coding (src/color_coding.cpp draw_optical_flow) of n
// W x H (u,v) fields into BGR u8, on the GPU.
inline void flow_color(const float* flow, int n, int width, int height, uint8_t* bgr, float maxmotion = -1.0f,
                       dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_color(flow, n, width, height, maxmotion, bgr, where, stream, device));
}

// Forward-backward consistency (dis_flow_consistency) of n W x H (u,v) fields,
// on the GPU: mask 255 where fw and the backward vector sampled at its target
// cancel within alpha1 * (|fw|^2 + |bw|^2) + alpha2; err (optional) the squared
// round-trip distance.
inline void flowConsistency(const float* fw, const float* bw, int n, int width, int height, uint8_t* mask,
                            float* err = nullptr, float alpha1 = 0.01f, float alpha2 = 0.5f,
                            dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_consistency(fw, bw, n, width, height, alpha1, alpha2, mask, err, where, stream, device));
}

// `count` flow values between the two formats (dis_flow_convert), on the GPU:
// F32 -> F16 is the engine's own narrowing (round to nearest even), F16 -> F32
// is exact. src / dst point at float or half_bits as their format says.
inline void flowConvert(const void* src, FlowFormat src_format, void* dst, FlowFormat dst_format, size_t count,
                        dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_convert(src, static_cast<int>(src_format), dst, static_cast<int>(dst_format), count, where, stream,
                           device));
}

// n W x H frames of `format` to n W x H gray images (dis_frames_to_gray_u8), on
// the GPU: gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14, alpha ignored -- what
// an engine with that frame format applies to its input; GRAY8 copies. Strides
// in bytes, 0 = tight.
inline void framesToGray(const uint8_t* src, FrameFormat format, int n, int width, int height, uint8_t* dst,
                         size_t src_stride = 0, size_t src_image_stride = 0, size_t dst_stride = 0,
                         size_t dst_image_stride = 0, dis_mem where = DIS_MEM_HOST, void* stream = nullptr,
                         int device = 0)
{
    check(dis_frames_to_gray_u8(src, src_stride, src_image_stride, static_cast<int>(format), n, width, height, dst,
                                dst_stride, dst_image_stride, where, stream, device));
}

// 4:2:0 video surfaces (dis_yuv420_to_frames_u8 / dis_frames_to_yuv420_u8): the
// matrix and the range of the conversion, and a view of n surfaces of W x H
// pixels (both even) -- where the Y plane and the Cb and Cr samples lie. The
// makers describe one buffer per layout: the Y plane with rows `stride` bytes
// apart (0 = width), then H/2 rows of Cb/Cr pairs (nv12; nv21: Cr/Cb pairs), or
// the Cb plane and the Cr plane with rows stride/2 apart (i420; yv12: Cr, then
// Cb); image k of n lies stride * H * 3/2 bytes after image k - 1. y is a gray
// frame stack as it is: calc(n, view.y, ..., view.y_stride, view.y_image_stride).
enum class YuvMatrix { BT601 = DIS_YUV_BT601, BT709 = DIS_YUV_BT709 };
enum class YuvRange { LIMITED = DIS_YUV_LIMITED, FULL = DIS_YUV_FULL };
struct Yuv420 {
    uint8_t* y;
    uint8_t* cb;
    uint8_t* cr;
    int width, height;
    size_t y_stride, y_image_stride, c_stride, c_image_stride;
    int c_step;  // 1: planar, 2: interleaved

    static Yuv420 nv12(uint8_t* p, int width, int height, size_t stride = 0)
    {
        const size_t s = stride ? stride : static_cast<size_t>(width), img = s * height * 3 / 2;
        uint8_t* const c = p ? p + s * height : nullptr;
        return {p, c, c ? c + 1 : nullptr, width, height, s, img, s, img, 2};
    }
    static Yuv420 nv21(uint8_t* p, int width, int height, size_t stride = 0)
    {
        Yuv420 v = nv12(p, width, height, stride);
        std::swap(v.cb, v.cr);
        return v;
    }
    static Yuv420 i420(uint8_t* p, int width, int height, size_t stride = 0)
    {
        const size_t s = stride ? stride : static_cast<size_t>(width), img = s * height * 3 / 2;
        uint8_t* const c = p ? p + s * height : nullptr;
        return {p, c, c ? c + (s / 2) * (height / 2) : nullptr, width, height, s, img, s / 2, img, 1};
    }
    static Yuv420 yv12(uint8_t* p, int width, int height, size_t stride = 0)
    {
        Yuv420 v = i420(p, width, height, stride);
        std::swap(v.cb, v.cr);
        return v;
    }
};

// n surfaces to n W x H frames of `format` (dst_stride in bytes, 0 = tight), on
// the GPU, by the exact integer arithmetic of dis_abi.h: nearest chroma, `alpha`
// in the fourth sample of BGRA8 / RGBA8; a GRAY8 target reads no chroma.
inline void yuv420ToFrames(const Yuv420& src, int n, uint8_t* dst, FrameFormat format,
                           YuvMatrix matrix = YuvMatrix::BT601, YuvRange range = YuvRange::LIMITED, int alpha = 255,
                           size_t dst_stride = 0, size_t dst_image_stride = 0, dis_mem where = DIS_MEM_HOST,
                           void* stream = nullptr, int device = 0)
{
    check(dis_yuv420_to_frames_u8(src.y, src.y_stride, src.y_image_stride, src.cb, src.cr, src.c_stride,
                                  src.c_image_stride, src.c_step, static_cast<int>(matrix), static_cast<int>(range), n,
                                  src.width, src.height, dst, dst_stride, dst_image_stride, static_cast<int>(format),
                                  alpha, where, stream, device));
}

// n W x H frames of `format` to n surfaces: Y per pixel, Cb and Cr from each
// 2 x 2 block's sums. With BT601 and FULL the Y plane is framesToGray's image.
inline void framesToYuv420(const uint8_t* src, FrameFormat format, int n, const Yuv420& dst,
                           YuvMatrix matrix = YuvMatrix::BT601, YuvRange range = YuvRange::LIMITED,
                           size_t src_stride = 0, size_t src_image_stride = 0, dis_mem where = DIS_MEM_HOST,
                           void* stream = nullptr, int device = 0)
{
    check(dis_frames_to_yuv420_u8(src, src_stride, src_image_stride, static_cast<int>(format),
                                  static_cast<int>(matrix), static_cast<int>(range), n, dst.width, dst.height, dst.y,
                                  dst.y_stride, dst.y_image_stride, dst.cb, dst.cr, dst.c_stride, dst.c_image_stride,
                                  dst.c_step, where, stream, device));
}

// Backward warp (dis_flow_warp_u8) of n W x H u8 images of `channels` (1, 3, 4)
// interleaved samples by n (u,v) fields, on the GPU: dst(x, y) = src sampled
// bilinearly at (x + scale*u, y + scale*v), rounded to nearest even. With the
// I0 -> I1 flow and src = I1, dst reconstructs I0. valid (optional): 255 where
// the target lies inside the frame. The half_bits overload reads an F16 flow
// as it is (no flowConvert pass).
inline void flowWarp(const uint8_t* src, int channels, const float* flow, int n, int width, int height, uint8_t* dst,
                     float scale = 1.0f, Border border = Border::REPLICATE, uint8_t* valid = nullptr,
                     size_t src_stride = 0, size_t src_image_stride = 0, dis_mem where = DIS_MEM_HOST,
                     void* stream = nullptr, int device = 0)
{
    check(dis_flow_warp_u8(src, src_stride, src_image_stride, channels, flow, DIS_FLOW_F32, n, width, height, scale,
                           static_cast<int>(border), dst, valid, where, stream, device));
}
inline void flowWarp(const uint8_t* src, int channels, const half_bits* flow, int n, int width, int height,
                     uint8_t* dst, float scale = 1.0f, Border border = Border::REPLICATE, uint8_t* valid = nullptr,
                     size_t src_stride = 0, size_t src_image_stride = 0, dis_mem where = DIS_MEM_HOST,
                     void* stream = nullptr, int device = 0)
{
    check(dis_flow_warp_u8(src, src_stride, src_image_stride, channels, flow, DIS_FLOW_F16, n, width, height, scale,
                           static_cast<int>(border), dst, valid, where, stream, device));
}

// The frame at time t in [0, 1] between n pairs of W x H u8 images
// (dis_flow_interp_u8), on the GPU: the forward flow fw (I0 -> I1) projected to
// time t, collisions resolved by photoconsistency, both frames sampled with
// the projected flow; holes filled from I1 through bw (I1 -> I0, may be null)
// or with fw's own vector. fill (optional): 0 = a projected vector, 1 = from
// bw, 2 = from fw. Device pointers need a workspace of flowInterpWorkspace(n,
// width, height) bytes, 8-byte aligned; host pointers need none. The half_bits
// overload reads F16 flows as they are.
inline size_t flowInterpWorkspace(int n, int width, int height)
{
    size_t bytes = 0;
    check(dis_flow_interp_workspace(n, width, height, &bytes));
    return bytes;
}
inline void flowInterp(const uint8_t* I0, const uint8_t* I1, int channels, const float* fw, const float* bw, int n,
                       int width, int height, float t, uint8_t* dst, uint8_t* fill = nullptr,
                       void* workspace = nullptr, size_t stride = 0, size_t image_stride = 0,
                       dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_interp_u8(I0, I1, stride, image_stride, channels, fw, bw, DIS_FLOW_F32, n, width, height, t, dst,
                             fill, workspace, where, stream, device));
}
inline void flowInterp(const uint8_t* I0, const uint8_t* I1, int channels, const half_bits* fw, const half_bits* bw,
                       int n, int width, int height, float t, uint8_t* dst, uint8_t* fill = nullptr,
                       void* workspace = nullptr, size_t stride = 0, size_t image_stride = 0,
                       dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_interp_u8(I0, I1, stride, image_stride, channels, fw, bw, DIS_FLOW_F16, n, width, height, t, dst,
                             fill, workspace, where, stream, device));
}

// Composition of n W x H (u,v) fields (dis_flow_compose), on the GPU: with a
// the flow frame 0 -> k and b the flow k -> k+1, out = a(x) + b(x + a(x)) is the
// flow 0 -> k+1; pixels whose vector, target or taps are not to be trusted get
// NaN and valid_out 0. valid_a (the previous call's valid_out), mask_b
// (flowConsistency's mask of pair k) and valid_out are optional; out may be a
// itself and valid_out valid_a itself. The half_bits overload accumulates an
// F16 engine's pair flows into an F32 field (the accumulator stays F32: F16 has
// whole-pixel steps beyond 1024 px; the C entry point takes any three formats).
inline void flowCompose(const float* a, const float* b, int n, int width, int height, float* out,
                        const uint8_t* valid_a = nullptr, const uint8_t* mask_b = nullptr, uint8_t* valid_out = nullptr,
                        dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_compose(a, DIS_FLOW_F32, b, DIS_FLOW_F32, n, width, height, valid_a, mask_b, out, DIS_FLOW_F32,
                           valid_out, where, stream, device));
}
inline void flowCompose(const float* a, const half_bits* b, int n, int width, int height, float* out,
                        const uint8_t* valid_a = nullptr, const uint8_t* mask_b = nullptr, uint8_t* valid_out = nullptr,
                        dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_compose(a, DIS_FLOW_F32, b, DIS_FLOW_F16, n, width, height, valid_a, mask_b, out, DIS_FLOW_F32,
                           valid_out, where, stream, device));
}

// Untrusted vectors of n W x H (u,v) fields filled from the trusted ones by
// push-pull (dis_flow_fill), on the GPU: a vector is trusted when it is valid
// (not NaN, |c| < 1e9) and its mask byte, if a mask is given, is not 0
// (flowConsistency's mask, flowCompose's valid_out); every other pixel gets the
// bilinear upsample of the nearest coarser level that holds trusted data, and
// level (optional) tells which: 0 = kept, l = from about 2^l pixels away, 255 =
// the field has no trusted vector (it comes back as NaN). out may be flow
// itself. Device pointers need flowFillWorkspace(n, width, height) bytes of
// workspace, 8-byte aligned; host pointers need none. The half_bits overload
// fills an F16 engine's flows into an F32 field (the C entry point takes any
// two formats).
inline size_t flowFillWorkspace(int n, int width, int height)
{
    size_t bytes = 0;
    check(dis_flow_fill_workspace(n, width, height, &bytes));
    return bytes;
}
inline void flowFill(const float* flow, int n, int width, int height, float* out, const uint8_t* mask = nullptr,
                     uint8_t* level = nullptr, void* workspace = nullptr, dis_mem where = DIS_MEM_HOST,
                     void* stream = nullptr, int device = 0)
{
    check(dis_flow_fill(flow, DIS_FLOW_F32, mask, n, width, height, out, DIS_FLOW_F32, level, workspace, where, stream,
                        device));
}
inline void flowFill(const half_bits* flow, int n, int width, int height, float* out, const uint8_t* mask = nullptr,
                     uint8_t* level = nullptr, void* workspace = nullptr, dis_mem where = DIS_MEM_HOST,
                     void* stream = nullptr, int device = 0)
{
    check(dis_flow_fill(flow, DIS_FLOW_F16, mask, n, width, height, out, DIS_FLOW_F32, level, workspace, where, stream,
                        device));
}

// The global motion of n W x H (u,v) fields (dis_flow_fit_motion), on the GPU:
// six floats per field, u = p0 + p1 x + p2 y and v = p3 + p4 x + p5 y over pixel
// indices, fitted to the trusted vectors (valid, mask byte not 0) by least
// squares and refitted `iterations` times on those within `threshold` pixels
// of the previous fit; NaN when a fit fails. info (optional): per field
// {1 fitted / 0 failed, trusted, fitted, agree}; inliers (optional): 255 where a
// trusted vector agrees with the result. Device pointers need
// fitMotionWorkspace(n, width, height) bytes of workspace, 8-byte aligned; host
// pointers need none. The half_bits overload reads an F16 engine's flows.
inline size_t fitMotionWorkspace(int n, int width, int height)
{
    size_t bytes = 0;
    check(dis_flow_fit_motion_workspace(n, width, height, &bytes));
    return bytes;
}
inline void fitMotion(const float* flow, int n, int width, int height, float* params,
                      MotionModel model = MotionModel::AFFINE, int iterations = 3, float threshold = 1.0f,
                      const uint8_t* mask = nullptr, uint32_t* info = nullptr, uint8_t* inliers = nullptr,
                      void* workspace = nullptr, dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_fit_motion(flow, DIS_FLOW_F32, mask, n, width, height, static_cast<int>(model), iterations, threshold,
                              params, info, inliers, workspace, where, stream, device));
}
inline void fitMotion(const half_bits* flow, int n, int width, int height, float* params,
                      MotionModel model = MotionModel::AFFINE, int iterations = 3, float threshold = 1.0f,
                      const uint8_t* mask = nullptr, uint32_t* info = nullptr, uint8_t* inliers = nullptr,
                      void* workspace = nullptr, dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_flow_fit_motion(flow, DIS_FLOW_F16, mask, n, width, height, static_cast<int>(model), iterations, threshold,
                              params, info, inliers, workspace, where, stream, device));
}

// The fields of n motion models (dis_motion_to_flow): what flowWarp needs for
// the stabilised frame and flowCompose for the camera path. A model with a
// parameter that is not finite gives a NaN field.
inline void motionToFlow(const float* params, int n, int width, int height, float* out, dis_mem where = DIS_MEM_HOST,
                         void* stream = nullptr, int device = 0)
{
    check(dis_motion_to_flow(params, n, width, height, out, DIS_FLOW_F32, where, stream, device));
}
inline void motionToFlow(const float* params, int n, int width, int height, half_bits* out, dis_mem where = DIS_MEM_HOST,
                         void* stream = nullptr, int device = 0)
{
    check(dis_motion_to_flow(params, n, width, height, out, DIS_FLOW_F16, where, stream, device));
}

// The corrections of a stabiliser (dis_motion_stabilize, host only): the
// n_frames - 1 pair models of a video (fitMotion's params, frame k -> k+1; may
// be null for one frame) composed into the camera path, the path smoothed by a
// Gaussian of `sigma` frames cut at `radius` frames, and per frame the six
// parameters that move it onto the smoothed path, magnified by `zoom` (1..16)
// about the frame centre: what warpMotion takes. status (optional, n_frames
// bytes): 0 where the smoothed path could not be inverted (that correction is all
// zeros); replaced (optional): the pair models that were not finite and counted
// as no motion.
inline std::vector<float> stabilizePath(const float* pair_params, int n_frames, int width, int height, int radius,
                                        float sigma, float zoom = 1.0f, uint8_t* status = nullptr,
                                        int* replaced = nullptr)
{
    std::vector<float> corrections(n_frames > 0 ? (size_t)n_frames * 6 : 6);
    check(dis_motion_stabilize(pair_params, n_frames, width, height, radius, sigma, zoom, corrections.data(), status,
                               replaced));
    return corrections;
}

// Backward warp (dis_warp_motion_u8) of n W x H u8 images of `channels` (1, 3, 4)
// interleaved samples by n motion models of six parameters, on the GPU: bit for
// bit motionToFlow followed by flowWarp at scale 1, without the field. params
// lives where `where` says. valid (optional): 255 where the target lies inside
// the frame.
inline void warpMotion(const uint8_t* src, int channels, const float* params, int n, int width, int height,
                       uint8_t* dst, Border border = Border::REPLICATE, uint8_t* valid = nullptr, size_t src_stride = 0,
                       size_t src_image_stride = 0, dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_warp_motion_u8(src, src_stride, src_image_stride, channels, params, n, width, height,
                             static_cast<int>(border), dst, valid, where, stream, device));
}

// The homography (eight-parameter) family beside the affine one above, for a
// camera that rotates: with g = p6 x + p7 y, u = (p0 + p1 x + p2 y - x g) / (1 + g)
// and v = (p3 + p4 x + p5 y - y g) / (1 + g) over pixel indices.
// fitHomography is fitMotion without a model (dis_flow_fit_homography; params:
// n * 8 floats, NaN when a fit fails; device pointers need
// fitHomographyWorkspace bytes); homographyToFlow is motionToFlow
// (dis_homography_to_flow; a pixel behind the model's horizon is NaN);
// stabilizePathHomography is stabilizePath (dis_homography_stabilize;
// (n_frames - 1) * 8 floats in, n_frames * 8 out); warpHomography is warpMotion
// (dis_warp_homography_u8; bit for bit homographyToFlow followed by flowWarp).
inline size_t fitHomographyWorkspace(int n, int width, int height)
{
    size_t bytes = 0;
    check(dis_flow_fit_homography_workspace(n, width, height, &bytes));
    return bytes;
}
inline void fitHomography(const float* flow, int n, int width, int height, float* params, int iterations = 3,
                          float threshold = 1.0f, const uint8_t* mask = nullptr, uint32_t* info = nullptr,
                          uint8_t* inliers = nullptr, void* workspace = nullptr, dis_mem where = DIS_MEM_HOST,
                          void* stream = nullptr, int device = 0)
{
    check(dis_flow_fit_homography(flow, DIS_FLOW_F32, mask, n, width, height, iterations, threshold, params, info, inliers,
                                  workspace, where, stream, device));
}
inline void fitHomography(const half_bits* flow, int n, int width, int height, float* params, int iterations = 3,
                          float threshold = 1.0f, const uint8_t* mask = nullptr, uint32_t* info = nullptr,
                          uint8_t* inliers = nullptr, void* workspace = nullptr, dis_mem where = DIS_MEM_HOST,
                          void* stream = nullptr, int device = 0)
{
    check(dis_flow_fit_homography(flow, DIS_FLOW_F16, mask, n, width, height, iterations, threshold, params, info, inliers,
                                  workspace, where, stream, device));
}
inline void homographyToFlow(const float* params, int n, int width, int height, float* out, dis_mem where = DIS_MEM_HOST,
                             void* stream = nullptr, int device = 0)
{
    check(dis_homography_to_flow(params, n, width, height, out, DIS_FLOW_F32, where, stream, device));
}
inline void homographyToFlow(const float* params, int n, int width, int height, half_bits* out,
                             dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_homography_to_flow(params, n, width, height, out, DIS_FLOW_F16, where, stream, device));
}
inline std::vector<float> stabilizePathHomography(const float* pair_params, int n_frames, int width, int height,
                                                  int radius, float sigma, float zoom = 1.0f, uint8_t* status = nullptr,
                                                  int* replaced = nullptr)
{
    std::vector<float> corrections(n_frames > 0 ? (size_t)n_frames * 8 : 8);
    check(dis_homography_stabilize(pair_params, n_frames, width, height, radius, sigma, zoom, corrections.data(), status,
                                   replaced));
    return corrections;
}
inline void warpHomography(const uint8_t* src, int channels, const float* params, int n, int width, int height,
                           uint8_t* dst, Border border = Border::REPLICATE, uint8_t* valid = nullptr,
                           size_t src_stride = 0, size_t src_image_stride = 0, dis_mem where = DIS_MEM_HOST,
                           void* stream = nullptr, int device = 0)
{
    check(dis_warp_homography_u8(src, src_stride, src_image_stride, channels, params, n, width, height,
                                 static_cast<int>(border), dst, valid, where, stream, device));
}

// Motion-compensated temporal denoising (dis_temporal_denoise_u8) of n W x H u8
// images of `channels` (1, 3, 4) interleaved samples, on the GPU: each of the
// k_neighbours (1..8) frames is warped to cur by its flow (cur -> neighbour k)
// and blended in with weights[d], d the mean absolute difference to cur over the
// pixel's 3 x 3 window. neighbours, flows and masks are host arrays of
// k_neighbours pointers (host or device pointers as `where` says); masks or any
// of its entries may be null; weights are 256 host floats in [0, 1], for
// instance denoiseWeights(1.5 * the noise's sigma). support (optional): how many
// neighbours took part at each pixel. The half_bits overload reads F16 flows.
inline std::vector<float> denoiseWeights(float sigma)
{
    std::vector<float> table(256);
    check(dis_denoise_weights(sigma, table.data()));
    return table;
}
inline void temporalDenoise(const uint8_t* cur, const uint8_t* const* neighbours, int channels, const float* const* flows,
                            int k_neighbours, int n, int width, int height, const float* weights, uint8_t* dst,
                            const uint8_t* const* masks = nullptr, uint8_t* support = nullptr, size_t stride = 0,
                            size_t image_stride = 0, dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_temporal_denoise_u8(cur, neighbours, stride, image_stride, channels,
                                  reinterpret_cast<const void* const*>(flows), DIS_FLOW_F32, masks, k_neighbours, n, width,
                                  height, weights, dst, support, where, stream, device));
}
inline void temporalDenoise(const uint8_t* cur, const uint8_t* const* neighbours, int channels,
                            const half_bits* const* flows, int k_neighbours, int n, int width, int height,
                            const float* weights, uint8_t* dst, const uint8_t* const* masks = nullptr,
                            uint8_t* support = nullptr, size_t stride = 0, size_t image_stride = 0,
                            dis_mem where = DIS_MEM_HOST, void* stream = nullptr, int device = 0)
{
    check(dis_temporal_denoise_u8(cur, neighbours, stride, image_stride, channels,
                                  reinterpret_cast<const void* const*>(flows), DIS_FLOW_F16, masks, k_neighbours, n, width,
                                  height, weights, dst, support, where, stream, device));
}

// n fields' points moved by their field (dis_flow_advect_points), on the GPU:
// `count` (x, y) float pairs per field; a point outside the frame or on an
// invalid vector stays where it is with status 0, else status 255. points_out
// may be points; status is optional. The half_bits overload reads an F16 flow.
inline void advectPoints(const float* flow, int n, int width, int height, const float* points, int count,
                         float* points_out, uint8_t* status = nullptr, dis_mem where = DIS_MEM_HOST,
                         void* stream = nullptr, int device = 0)
{
    check(dis_flow_advect_points(flow, DIS_FLOW_F32, n, width, height, points, count, points_out, status, where, stream,
                                 device));
}
inline void advectPoints(const half_bits* flow, int n, int width, int height, const float* points, int count,
                         float* points_out, uint8_t* status = nullptr, dis_mem where = DIS_MEM_HOST,
                         void* stream = nullptr, int device = 0)
{
    check(dis_flow_advect_points(flow, DIS_FLOW_F16, n, width, height, points, count, points_out, status, where, stream,
                                 device));
}

// Middlebury .flo files (src/IO_flow.cpp ReadFlowFile / SaveFlowFile).
inline void write_flo(const std::string& path, const float* data, int width, int height, int channels = 2)
{
    check(dis_write_flo(path.c_str(), data, width, height, channels));
}
inline std::vector<float> read_flo(const std::string& path, int* width, int* height, int channels = 2)
{
    check(dis_flo_info(path.c_str(), width, height));
    std::vector<float> v((size_t)*width * *height * channels);
    check(dis_read_flo(path.c_str(), v.data(), *width, *height, channels));
    return v;
}

}  // namespace dis

namespace OpticalFlow {

// Same constructor signature and semantics as the reference
// (include/optical_flow.hpp:43-54): the whole coarse-to-fine computation runs
// inside the constructor and writes `outflow` ((width>>F) x (height>>F) x 2).
// draw_grid (an OpenCV GUI debug view) is not supported.
class OpticalFlowClass {
public:
    OpticalFlowClass(float** img_first_in, float** img_first_dx_in, float** img_first_dy_in,
                     float** img_second_in, float** img_second_dx_in, float** img_second_dy_in,
                     int img_padding_in, float* outflow, int width_in, int height_in, int coarsest_scale,
                     int finest_scale, int iterations, int patch_size, float patch_overlap, bool patnorm_in,
                     bool draw_grid, int device = 0)
    {
        if (draw_grid) throw dis::Error(DIS_ERR_UNSUPPORTED, "dis: draw_grid (OpenCV GUI) is not supported");
        dis::check(dis_flow_from_pyramids(img_first_in, img_first_dx_in, img_first_dy_in, img_second_in,
                                          img_second_dx_in, img_second_dy_in, img_padding_in, outflow, width_in,
                                          height_in, coarsest_scale, finest_scale, iterations, patch_size,
                                          patch_overlap, patnorm_in ? 1 : 0, device));
    }
};

}  // namespace OpticalFlow
