/*
 * dis_abi.h -- C-ABI of the MI355X-native DIS (Dense Inverse Search) optical
 * flow engine. Plain C types only: pointers, sizes, ints, floats.
 *
 * The reference (nejcgalof/Optical-Flow-using-Dense-Inverse-Search) has no
 * C-ABI or plugin interface; its hot path is reached through
 *   (R1) construct_pyramide()                       src/main.cpp:12-50
 *   (R2) OpticalFlow::OpticalFlowClass::ctor(...)   include/optical_flow.hpp:43-54,
 *                                                   src/optical_flow.cpp:19-91
 *   (R3) the pad / convert / upsample / crop glue   src/main.cpp:135-160, 191-198
 * Each entry point below names the reference interface it replaces. The C++
 * facade in include/dis/dis.hpp (DenseInverseSearch::calc and the
 * OpticalFlow::OpticalFlowClass compatibility class) is built on these.
 *
 * Threading: a dis_ctx is bound to one HIP device; calls on one context must
 * be serialised by the caller. Distinct contexts may run concurrently.
 * Errors: every call returns a dis_status; dis_last_error() returns the
 * calling thread's last error text. No C++ exception crosses this boundary.
 */
#ifndef DIS_ABI_H
#define DIS_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIS_ABI_VERSION 8

typedef enum dis_status {
    DIS_OK = 0,
    DIS_ERR_INVALID_ARGUMENT = -1, /* bad parameter / pointer / size          */
    DIS_ERR_UNSUPPORTED = -2,      /* valid request this build does not do     */
    DIS_ERR_DEVICE = -3,           /* HIP runtime error or no usable device    */
    DIS_ERR_OUT_OF_MEMORY = -4,    /* device or host allocation failed         */
    DIS_ERR_INTERNAL = -5
} dis_status;

/* Build-defined presets (the reference has none). */
typedef enum dis_preset {
    DIS_PRESET_ULTRAFAST = 0, /* ps 8, overlap 0.5   (steps 4), it 12,  F 2, C auto */
    DIS_PRESET_FAST = 1,      /* ps 8, overlap 0.5   (steps 4), it 16,  F 2, C auto */
    DIS_PRESET_MEDIUM = 2,    /* ps 8, overlap 0.625 (steps 3), it 25,  F 1, C auto */
    DIS_PRESET_SLOW = 3,      /* ps 8, overlap 0.75  (steps 2), it 128, F 0, C auto */
    DIS_PRESET_REFERENCE = 4  /* CLI defaults src/main.cpp:66-71: ps 8, 0.7, it 1000, F 0, C 3 */
} dis_preset;

typedef enum dis_mem {
    DIS_MEM_HOST = 0,  /* pointers are host memory: the call copies and synchronises */
    DIS_MEM_DEVICE = 1 /* pointers are device memory on the context's device: the call
                          is asynchronous on `stream` */
} dis_mem;

/* The reference's scalar knobs (src/optical_flow.cpp:19-31; CLI src/main.cpp:63-92). */
typedef struct dis_params {
    int coarsest_scale;      /* C: coarsest pyramid level, >= finest_scale              */
    int finest_scale;        /* F: finest level searched; output upsampled by 2^F       */
    int patch_size;          /* even, 2..16                                              */
    int iterations;          /* >= 0; each patch does iterations+1 updates (Q3)          */
    float patch_overlap;     /* [0,1); steps = max(1, floor(ps*(1-overlap))) in float    */
    int patch_normalization; /* 0/1: mean-normalise the warped patch (src/patch.cpp:264) */
    int var_refine_iters;    /* 0 = the reference (no refinement, README.md:11); > 0: fixed-point iterations of
                                variational refinement per level (parity unpinned) */
    int paper_mode;          /* 0 = the reference; 1 = the DIS paper's residual and densification (SURVEY 8f
                                row 4, not in the reference, parity unpinned): template-subtracted (and, with
                                normalisation, mean-normalised) residual instead of Q2's warped-patch-only one,
                                and votes weighted by 1/max(1, |I1(x+u) - I0(x)|) instead of Q6's plain mean */
} dis_params;

typedef struct dis_ctx dis_ctx;

/* Work/traffic figures of one frame pair (SURVEY.md 8d formula). */
typedef struct dis_workload {
    int padded_width, padded_height;
    int steps;
    long long patches;          /* sum of n_l over levels F..C                 */
    long long updates;          /* sum of n_l*(iterations+1)                    */
    double algorithmic_bytes;   /* SURVEY.md 8d "B" for one pair                */
    double search_bytes_finest; /* 16*W_F*H_F + 16*n_F: the finest search launch */
    double search_bytes_all;    /* sum over search launches (levels F..C) of
                                   16*W_l*H_l + 16*n_l (+ 8*W_{l+1}*H_{l+1} coarse read) */
    int search_launches;        /* C - F + 1 */
    long long patches_finest;   /* n_F                                          */
    double search_flops_finest; /* algorithmic f32 operations of the finest search
                                   for one pair: n_F * (16N - 3 + 6 + (it+1)(13N + 12))
                                   with normalisation, N = patch_size^2 */
} dis_workload;

int dis_abi_version(void);
const char* dis_last_error(void);
/* "product" (ABI v6; since v7 the sources have no compile-time variants,
 * so every build is the product build) */
const char* dis_build_kind(void);

/* Fill *out with the preset's knobs for a W x H input (C = auto rule). */
dis_status dis_preset_params(dis_preset preset, int width, int height, dis_params* out);

/* Validate knobs for a W x H input (what dis_create checks). */
dis_status dis_validate_params(const dis_params* params, int width, int height);

/* Work and algorithmic bytes per pair for these knobs. */
dis_status dis_workload_info(const dis_params* params, int width, int height, dis_workload* out);

/* Create a context for W x H u8 pairs on HIP device `device`, with device
 * workspace for up to max_batch pairs per call (no allocation in calc). */
dis_status dis_create(dis_ctx** out, const dis_params* params, int width, int height,
                      int max_batch, int device);
dis_status dis_destroy(dis_ctx* ctx);

/* Flow output format (added within ABI v8: purely additive, DIS_ABI_VERSION
 * unchanged; the reference writes float flows only). Context state, like
 * dis_set_precision; DIS_FLOW_F32 is the default, and with it every result is
 * bit for bit what it was. With DIS_FLOW_F16 every full-resolution flow a
 * dis_calc_* call of this context writes -- dis_calc_u8, dis_calc_batch_u8,
 * both outputs of dis_calc_bidir_batch_u8, dis_calc_batch_init_u8 -- holds
 * W*H*2 IEEE binary16 values instead of floats: (u,v) interleaved, pair stride
 * W*H*2 halves. The `float*` flow parameters keep their C type and are
 * format-typed: they point at floats or at halves as the context's format says.
 * Each stored half is the float the F32 format would have stored, converted
 * once: round to nearest, ties to even; subnormals kept; |v| >= 65520 gives
 * +-inf; NaN stays NaN. The write-out kernels narrow in their stores: no f32
 * intermediate, no extra launch. In DIS_PRECISION_EXACT the F16 output is the
 * oracle's flow narrowed, bit for bit.
 * A DIS_INIT_FULLRES init and dis_flow_to_init's flow are read in the
 * context's format too (a previous call's output, the output buffer itself
 * included, stays a valid argument): the halves are widened exactly, then
 * sanitised and reduced as floats are. DIS_INIT_COARSE planes, the context's
 * init planes, dis_flow_to_init's output, the debug dumps (DIS_STAGE_*) and
 * dis_flow_from_pyramids stay f32. dis_flow_color and dis_flow_consistency
 * take f32 fields only: dis_flow_convert is how f16 flows reach them.
 * dis_flow_warp_u8 reads f16 flows directly (its flow_format argument).
 * Alignment of DIS_MEM_DEVICE flow pointers in DIS_FLOW_F16: 4 bytes (one
 * (u,v) pair), else DIS_ERR_INVALID_ARGUMENT; a pointer that is 8-byte aligned
 * (and an even W) gets 8-byte stores of two pixels, any other one 4-byte store
 * per pixel. The host pipeline's chunks and device slots, the graph cache key
 * and every overlap check follow the format; changing it rebuilds the host
 * pipeline on the next host call. Other values of `format` are refused with
 * DIS_ERR_INVALID_ARGUMENT. */
typedef enum dis_flow_format { DIS_FLOW_F32 = 0, DIS_FLOW_F16 = 1 } dis_flow_format;
dis_status dis_set_flow_format(dis_ctx* ctx, int format);

/* `count` flow values from src_format to dst_format (dis_flow_format each; no
 * context, like dis_flow_color; added within ABI v8). f32 -> f16 is the
 * conversion described above (the very device function the engine's writers
 * use), f16 -> f32 is exact, equal formats copy. src and dst must not overlap.
 * Host pointers: synchronous (staged through HIP device `device`). Device
 * pointers: asynchronous on `stream`; aligned to their element (4 / 2 bytes),
 * vectorised when the two buffers are equally offset from 16- / 8-byte
 * boundaries. */
dis_status dis_flow_convert(const void* src, int src_format, void* dst, int dst_format, size_t count,
                            dis_mem where, void* stream, int device);

/* Frame input format (added within ABI v8: purely additive, DIS_ABI_VERSION
 * unchanged; the reference reads gray frames only, cv::imread(..., GRAYSCALE),
 * src/main.cpp:115-116). Context state, like dis_set_flow_format;
 * DIS_FRAME_GRAY8 is the default, and with it every result, launch and code
 * path is what it was. With another format the I0 / I1 of every dis_calc_* call
 * of this context -- dis_calc_u8, dis_calc_batch_u8, dis_calc_bidir_batch_u8,
 * dis_calc_batch_init_u8, with both dis_mem values -- are W x H pixels of 3
 * (BGR8, RGB8) or 4 (BGRA8, RGBA8) interleaved u8 samples in the named order.
 * `stride` and `pair_stride` stay in bytes: 0 means W * channels and stride * H.
 * The `const uint8_t*` frame parameters keep their C type and are format-typed.
 * The engine reduces the frames to gray on the device,
 *   gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14      (alpha ignored),
 * in integer arithmetic: OpenCV's fixed-point Rec.601 (what imread's GRAYSCALE
 * applies to 8-bit colour, and what the CLI's PNG reader applies on the host).
 * The coefficients sum to 2^14, so R = G = B = v gives v; nothing is rounded.
 * The flow is bit for bit what the same context gives in DIS_FRAME_GRAY8 on the
 * frames so reduced. The front stage of a call runs one more launch per
 * sub-batch, on the sub-batch's stream, into a gray buffer of the context
 * (max_batch pairs x 2 frames, rows of W rounded up to 16 bytes), which the
 * unchanged pyramid kernels then read; a bidirectional call converts once.
 * The buffer is allocated by dis_set_frame_format on the first colour format,
 * never inside a calc call (DIS_ERR_OUT_OF_MEMORY if that fails: the format is
 * then unchanged), kept when the format goes back to gray, and freed by
 * dis_destroy. Every argument check follows the format: the frames' byte
 * extents, and with them every overlap rule (flow against frames, init against
 * frames), are computed with the pixel size. The graph cache key holds the
 * format and the luma launch is part of the captured call; the host pipeline's
 * slots and the staging of host bidirectional / warm-started calls take the
 * colour frames as they are (the conversion runs on the device; changing the
 * format rebuilds the host pipeline on the next host call). Frame pointers need
 * no alignment; a base and strides that are multiples of 16 get 16-byte loads.
 * dis_kernel_time class 7 times the luma launches. The debug dumps and
 * dis_flow_from_pyramids are unaffected (DIS_STAGE_IMG0 / IMG1 level 0 is the
 * gray frame as a float plane, as ever). Other values of `format` are refused
 * with DIS_ERR_INVALID_ARGUMENT. */
typedef enum dis_frame_format { DIS_FRAME_GRAY8 = 0, DIS_FRAME_BGR8 = 1, DIS_FRAME_RGB8 = 2,
                                DIS_FRAME_BGRA8 = 3, DIS_FRAME_RGBA8 = 4 } dis_frame_format;
dis_status dis_set_frame_format(dis_ctx* ctx, int format);

/* The conversion alone (no context, like dis_flow_convert and dis_flow_warp_u8;
 * added within ABI v8): n W x H images of `frame_format` to n W x H gray images
 * by the formula above; DIS_FRAME_GRAY8 is a strided copy. Strides in bytes, 0 =
 * tight (src: W * channels and stride * H; dst: W and stride * H), else at
 * least that, dis_flow_warp_u8's conventions. Only the W bytes of a destination
 * row are written, and no byte after a source row's last sample is read: the
 * padding of either buffer is never touched, and what follows the last row's
 * last sample is not part of the buffer. Refused with DIS_ERR_INVALID_ARGUMENT,
 * before any device call: a null src or dst; n, width or height < 1; an unknown
 * frame_format or where; strides smaller than a row / image; any overlap of dst
 * with src; more work than one launch's grid holds. No pointer needs any
 * alignment (a source whose base and strides are multiples of 16 is read with
 * 16-byte loads, such a destination written with 16-byte stores; same bytes).
 * Host pointers: synchronous, staged through HIP device `device`; device
 * pointers: asynchronous on `stream`, one launch. */
dis_status dis_frames_to_gray_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int frame_format,
                                 int n, int width, int height,
                                 uint8_t* dst, size_t dst_stride, size_t dst_image_stride,
                                 dis_mem where, void* stream, int device);

/* 4:2:0 video surfaces in and out (no context; added within ABI v8: purely
 * additive): n surfaces of W x H pixels, W and H even -- a Y plane of W x H
 * bytes and one Cb and one Cr sample per 2 x 2 block -- to n W x H frames of
 * `frame_format` (any dis_frame_format; the enum itself does not grow), and
 * back. What a video decoder delivers and an encoder takes: the Y plane is
 * already a gray frame with a row stride and an image stride, which
 * dis_calc_batch_u8 takes as it lies; these two calls are the colour side.
 *
 * Layout. Pixel (x, y) of image i has its luma at y_ptr + i*y_image_stride +
 * y*y_stride + x; the chroma of block (X, Y) is at cb + i*c_image_stride +
 * Y*c_stride + X*c_step, and at cr likewise. c_step is 1 for planar layouts and
 * 2 for interleaved ones. NV12 in one buffer: cb = y + y_stride*H, cr = cb + 1,
 * c_step = 2, c_stride = y_stride, both image strides y_stride*H*3/2; NV21 swaps
 * cb and cr; I420 and YV12 are the planar forms (c_step = 1, the Cb plane first,
 * or the Cr plane). Strides in bytes; 0 means W and y_stride*H for the Y plane,
 * (W/2)*c_step and c_stride*(H/2) for the chroma planes, and W*channels and
 * stride*H for the frames; otherwise at least that.
 *
 * Arithmetic: integers only, signed 32 bits, >> the arithmetic (floor) shift,
 * clamp to 0..255. One row per (matrix, range):
 *                 yoff    yy     rv     gu      gv     bu
 *   601 full         0  16384  22970  -5638  -11700  29032
 *   601 limited     16  19077  26149  -6419  -13320  33050
 *   709 full         0  16384  25802  -3069   -7670  30402
 *   709 limited     16  19077  29372  -3494   -8731  34610
 *                 Y <- (R,G,B)        Cb <- (R,G,B)         Cr <- (R,G,B)
 *   601 full      4899  9617 1868    -2765 -5427 8192     8192 -6860 -1332
 *   601 limited   4207  8260 1604    -2428 -4768 7196     7196 -6026 -1170
 *   709 full      3483 11718 1183    -1877 -6315 8192     8192 -7441  -751
 *   709 limited   2991 10064 1016    -1649 -5547 7196     7196 -6536  -660
 * (the standards' coefficients times 2^14, rounded to nearest, green adjusted so
 * that a Y row sums to 16384 or 14071 and a chroma row to 0).
 * To frames: pixel (x, y) takes Y(x, y) and the chroma of block (x>>1, y>>1)
 * (nearest chroma); c = yy*(Y - yoff) + 8192, u = Cb - 128, v = Cr - 128,
 *   R = clamp((c + rv*v) >> 14), G = clamp((c + gu*u + gv*v) >> 14), B = clamp((c + bu*u) >> 14);
 * DIS_FRAME_GRAY8 is clamp(c >> 14): chroma is not read, cb and cr may be NULL.
 * `alpha` (0..255) fills the fourth sample of BGRA8 / RGBA8 and is ignored
 * otherwise. From frames: Y = yoff + ((ky.(R,G,B) + 8192) >> 14) per pixel; per
 * block, with (sR, sG, sB) the sums of its four pixels,
 *   Cb = clamp((kcb.(sR,sG,sB) + (128 << 16) + (1 << 15)) >> 16), Cr likewise
 * (one rounding for the average and the conversion); alpha is ignored, and
 * DIS_FRAME_GRAY8 is R = G = B = v. Gray gives Cb = Cr = 128 exactly; with 601
 * full, Y is dis_frames_to_gray_u8's byte.
 *
 * Refused with DIS_ERR_INVALID_ARGUMENT, before any device call: a null
 * pointer (except cb / cr with a GRAY8 target); n, width or height < 1, an odd
 * width or height, a width or height above 2^24; an unknown frame_format,
 * matrix, range or where; c_step other than 1 or 2; alpha outside 0..255;
 * strides smaller than a row / an image; any overlap of an output plane with
 * an input or with another output plane (plane by plane and image by image when
 * the planes share one image stride, as those of one buffer do; cb and cr one
 * byte apart with c_step 2 are one plane); more work than one launch's grid
 * holds. No pointer needs any alignment: each of the three sides (Y, chroma,
 * frames) moves in 16-byte groups when its bases and strides are multiples of
 * 16 (planar chroma: in 8-byte groups, multiples of 8), byte by byte otherwise;
 * same bytes. Only samples are read and written: no padding byte of any plane
 * is touched. Host pointers: synchronous, staged through HIP device `device`;
 * device pointers: asynchronous on `stream`, one launch, no allocation. */
typedef enum dis_yuv_matrix { DIS_YUV_BT601 = 0, DIS_YUV_BT709 = 1 } dis_yuv_matrix;
typedef enum dis_yuv_range { DIS_YUV_LIMITED = 0, DIS_YUV_FULL = 1 } dis_yuv_range;
dis_status dis_yuv420_to_frames_u8(const uint8_t* y, size_t y_stride, size_t y_image_stride,
                                   const uint8_t* cb, const uint8_t* cr, size_t c_stride, size_t c_image_stride,
                                   int c_step, int matrix, int range, int n, int width, int height,
                                   uint8_t* dst, size_t dst_stride, size_t dst_image_stride, int frame_format,
                                   int alpha, dis_mem where, void* stream, int device);
dis_status dis_frames_to_yuv420_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int frame_format,
                                   int matrix, int range, int n, int width, int height,
                                   uint8_t* y, size_t y_stride, size_t y_image_stride,
                                   uint8_t* cb, uint8_t* cr, size_t c_stride, size_t c_image_stride, int c_step,
                                   dis_mem where, void* stream, int device);

/* One pair: u8 grayscale frames (row stride `stride` bytes, 0 = width; colour
 * frames under dis_set_frame_format, 0 = width * channels) to a
 * full-resolution W x H x 2 flow, (u,v) interleaved, row-major: floats, or
 * halves under DIS_FLOW_F16 (`flow` is format-typed, dis_set_flow_format).
 * Replaces R3 + R1 + R2 for one pair (src/main.cpp:135-198). */
dis_status dis_calc_u8(dis_ctx* ctx, const uint8_t* I0, const uint8_t* I1, size_t stride,
                       float* flow, dis_mem where, void* stream);

/* n pairs in one call: pair k's frames at I0 + k*pair_stride (bytes), its
 * flow at k*W*H*2 values (floats, or halves under DIS_FLOW_F16) after `flow`,
 * which is format-typed. n <= max_batch. */
dis_status dis_calc_batch_u8(dis_ctx* ctx, int n, const uint8_t* I0, const uint8_t* I1,
                             size_t stride, size_t pair_stride, float* flow,
                             dis_mem where, void* stream);

/* Both directions of n pairs in one call (added within ABI v8: purely
 * additive, DIS_ABI_VERSION unchanged, no v8 caller breaks): flow_fw[k] is
 * what dis_calc_batch_u8(I0, I1) gives for pair k, flow_bw[k] what
 * dis_calc_batch_u8(I1, I0) gives -- bit for bit in DIS_PRECISION_EXACT, and
 * bit for bit in DIS_PRECISION_FMA for the same n and concurrency. Each frame
 * is read and its pyramid built once; the backward pass is the same level loop
 * with the two frames' planes swapped. The two outputs (format-typed:
 * n*W*H*2 floats, or halves under DIS_FLOW_F16) must not overlap. Always enqueued eagerly (never a replayed graph). DIS_MEM_HOST is
 * synchronous and stages through device buffers for max_batch pairs that the
 * context allocates on the first such call (DIS_ERR_OUT_OF_MEMORY if that
 * fails); the chunked host pipeline below is not used. After this call
 * DIS_STAGE_FALLBACK and the debug dumps describe the backward pass (DX0 / DY0
 * are then the second frame's gradients). */
dis_status dis_calc_bidir_batch_u8(dis_ctx* ctx, int n, const uint8_t* I0, const uint8_t* I1,
                                   size_t stride, size_t pair_stride,
                                   float* flow_fw, float* flow_bw, dis_mem where, void* stream);

/* Temporal warm start (added within ABI v8: purely additive, DIS_ABI_VERSION
 * unchanged; the reference always starts from zero, src/patch_grid.cpp:45,80;
 * OpenCV's DIS takes an in/out flow the same way). A warm-started call behaves
 * as if a level C+1 had produced a dense flow: a coarsest-level patch with
 * reference pixel (rx, ry) starts at 2 * I[ry >> 1][rx >> 1], exactly as every
 * finer level starts from the level above it. I is the pair's init plane:
 * iw x ih = (W_C + 1) / 2 x (H_C + 1) / 2 float2 (u, v), row stride iw, in
 * level-(C+1) pixels, W_C x H_C the padded frame's level-C size
 * (dis_init_plane_size). `init` comes in one of two forms:
 *   DIS_INIT_COARSE:  n such planes, pair stride iw * ih float2;
 *   DIS_INIT_FULLRES: n W x H x 2 flows in full-resolution pixels, the layout
 *     dis_calc_batch_u8 writes (a previous call's output is a valid argument).
 *     The engine extends each to the padded frame (replicate) and halves it
 *     C+1 times, P_{j+1}(x, y) = ((a + b) + (c + d)) * 0.125f over the 2 x 2
 *     block a b / c d of P_j, every f32 operation separately rounded; only the
 *     last step can meet an odd size, and clamps its source indices.
 * In both forms the search reads a context-owned plane, never the caller's
 * memory: the kernel that fills it replaces every input component that is not
 * finite or has |c| >= 1e9 by 0 (dis_flow_color's notion of an invalid
 * vector). Finite starts of any size are safe: a start outside the level's
 * valid region is rejected by the search and the patch keeps its init.
 *
 * init == NULL is dis_calc_batch_u8, bit for bit; an all-zero plane gives the
 * same flow. Works with every kernel variant, patch size, paper_mode,
 * var_refine_iters, both precisions and any concurrency. `init` may be the
 * very buffer `flow` points to (flow in, flow out): the plane is filled on the
 * call's stream before the level chain is enqueued on it (and on streams
 * forked from it), so stream order completes the plane before any output is
 * written. Any other overlap of init with flow, and any overlap of init with
 * the frames, is refused. Always enqueued eagerly (never a replayed graph, and
 * the graph cache is not touched): the cache is keyed by the call's buffers
 * and a captured graph holds its arguments, while a video loop changes the
 * init buffer every call; one more key would evict the plain call's graphs.
 * DIS_MEM_HOST is synchronous and stages through device buffers for max_batch
 * pairs that the context allocates on the first such call
 * (DIS_ERR_OUT_OF_MEMORY if that fails); the chunked host pipeline is not
 * used. The context's init planes (a few KB) are allocated by dis_create.
 * dis_flow_to_init is the reduction alone, into the caller's planes (device
 * pointers 8-byte aligned; it touches no context workspace). Under
 * DIS_FLOW_F16 `flow`, a DIS_INIT_FULLRES `init` and dis_flow_to_init's `flow`
 * are format-typed (halves; device pointers 4-byte aligned); DIS_INIT_COARSE
 * planes and dis_flow_to_init's output stay float. */
typedef enum dis_init_kind { DIS_INIT_COARSE = 0, DIS_INIT_FULLRES = 1 } dis_init_kind;
dis_status dis_init_plane_size(dis_ctx* ctx, int* iw, int* ih);
dis_status dis_flow_to_init(dis_ctx* ctx, int n, const float* flow, float* init_planes,
                            dis_mem where, void* stream);
dis_status dis_calc_batch_init_u8(dis_ctx* ctx, int n, const uint8_t* I0, const uint8_t* I1,
                                  size_t stride, size_t pair_stride,
                                  const float* init, int init_kind,
                                  float* flow, dis_mem where, void* stream);

/* Host-frame path (ABI v8): with DIS_MEM_HOST a batch runs in chunks of
 * chunk_pairs pairs (0 = auto, the default: about 64 MB of flow per chunk)
 * through two device slots; chunk j+1's upload, chunk j's computation and
 * chunk j-1's download overlap (the downloads are issued by a thread of the
 * context). The copies go straight between the caller's buffers and the
 * device; page-locked caller buffers (dis_host_alloc, hipHostMalloc /
 * hipHostRegister) make them asynchronous. The results are the device path's,
 * bit for bit, for any chunking. The reference's per-pair loop hands over host
 * frames and gets host flow back (src/main.cpp:102-206). */
dis_status dis_set_host_pipeline(dis_ctx* ctx, int chunk_pairs);
typedef struct dis_host_info {
    int chunk_pairs;     /* pairs per chunk (0 before the first host call)          */
    int last_chunks;     /* chunks of the last host call                            */
    int last_direct_in;  /* 1: the last host call's frames were page-locked         */
    int last_direct_out; /* 1: the last host call's flow buffer was page-locked     */
} dis_host_info;
dis_status dis_host_pipeline_info(dis_ctx* ctx, dis_host_info* out);
/* Page-locked host memory for frames and flows (hipHostMalloc); no context. */
dis_status dis_host_alloc(size_t bytes, void** out);
dis_status dis_host_free(void* p);

/* Compatibility entry with the exact semantics of the reference constructor
 * OpticalFlowClass(...) (include/optical_flow.hpp:43-54): host pyramids of
 * (coarsest+1) PADDED planes (row stride W_l + 2*img_padding, pointer at the
 * padded origin, as built by construct_pyramide, src/main.cpp:41-49), output
 * `outflow` = (width>>F) x (height>>F) x 2 floats at the finest level.
 * width/height must be multiples of 2^coarsest. The *_dx/_dy planes of the
 * second frame are accepted and unused, as in the reference (Q15).
 * Synchronous; runs on HIP device `device`. */
dis_status dis_flow_from_pyramids(const float* const* img_first, const float* const* img_first_dx,
                                  const float* const* img_first_dy, const float* const* img_second,
                                  const float* const* img_second_dx, const float* const* img_second_dy,
                                  int img_padding, float* outflow, int width, int height,
                                  int coarsest_scale, int finest_scale, int iterations,
                                  int patch_size, float patch_overlap, int patch_normalization,
                                  int device);

/* Stage dumps for parity tests: copy one intermediate of pair `pair` from the
 * last calc on this context into host memory `dst` (count floats). Stages:
 * level image frame 0 / frame 1, frame-0 Sobel dx / dy, per-patch u (n_l*2),
 * dense flow (W_l*H_l*2). Requires dis_set_debug(ctx, 1) before the calc.
 * DIS_STAGE_FALLBACK (count 1, no debug mode needed): the number of patch
 * blocks of level `level` whose start positions were too spread for the LDS
 * tile and were searched by the fallback kernel in the last dis_calc_* on this
 * context (graph replays included), summed over the call's sub-batches (`pair`
 * only has to lie in the last batch). dis_flow_from_pyramids has no context
 * and keeps its own counters: a context's count is never changed by it. */
typedef enum dis_stage {
    DIS_STAGE_IMG0 = 0,
    DIS_STAGE_IMG1 = 1,
    DIS_STAGE_DX0 = 2,
    DIS_STAGE_DY0 = 3,
    DIS_STAGE_PATCH_U = 4,
    DIS_STAGE_DENSE = 5,
    DIS_STAGE_FALLBACK = 6
} dis_stage;
dis_status dis_set_debug(dis_ctx* ctx, int enable);

/* Concurrency: a batch call is split into `streams` sub-batches (1..8,
 * default 2) that run on context-owned HIP streams forked from and joined
 * back into the caller's stream. Results do not depend on this setting. */
dis_status dis_set_concurrency(dis_ctx* ctx, int streams);

/* Kernel variant: 0 = auto (specialised kernels where available: the
 * patch_size-8 search with 8 lanes per patch on levels with few patches and 2
 * lanes per patch on the rest), 1 = generic kernels only, 2 / 3 / 4 / 5 = the
 * patch_size-8 search with 4 / 2 / 8 / 1 lanes per patch on every level (5:
 * where the 16x8-patch block fits, grid step <= 7; else 2), 6 = one wave64
 * per patch (lane = pixel) on every exact non-paper level (else 2), 9 = 2
 * lanes per patch on every level with the usable LDS tile
 * capped at 24 rows / columns, so that most patch blocks take the fallback
 * list and kernel (a parity-test switch: natural inputs rarely spread a
 * block's start positions beyond the full tile). All are bit-identical; the
 * switch exists for parity tests and A/B timing. 7 and 8 (ABI v6: one launch
 * per coarse level, the fused coarse head) were removed in v7 -- the head
 * measured slower -- and are refused. */
dis_status dis_set_kernel_variant(dis_ctx* ctx, int variant);

/* Arithmetic of the patch_size-8 search kernels (ABI v4; no reference
 * counterpart -- the reference's own rounding is DIS_PRECISION_EXACT):
 *   DIS_PRECISION_EXACT (default): every float operation separately rounded in
 *     the reference's order -- bit-identical to the oracle;
 *   DIS_PRECISION_FMA: the bilinear warp, the steepest-descent and Hessian dot
 *     products contracted into fma, the LU solve by the pivots' reciprocals --
 *     within the stated tolerance of the reference (mean EPE
 *     <= 3.3e-4 px, p99.9 <= 5.1e-2 px, patch flips <= 0.014 %), faster.
 * Generic kernels (other patch sizes) and paper mode always run exact. */
/* HIP graphs (ABI v4): with graphs on (the default) a batch call is captured
 * once per (n, frame/flow pointers and strides, concurrency, precision,
 * variant) and replayed as one graph -- the fork into the sub-batch streams,
 * every level's launches and the join -- instead of ~25 eager launches; a
 * changed key re-captures (an LRU of four executable graphs per context; an
 * exec is updated only after its previous replay has finished). Kernel timing,
 * debug dumps and variational refinement run eagerly. The
 * capture is thread-local: if another thread synchronises the device or uses
 * the legacy default stream meanwhile, HIP invalidates it and that call runs
 * eagerly instead. Results do not depend on this setting. */
dis_status dis_set_graphs(dis_ctx* ctx, int enable);

/* Stream plans of a batch call (ABI v8; host only, no device needed). Ops are
 * 4 ints each: {kind (0 record, 1 wait, 2 work), stream (0 = the caller's,
 * 1 + k = sub-batch stream k), event (0 = fork, 1 + k = sub-batch k's join),
 * stage}. dis_batch_stream_plan writes the plan a call with `nsub` (2..8)
 * sub-batches and `nstages` stages issues (count ops; ops may be NULL to ask
 * for the count). dis_check_stream_plan applies the rules a plan must keep to
 * be captured into a HIP graph (every waited event recorded in the capture,
 * work only on streams in it, every stream joined back) and
 * returns DIS_ERR_UNSUPPORTED with the broken rule in dis_last_error()
 * otherwise. The runtime checks its plan this way before every capture. */
dis_status dis_batch_stream_plan(int nsub, int nstages, int* ops, int capacity, int* count);
dis_status dis_check_stream_plan(const int* ops, int nops, int nstreams, int nevents);

typedef enum dis_precision { DIS_PRECISION_EXACT = 0, DIS_PRECISION_FMA = 1 } dis_precision;
dis_status dis_set_precision(dis_ctx* ctx, int mode);

/* ABI v6: dis_pipeline_link (v5) is gone -- its linked calls ran eagerly on
 * the device's shared sub-batch streams and lost to two unlinked contexts on
 * two caller streams (DESIGN.md 4 "pipelined"), which needs no API. */
dis_status dis_stage_size(dis_ctx* ctx, int stage, int level, size_t* count);
dis_status dis_debug_dump(dis_ctx* ctx, int stage, int level, int pair, float* dst, size_t count);

/* Per-kernel timing with HIP events recorded on the context's launch stream
 * around every launch of the named kernel class (bench / roofline use).
 * kernel: 0 = fused pyramid, 1 = patch search (all levels), 2 = patch search
 * (finest level only), 3 = fused densify+upsample+crop, 4 / 5 = variational
 * refinement's linearisation / SOR launches at the finest level (ABI v7;
 * timing replaces the refinement's per-level graphs by eager launches),
 * 6 = the init-plane launch of a warm-started call (the reduction or the copy),
 * 7 = the luma launch of a colour frame format (dis_set_frame_format).
 * Enabling timing while
 * it is off starts a fresh measurement (accumulated launches and times are
 * cleared); dis_kernel_time returns the totals since then (the event pool
 * grows as needed, so no launch is left out; DIS_ERR_DEVICE if event creation
 * failed and records were lost). */
dis_status dis_set_kernel_timing(dis_ctx* ctx, int enable);
dis_status dis_kernel_time(dis_ctx* ctx, int kernel, int* launches, double* total_ms);

/* Middlebury flow colour coding, src/color_coding.cpp:13-117 (draw_optical_flow
 * with compute_color): n W x H (u,v) float fields (interleaved, row-major,
 * pair stride W*H*2) to n W x H x 3 u8 BGR images (OpenCV Vec3b order).
 * maxmotion > 0 fixes the motion range; <= 0 uses max(1, max |u| over valid
 * pixels) per field, as the reference's default -1. Invalid vectors (NaN or
 * |component| >= 1e9) are black. Host pointers: synchronous; device pointers:
 * asynchronous on `stream`. Runs on HIP device `device`. Any n >= 1 runs: the
 * field index travels in the launch grid's y extent, and a call with more than
 * 65,535 fields goes out in launches of at most that many. */
dis_status dis_flow_color(const float* flow, int n, int width, int height, float maxmotion, uint8_t* bgr,
                          dis_mem where, void* stream, int device);

/* Forward-backward consistency of n W x H (u,v) fields (added within ABI v8,
 * additive; no context, like dis_flow_color; no reference counterpart). With
 * fw(x,y) = (u,v) and s = bw sampled bilinearly at (x+u, y+v):
 *   err  = |fw + s|^2,  mask = err <= alpha1 * (|fw|^2 + |s|^2) + alpha2 ? 255 : 0;
 * a target outside [0,W-1] x [0,H-1] or a NaN vector gives mask 0, err +inf.
 * Every operation is a separately rounded f32 one (DESIGN.md "Bidirectional
 * flow"). alpha1, alpha2 finite and >= 0 (the literature's 0.01 and 0.5 are
 * the bindings' defaults); mask n*W*H bytes; err n*W*H floats or NULL. Device
 * pointers: fw and bw 8-byte aligned, asynchronous on `stream`; host pointers:
 * synchronous. bw's mask is the same call with the two fields swapped. */
dis_status dis_flow_consistency(const float* fw, const float* bw, int n, int width, int height,
                                float alpha1, float alpha2, uint8_t* mask, float* err /* may be NULL */,
                                dis_mem where, void* stream, int device);

/* Backward warp of u8 images by flow fields (added within ABI v8, additive; no
 * context, like dis_flow_color; no reference counterpart). With `flow` the
 * I0 -> I1 field and `src` = I1, `dst` reconstructs I0.
 *   src:   n images of W x H pixels of `channels` (1, 3 or 4) interleaved u8
 *          samples; row stride src_stride bytes (0 = W*channels, else >= that),
 *          image stride src_image_stride bytes (0 = stride*H, else >= that), as
 *          dis_calc_batch_u8's stride / pair_stride;
 *   flow:  n W x H (u,v) fields in the layout the engine writes, floats
 *          (DIS_FLOW_F32) or halves (DIS_FLOW_F16, widened exactly);
 *   dst:   n dense W x H x channels images; valid (may be NULL): n W x H bytes.
 * For pixel (x, y) of image k with flow vector (u, v):
 *   1. u or v NaN or |c| >= 1e9 (dis_flow_color's invalid vector, +-inf
 *      included): every channel of dst is 0 and valid is 0, in both border modes;
 *   2. else px = (float)x + scale*u, py = (float)y + scale*v, the product and the
 *      sum separately rounded (scale = 1 gives exactly x + u);
 *   3. inside = px >= 0 && px <= W-1 && py >= 0 && py <= H-1; valid = inside ? 255 : 0;
 *   4. not inside: DIS_BORDER_ZERO writes 0 to every channel; DIS_BORDER_REPLICATE
 *      clamps px into [0, W-1] and py into [0, H-1] and goes on;
 *   5. x0 = floorf(px), a = px - x0, ix0 = (int)x0, ix1 = min(ix0+1, W-1), likewise
 *      y0, b, iy0, iy1; ia = 1-a, ib = 1-b; w00 = ia*ib, w01 = a*ib, w10 = ia*b,
 *      w11 = a*b; per channel, with p the tap's byte as a float,
 *      s = ((w00*p00 + w01*p01) + w10*p10) + w11*p11 (dis_flow_consistency's
 *      sampler: same taps, same order), and the output byte is rintf(s) (ties to
 *      even) clamped to [0, 255].
 * Every operation is a separately rounded f32 one. Every tap index comes after
 * the invalid test and the clamp, so no input value leads to a read outside the
 * frame. Refused with DIS_ERR_INVALID_ARGUMENT, before any device call: a null
 * src, flow or dst; n, width or height < 1; width or height > 2^24; other
 * channels, flow_format, border or where; strides smaller than the row / image;
 * a scale that is not finite or has |scale| > 1024; any overlap of dst or valid
 * with src, flow or each other; more work than one launch's grid holds; for
 * DIS_MEM_DEVICE a flow pointer not aligned to one (u,v) pair (8 bytes F32,
 * 4 bytes F16). Image pointers need no alignment (aligned ones and W % 4 == 0
 * get wider accesses, same bytes). Host pointers: synchronous, staged through
 * HIP device `device`; device pointers: asynchronous on `stream`. */
typedef enum dis_border { DIS_BORDER_REPLICATE = 0, DIS_BORDER_ZERO = 1 } dis_border;
dis_status dis_flow_warp_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                            const void* flow, int flow_format, int n, int width, int height,
                            float scale, int border, uint8_t* dst, uint8_t* valid /* may be NULL */,
                            dis_mem where, void* stream, int device);

/* The frame at time t in [0, 1] between I0 (t = 0) and I1 (t = 1) (added within
 * ABI v8, additive; no context, like dis_flow_warp_u8; no reference counterpart):
 * the Middlebury interpolation algorithm (Baker et al., IJCV 2011, section 3.3).
 * The forward flow is projected to time t, collisions go to the photoconsistent
 * candidate, holes are filled apart, and both frames are sampled with the
 * projected flow.
 *   I0, I1: n images each of W x H pixels of `channels` (1, 3 or 4) interleaved
 *           u8 samples; both with row stride `stride` and image stride
 *           `image_stride` in bytes (0 = dense), dis_flow_warp_u8's conventions;
 *   fw, bw: the I0 -> I1 and the I1 -> I0 fields, n W x H (u,v) each, both floats
 *           (DIS_FLOW_F32) or both halves (DIS_FLOW_F16, widened exactly); bw may
 *           be NULL;
 *   dst:    n dense W x H x channels images; fill (may be NULL): n W x H bytes;
 *   workspace: n*W*H uint64 keys (dis_flow_interp_workspace gives the bytes),
 *           8-byte aligned; required for DIS_MEM_DEVICE, ignored for DIS_MEM_HOST
 *           (the call stages everything and allocates its own).
 * Every f32 operation is separately rounded. tb = 1.0f - t. A vector (u, v) is
 * valid when |u| < 1e9 && |v| < 1e9 (false for NaN). sample(I, x, y, u, v, k)
 * is dis_flow_warp_u8's steps 2-5 with scale k and DIS_BORDER_REPLICATE on
 * image I at pixel (x, y): px = (float)x + k*u, py = (float)y + k*v, the `inside`
 * flag, the clamp, and the unrounded sum s of every channel.
 *   1. Splat. Pixel (x, y) of I0 takes part when fw(x, y) = (u, v) is valid and
 *      sample(I1, x, y, u, v, 1) is inside. cost = sum over the channels, in
 *      their order, of |(float)I0_c(x, y) - s_c|; key = (uint64)bits(cost) << 32 |
 *      (y*W + x). tx = (float)x + t*u, ty = (float)y + t*v; the targets are
 *      {floorf(tx), ceilf(tx)} x {floorf(ty), ceilf(ty)} without duplicates
 *      and without those outside [0, W-1] x [0, H-1] (tested as floats); each
 *      target q gets workspace[k*W*H + q] = min(itself, key), from ~0 at the start.
 *      The bits of a non-negative float order as unsigned integers, so the lowest
 *      cost wins and, among equal costs, the lowest source index: a minimum over
 *      distinct keys does not depend on the order of arrival, and every run
 *      writes the same bytes.
 *   2. Blend. For output pixel (x, y) with key K:
 *      K != ~0: (u, v) = fw at source index K & 0xffffffff, fill = 0;
 *        s0 = sample(I0, x, y, u, v, -t), s1 = sample(I1, x, y, u, v, tb);
 *        both inside or neither: r = tb*s0 + t*s1 (two products, one sum);
 *        only s0 inside: r = s0; only s1 inside: r = s1;
 *      K == ~0, bw given, bw(x, y) valid and sample(I1, x, y, bw, -tb) inside:
 *        r = that sample, fill = 1 (a disoccluded pixel, visible only in I1);
 *      any other hole: fill = 2, (u, v) = fw(x, y), or (0, 0) if that is not
 *        valid, and the three cases of K != ~0.
 *      The output byte is rintf(r) (ties to even) clamped to [0, 255].
 * No tap or target index is formed before the validity test and the clamp or
 * the frame test. t = 1 gives I1 exactly; t = 0 gives I0 exactly when bw is NULL.
 * Refused with DIS_ERR_INVALID_ARGUMENT, before any device call:
 * dis_flow_warp_u8's list (null I0, I1, fw or dst; sizes; channels; flow_format;
 * where; strides; the grid), a t that is not finite or lies outside [0, 1],
 * W*H > 2^31, any overlap of dst, fill or workspace with I0, I1, fw, bw or each
 * other, and for DIS_MEM_DEVICE a NULL workspace, one that is not 8-byte aligned,
 * or an fw or bw not aligned to one (u,v) pair. Host pointers: synchronous,
 * staged through HIP device `device`; device pointers: asynchronous on `stream`
 * (one hipMemsetAsync of the workspace to 0xFF, then two kernel launches). */
dis_status dis_flow_interp_workspace(int n, int width, int height, size_t* bytes); /* n*W*H*8 */
dis_status dis_flow_interp_u8(const uint8_t* I0, const uint8_t* I1, size_t stride, size_t image_stride,
                              int channels, const void* fw, const void* bw /* may be NULL */, int flow_format,
                              int n, int width, int height, float t,
                              uint8_t* dst, uint8_t* fill /* may be NULL */,
                              void* workspace, dis_mem where, void* stream, int device);

/* Composition of flow fields (added within ABI v8, additive; no context, like
 * dis_flow_warp_u8; no reference counterpart): with `a` the field from frame 0
 * to frame k and `b` the field from frame k to frame k+1, `out` is the field
 * from frame 0 to frame k+1, out(x) = a(x) + b(x + a(x)). Chaining the pair
 * flows of a video this way follows every pixel of frame 0 through it.
 *   a, b, out: n W x H (u,v) fields each in the layout the engine writes, floats
 *          (DIS_FLOW_F32) or halves (DIS_FLOW_F16, widened exactly); the three
 *          formats are independent (f16 pair flows accumulate into an f32
 *          field; an f16 accumulator loses whole pixels beyond |v| = 2048);
 *   valid_a, mask_b, valid_out (each may be NULL): n*W*H bytes, nonzero =
 *          trusted; valid_a is typically the previous call's valid_out, mask_b
 *          dis_flow_consistency's mask of pair k.
 * Every f32 operation is separately rounded. A vector is valid when
 * |u| < 1e9 && |v| < 1e9 (false for NaN). For pixel (x, y) of field f with
 * (u, v) = a(x, y):
 *   1. (u, v) not valid, or valid_a given and its byte 0: the pixel is invalid;
 *   2. px = (float)x + u, py = (float)y + v; unless px >= 0 && px <= W-1 &&
 *      py >= 0 && py <= H-1 the pixel is invalid;
 *   3. the taps of dis_flow_consistency: x0 = floorf(px), a = px - x0,
 *      ix0 = (int)x0, ix1 = min(ix0+1, W-1), likewise y0, b, iy0, iy1; ia = 1-a,
 *      ib = 1-b; w00 = ia*ib, w01 = a*ib, w10 = ia*b, w11 = a*b;
 *   4. any of the four tap vectors of b not valid, or mask_b given and any of
 *      the four tap bytes 0: the pixel is invalid (a tap whose weight is 0
 *      counts too: a test on the inputs, not a consequence of the arithmetic);
 *   5. su = ((w00*b00.x + w01*b01.x) + w10*b10.x) + w11*b11.x, sv likewise;
 *      out = (u + su, v + sv), narrowed once with the engine's own conversion if
 *      out_format is F16; valid_out = 255;
 *   6. an invalid pixel writes the canonical quiet NaN to both components (f32
 *      bits 0x7fc00000, f16 bits 0x7e00) and valid_out = 0: what dis_flow_color,
 *      dis_flow_warp_u8 and dis_flow_interp_u8 treat as an invalid vector.
 * No tap index is formed before the tests of steps 1 and 2. `out` may be the
 * very buffer `a` when out_format == a_format (in-place accumulation: each
 * pixel's vector is read before it is written, by the same lane) and valid_out
 * the very buffer valid_a; every other overlap of out or valid_out with a, b,
 * valid_a, mask_b or each other is refused. Refused with
 * DIS_ERR_INVALID_ARGUMENT, before any device call: a null a, b or out; n, width
 * or height < 1; width or height > 2^24; formats other than F32 / F16; an
 * unknown `where`; an overlap the rule above does not allow; more work than one
 * launch's grid holds; for DIS_MEM_DEVICE a field pointer not aligned to one
 * (u,v) pair of its format (8 bytes F32, 4 bytes F16). Host pointers:
 * synchronous, staged through HIP device `device`; device pointers: asynchronous
 * on `stream`, one launch. */
dis_status dis_flow_compose(const void* a, int a_format, const void* b, int b_format,
                            int n, int width, int height,
                            const uint8_t* valid_a /* may be NULL */, const uint8_t* mask_b /* may be NULL */,
                            void* out, int out_format, uint8_t* valid_out /* may be NULL */,
                            dis_mem where, void* stream, int device);

/* Points moved by flow fields (added within ABI v8, additive; no context): n
 * fields, each with `count` points (x, y) as float pairs, field k's points from
 * k*count*2 floats on. For a point (x, y):
 *   1. unless x >= 0 && x <= W-1 && y >= 0 && y <= H-1 (false for NaN), or when
 *      any of its four tap vectors (dis_flow_compose's step 3 with px = x,
 *      py = y) is not valid, points_out gets the input bits unchanged and
 *      status 0;
 *   2. else points_out = (x + su, y + sv) (step 5's sums) and status 255, even
 *      if the new position lies outside the frame: the next call reports that.
 * points_out may be exactly `points`; every other overlap of points_out or
 * status (may be NULL, n*count bytes) with flow, points or each other is
 * refused, as are a null flow, points or points_out, n, width, height or
 * count < 1, width or height > 2^24, another flow_format or `where`, more points
 * than one launch's grid holds, and for DIS_MEM_DEVICE a flow pointer not
 * aligned to one (u,v) pair or point pointers not 8-byte aligned. Host
 * pointers: synchronous; device pointers: asynchronous on `stream`, one launch. */
dis_status dis_flow_advect_points(const void* flow, int flow_format, int n, int width, int height,
                                  const float* points, int count, float* points_out,
                                  uint8_t* status /* may be NULL */, dis_mem where, void* stream, int device);

/* Untrusted flow vectors filled from trusted ones (added within ABI v8,
 * additive; no context): validity-weighted push-pull (Gortler et al., "The
 * Lumigraph", section 4) over n W x H (u,v) fields, the stage between
 * "bidirectional flow + mask" (dis_flow_consistency, dis_flow_compose's
 * valid_out) and applying the flow. Every f32 operation is separately rounded.
 *   flow, out: n W x H (u,v) fields in the layout the engine writes, floats
 *          (DIS_FLOW_F32) or halves (DIS_FLOW_F16, widened exactly first); the
 *          two formats are independent;
 *   mask (may be NULL): n*W*H bytes, nonzero = trusted;
 *   level (may be NULL): n*W*H bytes, see below.
 * Levels: level 0 is the field, W_0 x H_0 = W x H; W_{l+1} = (W_l + 1) / 2 and
 * H likewise, until 1 x 1 at level L (L = 0 for a 1 x 1 field, 11 for 1080p).
 * Trust: ok_0(x, y) = |u| < 1e9 && |v| < 1e9 (false for NaN) && (mask == NULL
 * || its byte != 0).
 * Pull, for l = 0 .. L-1: cell (X, Y) of level l+1 has the children c00 = (2X,
 * 2Y), c01 = (2X+1, 2Y), c10 = (2X, 2Y+1), c11 = (2X+1, 2Y+1) of level l; a
 * child outside W_l x H_l is not ok. c = the number of ok children;
 * ok_{l+1} = c > 0. If ok: f = the first ok child's vector in that order;
 * d_i = ok_i ? v_i - f : 0 per component (a select: an untrusted vector never
 * enters arithmetic); m = f + ((d00 + d01) + (d10 + d11)) * k[c] with k[1] =
 * 1.0f, k[2] = 0.5f, k[3] = the float with the bits 0x3eaaaaab, k[4] = 0.25f.
 * (This form returns a constant exactly when all ok children are equal; a
 * plain sum times 1/3 does not.)
 * Empty field: if ok_L(0, 0) is false, every pixel of `out` gets the canonical
 * quiet NaN (f32 bits 0x7fc00000, f16 bits 0x7e00) and `level` 255.
 * Push, for l = L-1 .. 0, with g_L = m_L: for cell (x, y) of level l,
 * g_l = ok_l ? m_l (level 0: the input vector) : r, where px = x >> 1,
 * py = y >> 1, qx = clamp(px + (x & 1 ? 1 : -1), 0, W_{l+1} - 1), qy likewise;
 * P = g_{l+1}(px, py), Q = g_{l+1}(qx, py), R = g_{l+1}(px, qy),
 * S = g_{l+1}(qx, qy); h0 = P + 0.25f * (Q - P); h1 = R + 0.25f * (S - R);
 * r = h0 + 0.25f * (h1 - h0): the bilinear 9/3/3/1 upsample in lerp form (every
 * cell of g_{l+1} is defined, so no weights are needed).
 * Output: a trusted pixel keeps its input vector in out_format (equal formats:
 * the same bits; F16 -> F32: widened exactly; F32 -> F16: the engine's own
 * narrowing); every other pixel gets g_0, narrowed once if out_format is F16.
 * level: the smallest l with ok_l(x >> l, y >> l): 0 = kept, larger = the
 * nearest trusted data is about 2^l pixels away (callers threshold it).
 * Workspace: dis_flow_fill_workspace returns 8 * n * sum_{l=1..L} W_l * H_l
 * bytes (0 for a 1 x 1 field, and `workspace` may then be NULL): required and
 * 8-byte aligned for DIS_MEM_DEVICE, ignored for DIS_MEM_HOST; its contents are
 * unspecified. `out` may be the very buffer `flow` when the formats are equal
 * (each pixel's vector is read before it is written, by the same lane); every
 * other overlap of out, level or workspace with flow, mask or each other is
 * refused. Refused with DIS_ERR_INVALID_ARGUMENT, before any device call: a
 * null flow, out or bytes; n, width or height < 1; width or height > 2^24;
 * formats other than F32 / F16; an unknown `where`; an overlap the rule above
 * does not allow; more work than one launch's grid holds; for DIS_MEM_DEVICE a
 * missing or misaligned workspace or a field pointer not aligned to one (u,v)
 * pair of its format (8 bytes F32, 4 bytes F16). Host pointers: synchronous,
 * staged through HIP device `device`; device pointers: asynchronous on
 * `stream`, three launches (five or more when level 5 exceeds one block's
 * LDS: beyond about 4600 level-5 cells, as for 4K frames). */
dis_status dis_flow_fill_workspace(int n, int width, int height, size_t* bytes);
dis_status dis_flow_fill(const void* flow, int flow_format, const uint8_t* mask /* may be NULL */,
                         int n, int width, int height,
                         void* out, int out_format, uint8_t* level /* may be NULL */,
                         void* workspace, dis_mem where, void* stream, int device);

/* Global motion from flow fields (added within ABI v8, additive; no context):
 * a parametric model fitted to the trusted vectors of each of n W x H (u,v)
 * fields by least squares and refitted `iterations` times on the vectors that
 * agree with it, on the GPU; what a stabiliser needs of a flow. For every model
 * the result is six floats per field in frame coordinates (x, y the pixel
 * indices):
 *   u(x, y) = (p0 + p1*x) + p2*y,   v(x, y) = (p3 + p4*x) + p5*y;
 * translation has p1 = p2 = p4 = p5 = 0, similarity p1 = p5 and p4 = -p2.
 *   flow:  n fields in the layout the engine writes, floats (DIS_FLOW_F32) or
 *          halves (DIS_FLOW_F16, widened exactly first);
 *   mask (may be NULL): n*W*H bytes, nonzero = trusted;
 *   params: n*6 floats; info (may be NULL): n*4 words; inliers (may be NULL):
 *          n*W*H bytes.
 * The result is defined by its arithmetic, all of it f64 with every operation
 * rounded on its own. cx = (W-1)/2, cy = (H-1)/2, x' = x - cx, y' = y - cy;
 * (u, v) the pixel's vector widened to double (the products of two of these
 * values are exact: only the additions round).
 * Trusted: |u| < 1e9 && |v| < 1e9 on the f32 values (false for NaN) && (mask ==
 * NULL || its byte != 0).
 * Passes j = 0 .. iterations. Members of pass 0: the trusted pixels; of pass
 * j >= 1: the trusted pixels with r2 <= T2 against the centred model c of pass
 * j-1, T2 = (double)threshold * (double)threshold, eu = (c0 + c1*x') + c2*y',
 * ev = (c3 + c4*x') + c5*y', ru = u - eu, rv = v - ev, r2 = ru*ru + rv*rv (the
 * bound is inclusive; a NaN model has no members). A member contributes the
 * twelve terms 1, x', y', x'x', x'y', y'y', u, x'u, y'u, v, x'v, y'v, every
 * other pixel +0.0 twelve times.
 * Order of summation, per field and term: pixels are indexed row-major,
 * q = y*W + x, and cut into chunks of 16384. In a chunk, slot i (0..255) starts
 * from +0.0 and adds the terms of pixels chunk*16384 + k*256 + i for k = 0..63
 * in that order (pixels past the field's end: +0.0); the 256 slots are
 * combined in eight rounds of adjacent pairs, a[i] = a[2i] + a[2i+1]; the chunk
 * sums are added in increasing chunk order, starting from +0.0.
 * Solve, with the sums S1 Sx Sy Sxx Sxy Syy Su Sxu Syu Sv Sxv Syv:
 *   affine:      A = [[S1 Sx Sy] [Sx Sxx Sxy] [Sy Sxy Syy]], right-hand sides
 *                (Su Sxu Syu) -> (c0 c1 c2) and (Sv Sxv Syv) -> (c3 c4 c5);
 *   similarity:  unknowns (tx ty s r), u = tx + s*x' - r*y', v = ty + r*x' +
 *                s*y'; A = [[S1 0 Sx -Sy] [0 S1 Sy Sx] [Sx Sy Sxx+Syy 0]
 *                [-Sy Sx 0 Sxx+Syy]], right-hand side (Su Sv Sxu+Syv Sxv-Syu);
 *                c = (tx s -r ty r s);
 *   translation: S1*c0 = Su, S1*c3 = Sv; c1 = c2 = c4 = c5 = +0.0.
 * By LDL^T without pivoting: for column j, d_j = A_jj - sum_{k<j} (L_jk*L_jk)*d_k
 * and L_ij = (A_ij - sum_{k<j} (L_ik*L_jk)*d_k) / d_j, k ascending, each term
 * subtracted in turn; forward substitution (rows ascending, k ascending, z_i -=
 * L_ik*z_k), division by d, back substitution (rows descending, k ascending).
 * The fit fails when some d_j > 2^-20 * A_jj is false (too few members,
 * collinear members, none: a pivot that lost 20 bits of its diagonal element;
 * a design rule); then all six c are NaN, and the later passes have no members
 * and fail likewise.
 * Output: p0 = (c0 - c1*cx) - c2*cy, p3 = (c3 - c4*cx) - c5*cy in f64, each of
 * the six values rounded once to f32; a failed fit writes the bits 0x7fc00000
 * six times. info = {1 fitted / 0 failed, trusted = S1 of pass 0, fitted = S1 of
 * the last pass, agree}. inliers: 255 where a trusted pixel has r2 <= T2 against
 * the final centred model (in f64, as above), else 0; agree is the count of
 * those pixels, 0 when inliers is NULL.
 * Workspace: dis_flow_fit_motion_workspace returns n * (chunks*12 + 16) * 8
 * bytes, chunks = ceil(W*H / 16384): required and 8-byte aligned for
 * DIS_MEM_DEVICE, ignored for DIS_MEM_HOST; its contents are unspecified.
 * Refused with DIS_ERR_INVALID_ARGUMENT, before any device call: a null flow,
 * params or bytes; n, width or height < 1; width or height > 2^24; W*H > 2^31;
 * a format other than F32 / F16; an unknown model or `where`; iterations
 * outside 0..16; a threshold that is not finite or negative; any overlap of
 * params, info, inliers or the workspace with flow, mask or each other; more
 * work than one launch's grid holds; for DIS_MEM_DEVICE a missing or misaligned
 * workspace, a flow not aligned to one (u,v) pair of its format, params or info
 * not 4-byte aligned. Host pointers: synchronous, staged through HIP device
 * `device`; device pointers: asynchronous on `stream`, 2 * (iterations + 1)
 * launches and one more for inliers, no allocation, no host synchronisation. */
typedef enum dis_motion_model { DIS_MOTION_TRANSLATION = 0, DIS_MOTION_SIMILARITY = 1,
                                DIS_MOTION_AFFINE = 2 } dis_motion_model;
dis_status dis_flow_fit_motion_workspace(int n, int width, int height, size_t* bytes);
dis_status dis_flow_fit_motion(const void* flow, int flow_format, const uint8_t* mask /* may be NULL */,
                               int n, int width, int height, int model, int iterations, float threshold,
                               float* params /* n*6 */, uint32_t* info /* n*4, may be NULL */,
                               uint8_t* inliers /* n*W*H, may be NULL */,
                               void* workspace, dis_mem where, void* stream, int device);

/* The field of a motion model (added within ABI v8, additive; no context): n
 * W x H fields from n*6 parameters, in f32 with every operation rounded on its
 * own: u = (p0 + p1*(float)x) + p2*(float)y, v = (p3 + p4*(float)x) +
 * p5*(float)y, narrowed with the engine's own conversion when out_format is
 * DIS_FLOW_F16. A field is the canonical NaN everywhere (f32 bits 0x7fc00000,
 * f16 bits 0x7e00) when any of its six parameters is not finite. This is how a
 * model reaches dis_flow_warp_u8 (the stabilised frame) and dis_flow_compose
 * (the camera path). Refusals as above (sizes, format, `where`, the grid, an
 * overlap of out with params; for DIS_MEM_DEVICE out not aligned to one pair,
 * params not 4-byte aligned). One launch. */
dis_status dis_motion_to_flow(const float* params, int n, int width, int height,
                              void* out, int out_format, dis_mem where, void* stream, int device);

/* The camera path of a video smoothed, and per frame the model that steadies it
 * (added within ABI v8, additive; host only, no GPU, like dis_denoise_weights):
 * the stage between dis_flow_fit_motion and the warp of a stabiliser.
 *   pair_params: (n_frames-1)*6 floats, entry k what dis_flow_fit_motion writes
 *          for the flow from frame k to frame k+1 (may be NULL when n_frames is 1);
 *   corrections: n_frames*6 floats, entry k the model q whose field warps frame
 *          k into its stabilised version: it feeds dis_warp_motion_u8, or
 *          dis_motion_to_flow and from there dis_flow_warp_u8;
 *   status (may be NULL): n_frames bytes; replaced (may be NULL): one int.
 * The result is defined by its arithmetic, all of it f64 with every operation
 * rounded on its own and in the order stated. A matrix is 2 x 3 with an implied
 * third row 0 0 1; a product a.b has the entries (a_i0*b_0j + a_i1*b_1j), with
 * + a_i2 for j = 2, evaluated left to right.
 * Pair matrices: A_k = [[1+p1, p2, p0], [p4, 1+p5, p3]], each p widened from
 * f32; a model with any non-finite parameter is replaced by the identity, and
 * *replaced counts those models.
 * Path: C_0 = I, C_{k+1} = A_k . C_k.
 * Weights: g(d) = (double)(float)exp(-((double)d*d) / (2.0*(double)sigma*
 * (double)sigma)), dis_denoise_weights' rounding.
 * Smoothed path, per entry: S_k = (sum_j g(|j-k|)*C_j) / (sum_j g(|j-k|)), j
 * ascending over max(0, k-radius) .. min(n_frames-1, k+radius), both sums from
 * +0.0.
 * Inverse: det = s00*s11 - s01*s10; if det is not finite or |det| <= 2^-20,
 * frame k's correction is six times +0.0f and status[k] = 0. Otherwise
 * i00 = s11/det, i01 = -s01/det, i10 = -s10/det, i11 = s00/det,
 * i02 = -(i00*s02 + i01*s12), i12 = -(i10*s02 + i11*s12).
 * Correction: M_k = (C_k . S_k^-1) . Z with Z = [[z, 0, cx*(1-z)], [0, z,
 * cy*(1-z)]], z = 1.0/(double)zoom, cx = (width-1)/2.0, cy = (height-1)/2.0
 * (zoom > 1 magnifies about the centre, so that the moving borders leave the
 * picture); q = (m02, m00-1, m01, m12, m10, m11-1), each value rounded once to
 * f32, status[k] = 1; if any q is not finite the frame falls back to six times
 * +0.0f and status 0.
 * So identity pair models with zoom 1 give all-zero corrections bit for bit,
 * radius 0 gives M = (C_k . C_k^-1) . Z (Z itself where that product is exact,
 * as for translations), and n_frames = 1 is valid. Refused with
 * DIS_ERR_INVALID_ARGUMENT: a null pair_params when n_frames > 1; a null
 * corrections; n_frames < 1; width or height < 1 or > 2^24; radius outside
 * 0..1024; a sigma that is not finite or not > 0; a zoom that is not finite or
 * lies outside [1, 16]; any overlap of corrections, status or replaced with
 * pair_params or each other. DIS_ERR_OUT_OF_MEMORY, with nothing written, when
 * the 48 bytes of host memory a frame that the path needs cannot be had. */
dis_status dis_motion_stabilize(const float* pair_params /* (n_frames-1)*6 */, int n_frames,
                                int width, int height, int radius, float sigma, float zoom,
                                float* corrections /* n_frames*6 */, uint8_t* status /* n_frames, may be NULL */,
                                int* replaced /* may be NULL */);

/* Backward warp of u8 images by motion models (added within ABI v8, additive; no
 * context, like dis_flow_warp_u8; no reference counterpart): the stabilised
 * frame straight from six numbers. For image i and pixel (x, y), with
 * p = params + 6*i, in f32 with every operation rounded on its own:
 *   u = (p0 + p1*(float)x) + p2*(float)y, v = (p3 + p4*(float)x) + p5*(float)y
 * (dis_motion_to_flow's arithmetic exactly), then steps 1-5 of dis_flow_warp_u8
 * at scale = 1. An image with any non-finite parameter gets every channel 0 and
 * valid 0. dst and valid hold, bit for bit, what dis_motion_to_flow(DIS_FLOW_F32)
 * followed by dis_flow_warp_u8 writes; no field exists anywhere.
 *   src:   n images of W x H pixels of `channels` (1, 3 or 4) interleaved u8
 *          samples, dis_flow_warp_u8's strides (0 = dense);
 *   params: n*6 floats, where `where` says;
 *   dst:   n dense W x H x channels images; valid (may be NULL): n W x H bytes.
 * Refused with DIS_ERR_INVALID_ARGUMENT, before any device call: a null src,
 * params or dst; n, width or height < 1; width or height > 2^24; channels other
 * than 1, 3, 4; an unknown border or `where`; a stride smaller than a row or an
 * image; more work than one launch's grid holds (a block per 64 x 16 pixels);
 * any overlap of dst or valid with src, params or each other; for
 * DIS_MEM_DEVICE params not 4-byte aligned. Image pointers need no alignment
 * (aligned ones and W % 4 == 0 get wider accesses, same bytes). Host pointers:
 * synchronous, staged through HIP device `device`; device pointers:
 * asynchronous on `stream`, one launch, no allocation, no synchronisation. */
dis_status dis_warp_motion_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                              const float* params /* n*6 */, int n, int width, int height, int border,
                              uint8_t* dst, uint8_t* valid /* may be NULL */,
                              dis_mem where, void* stream, int device);

/* The homography (eight-parameter) motion family (added within ABI v8, additive;
 * no context): dis_flow_fit_motion, dis_motion_to_flow, dis_warp_motion_u8 and
 * dis_motion_stabilize again for projective models -- a camera that rotates.
 * Eight floats per model; p0..p5 have the affine family's meaning, p6 and p7 are
 * the projective row. In frame coordinates (x, y the pixel indices), with
 * g = p6*x + p7*y and d = 1 + g:
 *   u = (((p0 + p1*x) + p2*y) - x*g) / d,   v = (((p3 + p4*x) + p5*y) - y*g) / d,
 * the deviation form of the matrix [[1+p1 p2 p0] [p4 1+p5 p3] [p6 p7 1]].
 *
 * dis_flow_fit_homography: dis_flow_fit_motion without `model`; params is n*8
 * floats; flow, mask, iterations, threshold, info (n*4 words), inliers, the
 * workspace rule, the refusals and the launch counts are those of
 * dis_flow_fit_motion (2 * (iterations + 1) launches and one more for inliers).
 * dis_flow_fit_homography_workspace returns n * (chunks*27 + 16) * 8 bytes.
 * The result is defined by its arithmetic, all of it f64 with every operation
 * rounded on its own.
 * Coordinates: cx = (W-1)/2, cy = (H-1)/2; s = the smallest power of two >=
 * max(W, H, 2)/2; a = (x - cx)/s, b = (y - cy)/s, U = u/s, V = v/s with (u, v)
 * the pixel's vector widened to double (all exact); A = a + U, B = b + V.
 * Model: centred, scaled coefficients c0..c7 of the linear system
 *   U = c0 + c1*a + c2*b - c6*a*A - c7*b*A,  V = c3 + c4*a + c5*b - c6*a*B - c7*b*B.
 * Terms of a member, in this order (every other pixel: +0.0 27 times), with
 * aa = a*a, ab = a*b, bb = b*b, aA = a*A, bA = b*A, aB = a*B, bB = b*B,
 * Q = A*A + B*B:
 *    0..5   1, a, b, aa, ab, bb
 *    6..10  aA, bA, aa*A, ab*A, bb*A
 *   11..15  aB, bB, aa*B, ab*B, bb*B
 *   16..18  aa*Q, ab*Q, bb*Q
 *   19..24  U, a*U, b*U, V, a*V, b*V
 *   25, 26  aA*U + aB*V,  bA*U + bB*V
 * summed per term in dis_flow_fit_motion's order (256 slots x 64 pixels per
 * chunk of 16384, eight rounds of adjacent pairs, the chunks in turn).
 * Solve N c = r by dis_flow_fit_motion's LDL^T and pivot rule (d_j > 2^-20 *
 * N_jj), N symmetric 8 x 8 with G = [[S0 S1 S2] [S1 S3 S4] [S2 S4 S5]] at rows and
 * columns 0..2 and again at 3..5, zeros between the two; column 6 rows 0..5 =
 * (-S6 -S8 -S9 -S11 -S13 -S14), column 7 rows 0..5 = (-S7 -S9 -S10 -S12 -S14
 * -S15); N66 = S16, N67 = S17, N77 = S18; r = (S19 S20 S21 S22 S23 S24 -S25 -S26).
 * Members of pass 0: the trusted pixels (dis_flow_fit_motion's test); of pass
 * j >= 1, and the inliers: the trusted pixels with d > 0 and rU*rU + rV*rV <=
 * T2/(s*s) against the model c of pass j-1, where g = c6*a + c7*b, d = 1.0 + g,
 * eU = (((c0 + c1*a) + c2*b) - a*g) / d, eV = (((c3 + c4*a) + c5*b) - b*g) / d,
 * rU = U - eU, rV = V - eV, T2 = (double)threshold * (double)threshold: the
 * geometric residual in pixels against the threshold, both scaled by the power
 * of two s (exact); the bound is inclusive; a NaN model has no members.
 * The fit fails when a pivot fails, when a coefficient is not finite, or when
 * d = 1.0 + (c6*a + c7*b) is not > 1/8 at one of the frame's four corners (x in
 * {0, W-1}, y in {0, H-1}; a design rule: a model whose horizon approaches the
 * frame is no camera shake, and every later stage divides by d). Then all eight
 * c are NaN and the later passes have no members and fail likewise.
 * Output, conjugated back to frame coordinates and normalised by the bottom-
 * right entry w (d at pixel (0, 0), which the corner rule keeps above 1/8):
 * ax = cx/s, ay = cy/s, g00 = c6*((0 - cx)/s) + c7*((0 - cy)/s), w = 1.0 + g00,
 *   p0 = ((((s*c0) - c1*cx) - c2*cy) + cx*g00) / w,  p1 = ((c1 + ax*c6) - g00) / w,
 *   p2 = (c2 + ax*c7) / w,
 *   p3 = ((((s*c3) - c4*cx) - c5*cy) + cy*g00) / w,  p4 = (c4 + ay*c6) / w,
 *   p5 = ((c5 + ay*c7) - g00) / w,  p6 = (c6/s) / w,  p7 = (c7/s) / w,
 * each rounded once to f32; a failed fit writes the bits 0x7fc00000 eight times.
 * info and inliers as for dis_flow_fit_motion. */
dis_status dis_flow_fit_homography_workspace(int n, int width, int height, size_t* bytes);
dis_status dis_flow_fit_homography(const void* flow, int flow_format, const uint8_t* mask /* may be NULL */,
                                   int n, int width, int height, int iterations, float threshold,
                                   float* params /* n*8 */, uint32_t* info /* n*4, may be NULL */,
                                   uint8_t* inliers /* n*W*H, may be NULL */,
                                   void* workspace, dis_mem where, void* stream, int device);

/* The field of a homography (added within ABI v8, additive; no context):
 * dis_motion_to_flow for n*8 parameters, in f32 with every operation rounded on
 * its own: g = p6*(float)x + p7*(float)y, d = 1.0f + g,
 *   u = (((p0 + p1*(float)x) + p2*(float)y) - (float)x*g) / d,
 *   v = (((p3 + p4*(float)x) + p5*(float)y) - (float)y*g) / d,
 * the divisions correctly rounded. A field with a parameter that is not finite
 * is the canonical NaN everywhere, and so is a pixel whose d is not > 0 (behind
 * the horizon). With p6 = p7 = +0.0f the output is bit for bit
 * dis_motion_to_flow's of p0..p5. Refusals as for dis_motion_to_flow. One launch. */
dis_status dis_homography_to_flow(const float* params /* n*8 */, int n, int width, int height,
                                  void* out, int out_format, dis_mem where, void* stream, int device);

/* Backward warp of u8 images by homographies (added within ABI v8, additive; no
 * context): dis_warp_motion_u8 for n*8 parameters. dst and valid hold, bit for
 * bit, what dis_homography_to_flow(DIS_FLOW_F32) followed by dis_flow_warp_u8
 * writes (a pixel with d not > 0 gets every channel 0 and valid 0); no field
 * exists anywhere. Arguments, strides, borders, valid, refusals and the launch
 * (one, a block per 64 x 16 pixels) as for dis_warp_motion_u8. */
dis_status dis_warp_homography_u8(const uint8_t* src, size_t src_stride, size_t src_image_stride, int channels,
                                  const float* params /* n*8 */, int n, int width, int height, int border,
                                  uint8_t* dst, uint8_t* valid /* may be NULL */,
                                  dis_mem where, void* stream, int device);

/* The camera path of homographies smoothed (added within ABI v8, additive; host
 * only): dis_motion_stabilize with full 3 x 3 matrices; pair_params is
 * (n_frames-1)*8 floats, corrections n_frames*8. All of it f64 with every
 * operation rounded on its own, in this order. A product a.b has the entries
 * (a_i0*b_0j + a_i1*b_1j) + a_i2*b_2j; norm(m) divides each of the nine entries
 * by m22.
 * Pair matrices: A_k = [[1+p1 p2 p0] [p4 1+p5 p3] [p6 p7 1]], each p widened
 * from f32; a model with any non-finite parameter is replaced by the identity,
 * and *replaced counts those models.
 * Path: C_0 = I, C_{k+1} = norm(A_k . C_k).
 * Weights and smoothed path S_k: dis_motion_stabilize's, per entry, for all nine.
 * Inverse, by adjugate and determinant: k00 = s11*s22 - s12*s21, k01 = s10*s22 -
 * s12*s20, k02 = s10*s21 - s11*s20, det = (s00*k00 - s01*k01) + s02*k02; if det
 * is not finite or |det| <= 2^-20, frame k's correction is eight times +0.0f
 * and status[k] = 0. Otherwise the rows of the inverse are
 *   (k00, s02*s21 - s01*s22, s01*s12 - s02*s11) / det,
 *   (s12*s20 - s10*s22, s00*s22 - s02*s20, s02*s10 - s00*s12) / det,
 *   (k02, s01*s20 - s00*s21, s00*s11 - s01*s10) / det, each entry divided on its own.
 * Correction: M_k = norm((C_k . S_k^-1) . Z), Z = [[z 0 cx*(1-z)] [0 z cy*(1-z)]
 * [0 0 1]] as for dis_motion_stabilize; q = (m02, m00-1, m01, m12, m10, m11-1,
 * m20, m21), each value rounded once to f32, a q6 or q7 that compares equal to
 * zero written as +0.0f; status[k] = 1; if any q is not finite the frame falls
 * back to eight times +0.0f and status 0.
 * So identity pair models with zoom 1 give all-zero corrections bit for bit,
 * and affine inputs (p6 = p7 = 0) give q6 = q7 = +0.0f. Refusals as for
 * dis_motion_stabilize; the path needs 72 bytes of host memory a frame. */
dis_status dis_homography_stabilize(const float* pair_params /* (n_frames-1)*8 */, int n_frames,
                                    int width, int height, int radius, float sigma, float zoom,
                                    float* corrections /* n_frames*8 */, uint8_t* status /* n_frames, may be NULL */,
                                    int* replaced /* may be NULL */);

/* Motion-compensated temporal denoising of u8 images (added within ABI v8,
 * additive; no context, like dis_flow_warp_u8; no reference counterpart): each
 * of K neighbouring frames is warped to the current one by its flow and blended
 * in with a per-pixel weight that falls with the photometric difference over a
 * 3 x 3 window.
 *   cur, neighbours[k]: n images of W x H pixels of `channels` (1, 3 or 4)
 *          interleaved u8 samples each; one row stride `stride` and one image
 *          stride `image_stride` in bytes for all (0 = dense), dis_flow_warp_u8's
 *          conventions;
 *   flows[k]: n W x H (u,v) fields, cur -> neighbour k, all F32 or all F16;
 *   masks: NULL, or K entries each of which may be NULL; masks[k] holds n*W*H
 *          bytes, nonzero = the vector is trusted;
 *   weights: 256 floats in [0, 1], always host memory (dis_denoise_weights
 *          makes the Gaussian table; any non-increasing table is as good);
 *   dst:   n dense W x H x channels images; support (may be NULL): n W x H bytes.
 * neighbours, flows and masks are host arrays of K pointers, read during the
 * call; their entries are host or device pointers as `where` says. They and the
 * table reach the kernel by value in its arguments, so the device call
 * allocates nothing, copies nothing and does not synchronise (one launch; it
 * can be captured in a graph). For pixel (x, y) of image i:
 *   1. Wk, Vk = exactly the bytes dis_flow_warp_u8(neighbours[k], flows[k],
 *      scale 1, DIS_BORDER_REPLICATE) writes to dst and valid: an invalid
 *      vector gives 0 / 0, a target outside the frame the clamped sample and 0;
 *   2. ok_k = Vk != 0 && (masks == NULL || masks[k] == NULL || its byte != 0);
 *   3. D_k = the sum of |Wk(x', y', c) - cur(x', y', c)| over x' = x-1..x+1,
 *      y' = y-1..y+1, each clamped to the frame, and all channels c;
 *      idx = (D_k + cnt/2) / cnt in integers with cnt = 9*channels (0..255);
 *   4. w_k = ok_k ? weights[idx] : +0.0f;
 *   5. per channel num = sum over k ascending, from +0.0f, of
 *      w_k * (float)(Wk_c - cur_c) (the difference an exact integer);
 *      sw = the sum of w_k in the same order from +0.0f, den = 1.0f + sw;
 *   6. r = (float)cur_c + num / den; the output byte is rintf(r) (ties to even)
 *      clamped to [0, 255]; support = the number of k with ok_k && w_k > 0.
 * Every f32 operation is separately rounded, integers are exact. So weights
 * all 0 give dst == cur, neighbours equal to cur under zero flows give dst ==
 * cur, and weights all 1 under zero flows give the rounded mean of the K + 1
 * frames. Refused with DIS_ERR_INVALID_ARGUMENT, before any device call:
 * dis_flow_warp_u8's list (a null cur, neighbours, flows, weights or dst; sizes;
 * channels; flow_format; `where`; strides; the grid); k_neighbours outside
 * 1..DIS_DENOISE_MAX_NEIGHBOURS; a null entry of neighbours or flows; a weight
 * that is not finite or lies outside [0, 1]; any overlap of dst or support with
 * cur, a neighbour, a flow, a mask or each other (dst cannot be cur: the window
 * reads cur's surroundings); for DIS_MEM_DEVICE a flow not aligned to one (u,v)
 * pair (8 bytes F32, 4 bytes F16). Image pointers need no alignment (aligned
 * ones and W % 4 == 0 get wider accesses, same bytes). Host pointers:
 * synchronous, staged through HIP device `device`; device pointers:
 * asynchronous on `stream`.
 * dis_denoise_weights (host only, no GPU): table[d] = (float)exp(-((double)d*d)
 * / (2.0*(double)sigma*(double)sigma)), d = 0..255; refuses a null table and a
 * sigma that is not finite or not > 0. */
#define DIS_DENOISE_MAX_NEIGHBOURS 8
dis_status dis_denoise_weights(float sigma, float table[256]);
dis_status dis_temporal_denoise_u8(const uint8_t* cur, const uint8_t* const* neighbours /* K */, size_t stride,
                                   size_t image_stride, int channels,
                                   const void* const* flows /* K: field cur -> neighbour k */, int flow_format,
                                   const uint8_t* const* masks /* NULL, or K entries each of which may be NULL */,
                                   int k_neighbours, int n, int width, int height,
                                   const float* weights /* 256, always host memory */,
                                   uint8_t* dst, uint8_t* support /* may be NULL, n*W*H */,
                                   dis_mem where, void* stream, int device);

/* Middlebury .flo files (src/IO_flow.cpp:10-98): "PIEH", int32 width,
 * int32 height, width*height*channels float32 row-major interleaved,
 * little-endian; channels 1 (depth), 2 (flow) or 4 (scene flow). Host only
 * (no GPU). Reading validates the tag, the size against the buffer and the
 * exact file length. */
dis_status dis_flo_info(const char* path, int* width, int* height);
dis_status dis_read_flo(const char* path, float* data, int width, int height, int channels);
dis_status dis_write_flo(const char* path, const float* data, int width, int height, int channels);

/* Deterministic synthetic pair (SURVEY.md 8d generator): multi-octave value
 * noise I0 and I1 = I0 warped by a smooth sinusoidal flow; optional
 * ground-truth flow (W*H*2). Host memory, host compute; seed k -> pair k. */
dis_status dis_synth_pair(uint64_t seed, int width, int height, uint8_t* I0, uint8_t* I1,
                          float* gt_flow);

#ifdef __cplusplus
}
#endif
#endif /* DIS_ABI_H */
