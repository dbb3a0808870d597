// dis_runtime.hip -- the context of the C-ABI (include/dis_abi.h, struct
// dis_ctx in dis_ctx.h): the error slot, parameter validation, create /
// destroy and the device workspace, every entry point that takes a context
// (the others: dis_flowops.hip, dis_compat.hip), the host-frame pipeline and
// the staged host calls, the debug dumps and kernel timing. The launch
// sequence the calc entry points run is dis_enqueue.hip; geometry and kernel
// arguments are dis_launch_args.hip. Shared with dis_flowops.hip: argument
// rules dis_args.h, staging dis_stage.h, dis_host.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "dis_args.h"
#include "dis_ctx.h"
#include "dis_stage.h"

using dis::pool_mutex;
using dis::run_batches;
using dis::run_batches_graph;
using dis::timing;

static thread_local std::string g_err;

namespace dis {

Timing timing(dis_ctx* c, int kind, int kind2)
{
    Timing t;
    if (!c->timing) return t;
    if (c->pool_next + 2 > c->pool.size()) {  // grow: a record is never dropped
        const size_t n0 = c->pool.size();
        c->pool.resize(n0 + 1024);
        for (size_t i = n0; i < c->pool.size(); ++i)
            if (hipEventCreate(&c->pool[i]) != hipSuccess) {
                c->pool.resize(i);
                c->dropped += 1;
                return t;
            }
    }
    t.start = c->pool[c->pool_next++];
    t.stop = c->pool[c->pool_next++];
    c->recs.push_back({kind, t.start, t.stop});
    if (kind2 >= 0) c->recs.push_back({kind2, t.start, t.stop});
    return t;
}

// error reporting of every translation unit (dis_host.h; dis_io.cpp, dis_plan.cpp)
dis_status set_error(dis_status s, const std::string& msg)
{
    g_err = msg;
    return s;
}

dis_status use_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(DIS_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(DIS_ERR_INVALID_ARGUMENT, "device index out of range");
    DIS_HIP(hipSetDevice(device));
    return DIS_OK;
}

}  // namespace dis

namespace {

dis_status check_params(const dis_params* p, int W, int H)
{
    if (!p) return fail(DIS_ERR_INVALID_ARGUMENT, "params is null");
    if (W < 1 || H < 1) return fail(DIS_ERR_INVALID_ARGUMENT, "width and height must be >= 1");
    if ((long long)W * H > (1LL << 28)) return fail(DIS_ERR_INVALID_ARGUMENT, "frame too large");
    if (p->patch_size < 2 || p->patch_size > 16 || (p->patch_size & 1))
        return fail(DIS_ERR_INVALID_ARGUMENT,
                    "patch_size must be even and in [2,16] (odd sizes are broken in the reference, Q11)");
    if (!(p->patch_overlap >= 0.0f && p->patch_overlap < 1.0f))
        return fail(DIS_ERR_INVALID_ARGUMENT, "patch_overlap must be in [0,1)");
    if (p->finest_scale < 0 || p->coarsest_scale < p->finest_scale)
        return fail(DIS_ERR_INVALID_ARGUMENT, "need 0 <= finest_scale <= coarsest_scale");
    if (p->coarsest_scale >= dis::kMaxLevels - 1)
        return fail(DIS_ERR_INVALID_ARGUMENT, "coarsest_scale too large");
    if (p->iterations < 0) return fail(DIS_ERR_INVALID_ARGUMENT, "iterations must be >= 0");
    if (p->var_refine_iters < 0 || p->var_refine_iters > 64)
        return fail(DIS_ERR_INVALID_ARGUMENT, "var_refine_iters must be in [0, 64]");
    if (p->paper_mode != 0 && p->paper_mode != 1) return fail(DIS_ERR_INVALID_ARGUMENT, "paper_mode must be 0 or 1");
    const int sf = 1 << p->coarsest_scale;
    const int Wp = W + ((W % sf) ? sf - W % sf : 0), Hp = H + ((H % sf) ? sf - H % sf : 0);
    if ((Wp >> p->coarsest_scale) < 1 || (Hp >> p->coarsest_scale) < 1)
        return fail(DIS_ERR_INVALID_ARGUMENT, "frame smaller than 2^coarsest_scale");
    return DIS_OK;
}

void free_ws(dis_ctx* c)
{
    hipFree(c->img0);
    hipFree(c->img1);
    hipFree(c->dx);
    hipFree(c->dy);
    hipFree(c->pu);
    hipFree(c->dense);
    hipFree(c->fb);
    c->fb = nullptr;
    hipFree(c->vr_ws);
    c->vr_ws = nullptr;
    c->hp.reset();
    hipFree(c->stage_in);
    hipFree(c->stage_out);
    hipFree(c->gray);
    c->gray = nullptr;
    c->stage_in = nullptr;
    c->stage_out = nullptr;
    hipFree(c->init);
    c->init = nullptr;
    c->img0 = c->img1 = c->dx = c->dy = nullptr;
    c->pu = c->dense = nullptr;
}

// True when [p, p + bytes) lies in one page-locked host allocation
// (hipHostMalloc / hipHostRegister, e.g. torch's pin_memory): the DMA engines
// read or write it directly, no staging copy.
bool host_pinned(const void* p, size_t bytes)
{
    if (!p || !bytes) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory reports an error here
        return false;
    }
    if (a.type != hipMemoryTypeHost) return false;
    void *b0 = nullptr, *b1 = nullptr;
    const char* last = static_cast<const char*>(p) + bytes - 1;
    if (hipPointerGetAttribute(&b0, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, const_cast<void*>(p)) != hipSuccess ||
        hipPointerGetAttribute(&b1, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, const_cast<char*>(last)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return b0 && b0 == b1;
}

// Device slots, streams and the download thread of the host-frame path, made
// on the first host call (device-resident callers never pay for them).
// chunk = 0: about 64 MB of flow per chunk (4 pairs at 1920 x 1080, 8 of f16
// flow); debug mode keeps the whole batch in one chunk (the stage dumps read
// the last call's pairs). A changed chunk, flow format or frame format
// rebuilds the pipe. Colour frames go up as they are: the device path converts.
dis_status host_pipe_init(dis_ctx* c, int n)
{
    const size_t pixels = (size_t)c->g.W * c->g.H, frame = pixels * c->pixel_bytes();
    int chunk = c->host_chunk > 0 ? c->host_chunk
                                  : (int)std::max<size_t>(1, (size_t(64) << 20) / (pixels * c->vec_bytes()));
    if (c->debug) chunk = std::max(chunk, n);
    chunk = std::min(chunk, c->max_batch);
    if (c->hp && c->hp->chunk == chunk && c->hp->format == c->flow_format && c->hp->frame_format == c->frame_format)
        return DIS_OK;
    c->hp.reset();
    auto hp = std::make_unique<HostPipe>();
    hp->chunk = chunk;
    hp->format = c->flow_format;
    hp->frame_format = c->frame_format;
    hp->frame = frame;
    hp->device = c->device;
    for (int s = 0; s < 2; ++s) {
        if (hipMalloc(&hp->din[s], 2 * frame * chunk) != hipSuccess ||
            hipMalloc(&hp->dout[s], c->vec_bytes() * pixels * chunk) != hipSuccess)
            return fail(DIS_ERR_OUT_OF_MEMORY, "host-path device slot allocation failed");
        DIS_HIP(hipEventCreateWithFlags(&hp->up_done[s], hipEventDisableTiming));
        DIS_HIP(hipEventCreateWithFlags(&hp->comp_done[s], hipEventDisableTiming));
        DIS_HIP(hipEventCreateWithFlags(&hp->down_done[s], hipEventDisableTiming));
    }
    DIS_HIP(hipStreamCreateWithFlags(&hp->up, hipStreamNonBlocking));
    DIS_HIP(hipStreamCreateWithFlags(&hp->down, hipStreamNonBlocking));
    HostPipe* raw = hp.get();
    hp->th = std::thread([raw] { raw->run(); });
    c->hp = std::move(hp);
    return DIS_OK;
}

// dis_calc_batch_u8 on host frames and host flow. Chunk j: the calling thread
// uploads it into device slot j % 2 (once the computation of chunk j-2 has
// read that slot), enqueues its computation -- the device path on the
// context's own stream, after the upload and after the download of chunk j-2
// has read the output slot -- and posts its download to the download thread.
// Pageable copies block the thread that issues them until they are done, so
// the upload of chunk j+1 runs while chunk j computes and chunk j-1
// downloads (PCIe is full duplex); page-locked caller buffers (dis_host_alloc,
// hipHostMalloc / hipHostRegister) make every copy asynchronous. The flows are
// the device path's, bit for bit.
dis_status calc_host(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, size_t stride, size_t pair_stride,
                     float* flow)
{
    dis_status st = host_pipe_init(c, n);
    if (st != DIS_OK) return st;
    HostPipe& P = *c->hp;
    const int H = c->g.H, chunk = P.chunk;
    const size_t W = (size_t)c->g.W * c->pixel_bytes();  // bytes of one row of a frame
    const size_t fr = P.frame, fb = (size_t)c->g.W * H * c->vec_bytes();  // bytes of one frame, of one flow
    const size_t in_span = (size_t)(n - 1) * pair_stride + (size_t)(H - 1) * stride + W;
    const bool pin_in = host_pinned(I0, in_span) && host_pinned(I1, in_span);
    const bool pin_out = host_pinned(flow, fb * n);
    const hipStream_t s = c->own;
    const int nch = (n + chunk - 1) / chunk;
    const long long base = P.posted;  // jobs of earlier calls (all issued and done)
    auto drain = [&](hipError_t e0) -> dis_status {  // after an error: let the download thread finish
        const hipError_t e1 = P.wait_issued(P.posted);
        const hipError_t e = e0 != hipSuccess ? e0 : e1;
        return fail(DIS_ERR_DEVICE, std::string("host-frame path: ") + hipGetErrorString(e));
    };
    for (int j = 0; j < nch; ++j) {
        const int slot = j & 1, a = j * chunk, m = std::min(chunk, n - a);
        uint8_t* din0 = P.din[slot];
        uint8_t* din1 = P.din[slot] + (size_t)chunk * fr;
        hipError_t e = hipSuccess;
        // upload once the computation of chunk j-2 has read the slot
        if (P.comp_pending[slot]) e = hipStreamWaitEvent(P.up, P.comp_done[slot], 0);
        for (int k = 0; e == hipSuccess && k < m; ++k) {
            e = hipMemcpy2DAsync(din0 + k * fr, W, I0 + (size_t)(a + k) * pair_stride, stride, W, H,
                                 hipMemcpyHostToDevice, P.up);
            if (e == hipSuccess)
                e = hipMemcpy2DAsync(din1 + k * fr, W, I1 + (size_t)(a + k) * pair_stride, stride, W, H,
                                     hipMemcpyHostToDevice, P.up);
        }
        if (e == hipSuccess) e = hipEventRecord(P.up_done[slot], P.up);
        // compute after the upload and after the download of chunk j-2 (its
        // job must have been issued for down_done[slot] to stand for it)
        if (e == hipSuccess) e = hipStreamWaitEvent(s, P.up_done[slot], 0);
        if (e == hipSuccess && P.down_pending[slot]) {
            e = P.wait_issued(base + j - 1);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, P.down_done[slot], 0);
        }
        if (e != hipSuccess) return drain(e);
        // eager enqueue, not a replayed graph: this path is bound by PCIe (a
        // chunk's download takes ~10x its computation), and launching a graph
        // captured here crashed the HIP 7.2 runtime on the host in one call
        // sequence (tools/repro_graph_steps.py EKSFH) that the
        // eager form runs cleanly
        {
            std::lock_guard<std::mutex> lock(pool_mutex(c->device));
            st = run_batches(c, m, din0, din1, W, fr, P.dout[slot], s);
        }
        if (st != DIS_OK) {
            drain(hipSuccess);
            return st;
        }
        e = hipEventRecord(P.comp_done[slot], s);
        if (e != hipSuccess) return drain(e);
        P.comp_pending[slot] = true;
        P.down_pending[slot] = true;
        P.post({reinterpret_cast<char*>(flow) + (size_t)a * fb, reinterpret_cast<const char*>(P.dout[slot]), m * fb,
                slot});
    }
    hipError_t e = P.wait_issued(base + nch);
    if (e == hipSuccess) e = hipEventSynchronize(P.down_done[(nch - 1) & 1]);  // page-locked flow: the last copy
    if (e != hipSuccess) return fail(DIS_ERR_DEVICE, std::string("host-frame path: ") + hipGetErrorString(e));
    P.last_chunks = nch;
    P.last_direct_in = pin_in ? 1 : 0;
    P.last_direct_out = pin_out ? 1 : 0;
    return DIS_OK;
}

// The frame arguments of the three batch entry points; resolves the strides.
// What needs no context comes first: checked the same with or without a device.
dis_status check_frames(const dis_ctx* c, int n, const void* I0, const void* I1, const void* flow_a,
                        const void* flow_b, dis_mem where, size_t stride, size_t pair_stride, dis::FrameBatch* fb)
{
    if (!I0 || !I1 || !flow_a || !flow_b) return fail(DIS_ERR_INVALID_ARGUMENT, "null frame or flow pointer");
    if (n < 1) return fail(DIS_ERR_INVALID_ARGUMENT, "n must be in [1, max_batch]");
    if (where != DIS_MEM_HOST && where != DIS_MEM_DEVICE) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    DIS_ARG(dis::check_frame_batch(c->g.W, c->g.H, n, c->max_batch, stride, pair_stride, fb, c->pixel_bytes()));
    return DIS_OK;
}

// A bidirectional or warm-started call on host pointers: synchronous, staged
// through device buffers for max_batch pairs made on the first such call (the
// chunked pipeline of dis_calc_batch_u8 is not used here). The frames go up
// tightly packed, and `up_b` (if any) into the second of two output slots, each
// sized for a batch of float flows and serving either format; `enqueue` runs on
// them on the context's own stream; slot a comes down to `down_a`, b to `down_b`.
template <class Enqueue>
dis_status staged_call(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, const dis::FrameBatch& fb,
                       const void* up_b, size_t up_bytes, void* down_a, void* down_b, size_t down_bytes,
                       Enqueue&& enqueue)
{
    const int H = c->g.H, px = c->pixel_bytes();
    const size_t W = (size_t)c->g.W * px;  // bytes of one row of a frame
    const size_t fpp = (size_t)c->g.W * H, ipp = W * H, B = (size_t)c->max_batch;
    // colour frames go up as they are: sized for 4 bytes per pixel once the
    // format is not gray (these calls are synchronous: nothing is in flight)
    const int want_px = px > 1 ? 4 : 1;
    if (c->stage_in && c->stage_in_px < want_px) {
        hipFree(c->stage_in);
        c->stage_in = nullptr;
    }
    if (!c->stage_in) {
        if (hipMalloc(&c->stage_in, 2 * fpp * want_px * B) != hipSuccess) {
            (void)hipGetLastError();
            c->stage_in = nullptr;
            return fail(DIS_ERR_OUT_OF_MEMORY, "host-path device buffer allocation failed");
        }
        c->stage_in_px = want_px;
    }
    if (!c->stage_out && hipMalloc(&c->stage_out, 2 * sizeof(float2) * fpp * B) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DIS_ERR_OUT_OF_MEMORY, "host-path device buffer allocation failed");
    }
    const hipStream_t s = c->own;
    uint8_t *const d0 = c->stage_in, *const d1 = d0 + ipp * B;
    float2 *const da = c->stage_out, *const db = da + fpp * B;
    for (int k = 0; k < n; ++k) {
        DIS_HIP(hipMemcpy2DAsync(d0 + k * ipp, W, I0 + k * fb.pair_stride, fb.stride, W, H, hipMemcpyHostToDevice, s));
        DIS_HIP(hipMemcpy2DAsync(d1 + k * ipp, W, I1 + k * fb.pair_stride, fb.stride, W, H, hipMemcpyHostToDevice, s));
    }
    if (up_b) DIS_HIP(hipMemcpyAsync(db, up_b, up_bytes, hipMemcpyHostToDevice, s));
    const dis_status st = enqueue(d0, d1, W, ipp, da, db, s);
    if (st != DIS_OK) {
        (void)hipStreamSynchronize(s);
        return st;
    }
    DIS_HIP(hipMemcpyAsync(down_a, da, down_bytes, hipMemcpyDeviceToHost, s));
    if (down_b) DIS_HIP(hipMemcpyAsync(down_b, db, down_bytes, hipMemcpyDeviceToHost, s));
    DIS_HIP(hipStreamSynchronize(s));
    return DIS_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// exported C-ABI
// ---------------------------------------------------------------------------
extern "C" {

int dis_abi_version(void) { return DIS_ABI_VERSION; }
const char* dis_build_kind(void) { return "product"; }

const char* dis_last_error(void) { return g_err.c_str(); }

dis_status dis_preset_params(dis_preset preset, int width, int height, dis_params* out)
{
    if (!out) return fail(DIS_ERR_INVALID_ARGUMENT, "out is null");
    if (width < 1 || height < 1) return fail(DIS_ERR_INVALID_ARGUMENT, "width and height must be >= 1");
    dis_params p{};
    p.patch_size = 8;
    p.patch_normalization = 1;
    p.var_refine_iters = 0;
    switch (preset) {
        case DIS_PRESET_ULTRAFAST: p.patch_overlap = 0.5f; p.iterations = 12; p.finest_scale = 2; break;
        case DIS_PRESET_FAST: p.patch_overlap = 0.5f; p.iterations = 16; p.finest_scale = 2; break;
        case DIS_PRESET_MEDIUM: p.patch_overlap = 0.625f; p.iterations = 25; p.finest_scale = 1; break;
        case DIS_PRESET_SLOW:  // + variational refinement (BASELINE config 5; not in the reference)
            p.patch_overlap = 0.75f; p.iterations = 128; p.finest_scale = 0; p.var_refine_iters = 3; break;
        case DIS_PRESET_REFERENCE:
            // CLI defaults, src/main.cpp:66-71
            p.patch_overlap = 0.7f; p.iterations = 1000; p.finest_scale = 0; p.coarsest_scale = 3;
            *out = p;
            return DIS_OK;
        default: return fail(DIS_ERR_INVALID_ARGUMENT, "unknown preset");
    }
    // C = auto: integer division in min(W,H)/ps
    const int mx = std::max(width, height), mn = std::min(width, height);
    int c1 = (int)(std::log2((double)mx / (4.0 * p.patch_size)) + 0.5);
    int c2 = (mn / p.patch_size) > 0 ? (int)std::log2((double)(mn / p.patch_size)) : 0;
    int C = std::max(0, std::min(c1, c2));
    p.coarsest_scale = C;
    p.finest_scale = std::min(p.finest_scale, C);
    *out = p;
    return DIS_OK;
}

dis_status dis_validate_params(const dis_params* params, int width, int height)
{
    return check_params(params, width, height);
}

dis_status dis_workload_info(const dis_params* params, int width, int height, dis_workload* out)
{
    dis_status st = check_params(params, width, height);
    if (st != DIS_OK) return st;
    if (!out) return fail(DIS_ERR_INVALID_ARGUMENT, "out is null");
    dis::Geometry g;
    if (!dis::make_geometry(*params, width, height, &g)) return fail(DIS_ERR_INVALID_ARGUMENT, "bad geometry");
    // SURVEY.md 8d fixed formula
    double B = 2.0 * width * height;
    long long patches = 0, updates = 0;
    for (int l = 0; l <= g.C; ++l) B += 8.0 * g.lv[l].W * g.lv[l].H;
    for (int l = g.F; l <= g.C; ++l) {
        const double px = (double)g.lv[l].W * g.lv[l].H;
        B += 8.0 * px;                               // frame-0 dx, dy
        B += 16.0 * px + 16.0 * g.lv[l].n + 8.0 * px;  // search reads + u + dense write
        patches += g.lv[l].n;
        updates += (long long)g.lv[l].n * (g.iters + 1);
    }
    for (int l = g.F; l < g.C; ++l) B += 8.0 * g.lv[l + 1].W * g.lv[l + 1].H;
    if (g.F > 0) B += 8.0 * g.lv[g.F].W * g.lv[g.F].H + 8.0 * width * height;
    out->padded_width = g.Wp;
    out->padded_height = g.Hp;
    out->steps = g.steps;
    out->patches = patches;
    out->updates = updates;
    out->algorithmic_bytes = B;
    const dis::LevelGeom& LF = g.lv[g.F];
    out->search_bytes_finest = 16.0 * LF.W * LF.H + 16.0 * LF.n;
    double sb = 0.0;
    for (int l = g.F; l <= g.C; ++l) {
        sb += 16.0 * g.lv[l].W * g.lv[l].H + 16.0 * g.lv[l].n;
        if (l < g.C) sb += 8.0 * g.lv[l + 1].W * g.lv[l + 1].H;
    }
    out->search_bytes_all = sb;
    out->search_launches = g.C - g.F + 1;
    // algorithmic f32 operations per patch (each add/sub/mul/div = 1): Sobel
    // gradients ~10/pixel, Hessian 3 dot products, 2x2 LU; per update: bilinear
    // warp 7/pixel (4 mul + 3 add), mean normalisation 2/pixel, 2 dot products,
    // solve + update + outlier test ~12 (src/patch.cpp:31-267)
    const double N = (double)g.ps * g.ps;
    const double per_update = 7.0 * N + (g.norm ? 2.0 * N : 0.0) + 2.0 * (2.0 * N - 1.0) + 14.0;
    const double per_patch = 10.0 * N + 3.0 * (2.0 * N - 1.0) + 6.0 + (g.iters + 1) * per_update;
    out->patches_finest = LF.n;
    out->search_flops_finest = (double)LF.n * per_patch;
    return DIS_OK;
}

dis_status dis_create(dis_ctx** out, const dis_params* params, int width, int height, int max_batch,
                      int device)
{
    if (!out) return fail(DIS_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    dis_status st = check_params(params, width, height);
    if (st != DIS_OK) return st;
    if (max_batch < 1) return fail(DIS_ERR_INVALID_ARGUMENT, "max_batch must be >= 1");
    if (dis_status ds = dis::use_device(device)) return ds;
    dis_ctx* c = new (std::nothrow) dis_ctx();
    if (!c) return fail(DIS_ERR_OUT_OF_MEMORY, "host allocation failed");
    c->p = *params;
    c->device = device;
    c->max_batch = max_batch;
    if (!dis::make_geometry(*params, width, height, &c->g)) {
        delete c;
        return fail(DIS_ERR_INVALID_ARGUMENT, "bad geometry");
    }
    const dis::Geometry& g = c->g;
    c->k = dis::launch_consts(g, params->paper_mode);
    const size_t B = (size_t)max_batch;
    const size_t plane = sizeof(float) * (size_t)g.plane_stride * B;
    bool ok = hipMalloc(&c->img0, plane) == hipSuccess && hipMalloc(&c->img1, plane) == hipSuccess &&
              hipMalloc(&c->dx, plane) == hipSuccess && hipMalloc(&c->dy, plane) == hipSuccess &&
              hipMalloc(&c->pu, sizeof(float2) * (size_t)g.u_stride * B) == hipSuccess &&
              hipMalloc(&c->dense, sizeof(float2) * (size_t)g.dense_stride * B) == hipSuccess &&
              hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&c->done, hipEventDisableTiming) == hipSuccess;
    if (ok) {
        size_t off = (size_t)dis_ctx::kMaxSub * kFbCounters;
        for (int k = 0; k < dis_ctx::kMaxSub; ++k)
            for (int l = 0; l <= g.C; ++l) {
                c->fb_list_off[k][l] = off;
                off += dis::fb_list_blocks(g.lv[l]) * B;
            }
        ok = hipMalloc(&c->fb, sizeof(int) * off) == hipSuccess &&
             hipMemset(c->fb, 0, sizeof(int) * dis_ctx::kMaxSub * kFbCounters) == hipSuccess;
    }
    if (ok) {  // warm start: the init planes (a few KB)
        dis::init_plane_size(g, &c->iw, &c->ih);
        ok = hipMalloc(&c->init, sizeof(float2) * (size_t)c->iw * c->ih * B) == hipSuccess;
    }
    if (ok && params->var_refine_iters > 0) {
        c->vr_plane = (long long)g.lv[g.F].W * g.lv[g.F].H;  // the largest refined level
        ok = hipMalloc(&c->vr_ws, sizeof(float) * dis::kVarRefPlanes * c->vr_plane * B) == hipSuccess;
    }
    ok = ok && dis::sub_streams(device, c->sub);
    for (int k = 0; ok && k < dis_ctx::kMaxSub; ++k)
        ok = hipEventCreateWithFlags(&c->join[k], hipEventDisableTiming) == hipSuccess;
    // The capture-only stream exists only under refinement and is created last:
    // HIP assigns streams to its (GPU_MAX_HW_QUEUES = 4) hardware queues round
    // robin at creation, and an extra stream created before sub[] shifted
    // sub[1] onto the caller's (null stream's) queue, serialising the two
    // sub-batches (measured: 20.1k -> 15.5k pairs/s at 1080p MEDIUM).
    if (ok) ok = hipStreamCreateWithFlags(&c->cap, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        dis_destroy(c);  // (whatever was made so far)
        return fail(DIS_ERR_OUT_OF_MEMORY, "device workspace allocation failed");
    }
    *out = c;
    return DIS_OK;
}

dis_status dis_destroy(dis_ctx* c)
{
    if (!c) return DIS_OK;
    hipSetDevice(c->device);
    if (c->own) hipStreamSynchronize(c->own);
    if (c->done_pending) hipEventSynchronize(c->done);  // the last call, on whatever stream it ran
    for (int k = 0; k < dis_ctx::kMaxSub; ++k)  // the streams are shared (process pool): wait for this
        if (c->join[k]) hipEventSynchronize(c->join[k]);  // context's last join, not the stream
    free_ws(c);
    for (hipEvent_t e : c->pool) hipEventDestroy(e);
    for (int k = 0; k < dis_ctx::kMaxSub; ++k)
        if (c->join[k]) hipEventDestroy(c->join[k]);
    if (c->fork) hipEventDestroy(c->fork);
    if (c->done) hipEventDestroy(c->done);
    for (auto& d : c->vrg)
        for (auto& row : d)
            for (auto& G : row)
                if (G.exec) hipGraphExecDestroy(G.exec);
    for (auto& G : c->mg) {
        if (G.exec) hipGraphExecDestroy(G.exec);
        if (G.last) hipEventDestroy(G.last);
    }
    if (c->cap) hipStreamDestroy(c->cap);
    if (c->own) hipStreamDestroy(c->own);
    delete c;
    return DIS_OK;
}

dis_status dis_calc_batch_u8(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, size_t stride,
                             size_t pair_stride, float* flow, dis_mem where, void* stream)
{
    dis::FrameBatch fb;
    if (dis_status st = check_frames(c, n, I0, I1, flow, flow, where, stride, pair_stride, &fb)) return st;
    if (where == DIS_MEM_DEVICE && c->f16() && (reinterpret_cast<uintptr_t>(flow) & 3))
        return fail(DIS_ERR_INVALID_ARGUMENT, "DIS_FLOW_F16: flow must be 4-byte aligned");
    DIS_HIP(hipSetDevice(c->device));
    if (where == DIS_MEM_DEVICE) {
        return run_batches_graph(c, n, I0, I1, fb.stride, fb.pair_stride, reinterpret_cast<float2*>(flow),
                                 reinterpret_cast<hipStream_t>(stream));
    }
    return calc_host(c, n, I0, I1, fb.stride, fb.pair_stride, flow);
}

// Both directions in one call: always the eager enqueue (never the main graph
// cache, whose key and captured arguments know one direction only). After it,
// DIS_STAGE_FALLBACK and the debug dumps describe the backward pass.
dis_status dis_calc_bidir_batch_u8(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, size_t stride,
                                   size_t pair_stride, float* flow_fw, float* flow_bw, dis_mem where, void* stream)
{
    dis::FrameBatch fb;  // (what needs no context is refused first, this call's own such rule included)
    if (flow_fw && flow_fw == flow_bw) return fail(DIS_ERR_INVALID_ARGUMENT, "flow_fw and flow_bw overlap");
    if (dis_status st = check_frames(c, n, I0, I1, flow_fw, flow_bw, where, stride, pair_stride, &fb)) return st;
    const size_t fpp = (size_t)c->g.W * c->g.H;  // (u, v) vectors per pair
    const size_t fbytes = c->vec_bytes() * fpp * (size_t)n;  // in the context's flow format
    const dis::NamedRange out[2] = {{reinterpret_cast<uintptr_t>(flow_fw), fbytes, "flow_fw"},
                                    {reinterpret_cast<uintptr_t>(flow_bw), fbytes, "flow_bw"}};
    dis::PairMessage why;
    DIS_ARG(dis::check_disjoint(out, 0, 2, &why));
    if (where == DIS_MEM_DEVICE && c->f16() && ((out[0].p | out[1].p) & 3))
        return fail(DIS_ERR_INVALID_ARGUMENT, "DIS_FLOW_F16: flow_fw and flow_bw must be 4-byte aligned");
    DIS_HIP(hipSetDevice(c->device));
    auto enqueue = [&](const uint8_t* f0, const uint8_t* f1, size_t st, size_t pst, float2* fw, float2* bw,
                       hipStream_t s) {
        std::lock_guard<std::mutex> lock(pool_mutex(c->device));  // eager enqueue onto the pooled streams
        return run_batches(c, n, f0, f1, st, pst, fw, s, false, bw);
    };
    if (where == DIS_MEM_DEVICE)
        return enqueue(I0, I1, fb.stride, fb.pair_stride, reinterpret_cast<float2*>(flow_fw),
                       reinterpret_cast<float2*>(flow_bw), reinterpret_cast<hipStream_t>(stream));
    return staged_call(c, n, I0, I1, fb, nullptr, 0, flow_fw, flow_bw, fbytes, enqueue);
}

dis_status dis_init_plane_size(dis_ctx* c, int* iw, int* ih)
{
    if (!c || !iw || !ih) return fail(DIS_ERR_INVALID_ARGUMENT, "null argument");
    *iw = c->iw;
    *ih = c->ih;
    return DIS_OK;
}

// The reduction alone, into the caller's planes (no context workspace is
// touched: nothing to order against the context's other calls).
dis_status dis_flow_to_init(dis_ctx* c, int n, const float* flow, float* init_planes, dis_mem where, void* stream)
{
    if (!flow || !init_planes) return fail(DIS_ERR_INVALID_ARGUMENT, "null flow or init_planes pointer");
    if (n < 1 || n > 65535) return fail(DIS_ERR_INVALID_ARGUMENT, "n must be in [1, 65535]");
    if (where != DIS_MEM_HOST && where != DIS_MEM_DEVICE) return fail(DIS_ERR_INVALID_ARGUMENT, "bad dis_mem");
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    if (where == DIS_MEM_DEVICE &&
        (reinterpret_cast<uintptr_t>(flow) & (c->f16() ? 3 : 7) || reinterpret_cast<uintptr_t>(init_planes) & 7))
        return fail(DIS_ERR_INVALID_ARGUMENT, "flow and init_planes must be 8-byte aligned (a DIS_FLOW_F16 flow: 4-byte)");
    DIS_HIP(hipSetDevice(c->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t fbytes = c->vec_bytes() * (size_t)c->g.W * c->g.H * n;  // in the context's flow format
    const size_t pbytes = sizeof(float2) * (size_t)c->iw * c->ih * n;
    dis::HostStage st(s, where == DIS_MEM_HOST);
    const float* dflow = st.in(flow, fbytes);
    float* dplanes = st.out(init_planes, pbytes);
    return st.finish([&] { return dis::launch_flow_to_init(dflow, dplanes, n, c->g, s, {}, c->f16()); },
                     "flow to init plane reduction");
}

// Warm start: fill the context's init planes from `init` (the reduction or the
// sanitising copy), then the plain level chain with the coarsest level reading
// them. Always the eager enqueue: the main graph cache's key and captured
// arguments know nothing of an init buffer, and a video loop hands over a
// different (or the just-written) buffer every call.
dis_status dis_calc_batch_init_u8(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, size_t stride,
                                  size_t pair_stride, const float* init, int init_kind, float* flow, dis_mem where,
                                  void* stream)
{
    if (!init) return dis_calc_batch_u8(c, n, I0, I1, stride, pair_stride, flow, where, stream);
    dis::FrameBatch fb;  // (what needs no context is refused first, this call's own such rule included)
    if (init_kind != DIS_INIT_COARSE && init_kind != DIS_INIT_FULLRES)
        return fail(DIS_ERR_INVALID_ARGUMENT, "init_kind must be DIS_INIT_COARSE or DIS_INIT_FULLRES");
    if (dis_status st = check_frames(c, n, I0, I1, flow, flow, where, stride, pair_stride, &fb)) return st;
    const size_t fpp = (size_t)c->g.W * c->g.H;       // (u, v) vectors per flow
    const size_t ipp = (size_t)c->iw * c->ih;         // float2 per init plane (ipp <= fpp: never larger than a flow)
    const size_t fbytes = c->vec_bytes() * fpp * (size_t)n;  // in the context's flow format (FULLRES init too)
    const size_t ibytes = init_kind == DIS_INIT_FULLRES ? fbytes : sizeof(float2) * ipp * (size_t)n;
    DIS_ARG(dis::check_init_aliasing(reinterpret_cast<uintptr_t>(init), ibytes, reinterpret_cast<uintptr_t>(flow),
                                     fbytes, reinterpret_cast<uintptr_t>(I0), reinterpret_cast<uintptr_t>(I1),
                                     fb.bytes));
    const bool init_f16 = c->f16() && init_kind == DIS_INIT_FULLRES;
    if (where == DIS_MEM_DEVICE && (reinterpret_cast<uintptr_t>(init) & (init_f16 ? 3 : 7)))
        return fail(DIS_ERR_INVALID_ARGUMENT, "init must be 8-byte aligned (a DIS_FLOW_F16 flow: 4-byte)");
    if (where == DIS_MEM_DEVICE && c->f16() && (reinterpret_cast<uintptr_t>(flow) & 3))
        return fail(DIS_ERR_INVALID_ARGUMENT, "DIS_FLOW_F16: flow must be 4-byte aligned");
    DIS_HIP(hipSetDevice(c->device));
    // Fill the planes on `s`, then run the chain on `s`: every sub-batch stream
    // forks from `s` after the fill, so the planes are complete -- and `init`
    // has been read to the end -- before any kernel of the chain starts, the
    // one that writes `flow` included. That is what lets init be flow.
    auto enqueue = [&](const uint8_t* f0, const uint8_t* f1, size_t st, size_t pst, float2* out, const void* init_in,
                       hipStream_t s) -> dis_status {
        const float* in = static_cast<const float*>(init_in);
        if (c->needs_wait(s)) DIS_HIP(hipStreamWaitEvent(s, c->done, 0));  // the planes are workspace
        if (init_kind == DIS_INIT_FULLRES)
            DIS_HIP(dis::launch_flow_to_init(in, reinterpret_cast<float*>(c->init), n, c->g, s, timing(c, 6),
                                             c->f16()));
        else
            DIS_HIP(dis::launch_init_copy(in, reinterpret_cast<float*>(c->init), (long long)(2 * ipp) * n, s,
                                          timing(c, 6)));
        std::lock_guard<std::mutex> lock(pool_mutex(c->device));  // eager enqueue onto the pooled streams
        c->warm = true;
        const dis_status r = run_batches(c, n, f0, f1, st, pst, out, s);
        c->warm = false;
        return r;
    };
    if (where == DIS_MEM_DEVICE)
        return enqueue(I0, I1, fb.stride, fb.pair_stride, reinterpret_cast<float2*>(flow), init,
                       reinterpret_cast<hipStream_t>(stream));
    return staged_call(c, n, I0, I1, fb, init, ibytes, flow, nullptr, fbytes, enqueue);
}

dis_status dis_set_host_pipeline(dis_ctx* c, int chunk_pairs)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    if (chunk_pairs < 0) return fail(DIS_ERR_INVALID_ARGUMENT, "chunk_pairs must be >= 0 (0 = auto)");
    DIS_HIP(hipSetDevice(c->device));
    c->hp.reset();  // rebuilt on the next host call (host calls are synchronous: nothing in flight)
    c->host_chunk = chunk_pairs;
    return DIS_OK;
}

dis_status dis_host_pipeline_info(dis_ctx* c, dis_host_info* out)
{
    if (!c || !out) return fail(DIS_ERR_INVALID_ARGUMENT, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (c->hp) {
        out->chunk_pairs = c->hp->chunk;
        out->last_chunks = c->hp->last_chunks;
        out->last_direct_in = c->hp->last_direct_in;
        out->last_direct_out = c->hp->last_direct_out;
    }
    return DIS_OK;
}

dis_status dis_host_alloc(size_t bytes, void** out)
{
    if (!out) return fail(DIS_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (!bytes) return fail(DIS_ERR_INVALID_ARGUMENT, "bytes must be > 0");
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return fail(DIS_ERR_OUT_OF_MEMORY, "page-locked host allocation failed");
    }
    return DIS_OK;
}

dis_status dis_host_free(void* p)
{
    if (p && hipHostFree(p) != hipSuccess) return fail(DIS_ERR_INVALID_ARGUMENT, "not a dis_host_alloc pointer");
    return DIS_OK;
}

dis_status dis_calc_u8(dis_ctx* c, const uint8_t* I0, const uint8_t* I1, size_t stride, float* flow,
                       dis_mem where, void* stream)
{
    return dis_calc_batch_u8(c, 1, I0, I1, stride, 0, flow, where, stream);
}

dis_status dis_set_debug(dis_ctx* c, int enable)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    c->debug = enable ? 1 : 0;  // this build always materialises every stage
    return DIS_OK;
}

dis_status dis_set_concurrency(dis_ctx* c, int streams)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    if (streams < 1 || streams > dis_ctx::kMaxSub)
        return fail(DIS_ERR_INVALID_ARGUMENT, "streams must be in [1, 8]");
    c->nsub = streams;
    return DIS_OK;
}

dis_status dis_set_graphs(dis_ctx* c, int enable)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    c->graphs = enable ? 1 : 0;
    return DIS_OK;
}

dis_status dis_set_precision(dis_ctx* c, int mode)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    if (mode != DIS_PRECISION_EXACT && mode != DIS_PRECISION_FMA)
        return fail(DIS_ERR_INVALID_ARGUMENT, "precision must be DIS_PRECISION_EXACT or DIS_PRECISION_FMA");
    c->precision = mode;
    return DIS_OK;
}

dis_status dis_set_flow_format(dis_ctx* c, int format)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    if (format != DIS_FLOW_F32 && format != DIS_FLOW_F16)
        return fail(DIS_ERR_INVALID_ARGUMENT, "format must be DIS_FLOW_F32 or DIS_FLOW_F16");
    // (the host pipeline's slots and the graph cache follow at the next call:
    // both compare the format they were made for)
    c->flow_format = format;
    return DIS_OK;
}

// The gray buffer is made here, on the first colour format, never inside a calc
// call; it stays when the format goes back to gray (dis_destroy frees it).
dis_status dis_set_frame_format(dis_ctx* c, int format)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!dis::frame_format_channels(format))
        return fail(DIS_ERR_INVALID_ARGUMENT, "format must be a dis_frame_format (DIS_FRAME_GRAY8 .. DIS_FRAME_RGBA8)");
    if (format != DIS_FRAME_GRAY8 && !c->gray) {
        DIS_HIP(hipSetDevice(c->device));
        if (hipMalloc(&c->gray, 2 * c->gray_stride() * c->g.H * (size_t)c->max_batch) != hipSuccess) {
            (void)hipGetLastError();
            c->gray = nullptr;
            return fail(DIS_ERR_OUT_OF_MEMORY, "gray staging buffer allocation failed (the frame format is unchanged)");
        }
    }
    // (the host pipeline's slots and the graph cache follow at the next call:
    // both compare the format they were made for)
    c->frame_format = format;
    return DIS_OK;
}

dis_status dis_set_kernel_variant(dis_ctx* c, int variant)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    if (variant < 0 || variant > 9 || variant == 7 || variant == 8)
        return fail(DIS_ERR_INVALID_ARGUMENT, "variant must be 0..6 or 9 (7 and 8 were removed in ABI v7)");
    c->variant = variant;
    return DIS_OK;
}

dis_status dis_stage_size(dis_ctx* c, int stage, int level, size_t* count)
{
    if (!c || !count) return fail(DIS_ERR_INVALID_ARGUMENT, "null argument");
    const dis::Geometry& g = c->g;
    if (level < 0 || level > g.C) return fail(DIS_ERR_INVALID_ARGUMENT, "level out of range");
    const dis::LevelGeom& L = g.lv[level];
    switch (stage) {
        case DIS_STAGE_IMG0:
        case DIS_STAGE_IMG1:
        case DIS_STAGE_DX0:
        case DIS_STAGE_DY0: *count = (size_t)L.W * L.H; return DIS_OK;
        case DIS_STAGE_PATCH_U: *count = (size_t)L.n * 2; return DIS_OK;
        case DIS_STAGE_DENSE: *count = (size_t)L.W * L.H * 2; return DIS_OK;
        case DIS_STAGE_FALLBACK: *count = 1; return DIS_OK;
        default: return fail(DIS_ERR_INVALID_ARGUMENT, "unknown stage");
    }
}

dis_status dis_debug_dump(dis_ctx* c, int stage, int level, int pair, float* dst, size_t count)
{
    size_t need = 0;
    dis_status st = dis_stage_size(c, stage, level, &need);
    if (st != DIS_OK) return st;
    if (!dst || count < need) return fail(DIS_ERR_INVALID_ARGUMENT, "dst null or too small");
    if (pair < 0 || pair >= c->last_batch) return fail(DIS_ERR_INVALID_ARGUMENT, "pair not in last batch");
    const dis::Geometry& g = c->g;
    const dis::LevelGeom& L = g.lv[level];
    if ((stage == DIS_STAGE_DX0 || stage == DIS_STAGE_DY0 || stage == DIS_STAGE_PATCH_U ||
         stage == DIS_STAGE_DENSE) && level < g.F)
        return fail(DIS_ERR_INVALID_ARGUMENT, "stage not computed below finest_scale");
    DIS_HIP(hipSetDevice(c->device));
    DIS_HIP(hipDeviceSynchronize());
    if (stage == DIS_STAGE_FALLBACK) {  // blocks the level's tile search listed for k_search8_fb, all sub-batches
        std::vector<int> cnt((size_t)c->last_nsub);
        for (int k = 0; k < c->last_nsub; ++k)
            DIS_HIP(hipMemcpy(&cnt[k], c->fb + (size_t)k * kFbCounters + level, sizeof(int), hipMemcpyDeviceToHost));
        long long t = 0;
        for (int v : cnt) t += v;
        *dst = (float)t;
        return DIS_OK;
    }
    const void* src = nullptr;
    switch (stage) {
        case DIS_STAGE_IMG0: src = c->img0 + pair * g.plane_stride + L.plane_off; break;
        case DIS_STAGE_IMG1: src = c->img1 + pair * g.plane_stride + L.plane_off; break;
        case DIS_STAGE_DX0: src = c->dx + pair * g.plane_stride + L.plane_off; break;
        case DIS_STAGE_DY0: src = c->dy + pair * g.plane_stride + L.plane_off; break;
        case DIS_STAGE_PATCH_U: src = c->pu + pair * g.u_stride + L.u_off; break;
        case DIS_STAGE_DENSE: src = c->dense + pair * g.dense_stride + L.dense_off; break;
    }
    DIS_HIP(hipMemcpy(dst, src, sizeof(float) * need, hipMemcpyDeviceToHost));
    return DIS_OK;
}

dis_status dis_set_kernel_timing(dis_ctx* c, int enable)
{
    if (!c) return fail(DIS_ERR_INVALID_ARGUMENT, "ctx is null");
    DIS_HIP(hipSetDevice(c->device));
    if (enable && c->pool.empty()) {
        c->pool.resize(8192);
        for (auto& e : c->pool) DIS_HIP(hipEventCreate(&e));
    }
    if (enable && !c->timing) {  // (re)enabling starts a fresh measurement
        for (auto& r : c->recs) DIS_HIP(hipEventSynchronize(r.b));
        c->recs.clear();
        c->pool_next = 0;
        for (int k = 0; k < dis_ctx::kKinds; ++k) {
            c->launches[k] = 0;
            c->total_ms[k] = 0.0;
        }
        c->dropped = 0;
    }
    c->timing = enable ? 1 : 0;
    return DIS_OK;
}

dis_status dis_kernel_time(dis_ctx* c, int kernel, int* launches, double* total_ms)
{
    if (!c || kernel < 0 || kernel >= dis_ctx::kKinds) return fail(DIS_ERR_INVALID_ARGUMENT, "bad argument");
    DIS_HIP(hipSetDevice(c->device));
    for (auto& r : c->recs) {
        DIS_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        DIS_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        if (r.kind >= 0 && r.kind < dis_ctx::kKinds) {
            c->launches[r.kind] += 1;
            c->total_ms[r.kind] += ms;
        }
    }
    c->recs.clear();
    c->pool_next = 0;
    if (c->dropped) return fail(DIS_ERR_DEVICE, "kernel timing records were dropped (event creation failed)");
    if (launches) *launches = c->launches[kernel];
    if (total_ms) *total_ms = c->total_ms[kernel];
    return DIS_OK;
}

}  // extern "C"
