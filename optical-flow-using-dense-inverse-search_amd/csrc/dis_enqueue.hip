// dis_enqueue.hip -- the launch sequence of a context (dis_ctx.h): the four
// stages of one sub-batch, the split of a batch call over the sub-batch
// streams, and the call replayed as a HIP graph. Kernel arguments come from
// the builders of dis_launch_args.h; what depends on the call is set here.
//
// The sequence is the reference's control flow restated for a batch of pairs
// resident in HBM: src/main.cpp:135-198 (pad/convert, pyramid, upsample, crop)
// around src/optical_flow.cpp:67-91 (coarse-to-fine scale loop).
#include <algorithm>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <dlfcn.h>

#include "dis_ctx.h"
#include "dis_plan.h"

namespace dis {

void set_search8_lanes(Search8Args* b, int lanes)
{
    if (lanes == 1 && !search8_lpp1_fits(b->steps)) lanes = 2;
    b->lanes_per_patch = lanes;
    b->tile_stride = search8_tile_stride(b->steps, lanes);
    b->quad = search8_tile_quad(b->steps, lanes);
}

namespace {

constexpr int kStageFront = 1000, kStageBack = -1000;  // other stages: the level index
// between the two passes of a bidirectional call: what the front stage did for
// frame 0's role, redone for frame 1 (fallback counts, generic-path gradients)
constexpr int kStageTurn = 2000;

// roctx markers, resolved at first use with dlopen (no link-time dependency:
// without the roctx library, or without a tool attached, they are no-ops).
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("/opt/rocm/lib/librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
const Roctx& roctx()
{
    static const Roctx r;
    return r;
}

// roctx range around the host-side enqueue of one stage of one sub-batch
// ("dis: level 3 sub 1"), or of a call phase: visible in rocprofv3
// --marker-trace timelines.
struct StageRange {
    StageRange(int stage, int sub)
    {
        char b[48];
        if (stage == kStageFront)
            std::snprintf(b, sizeof b, "dis: pyramid sub %d", sub);
        else if (stage == kStageBack)
            std::snprintf(b, sizeof b, "dis: output sub %d", sub);
        else if (stage == kStageTurn)
            std::snprintf(b, sizeof b, "dis: turn sub %d", sub);
        else
            std::snprintf(b, sizeof b, "dis: level %d sub %d", stage, sub);
        if (roctx().push) roctx().push(b);
    }
    explicit StageRange(const char* what)
    {
        if (roctx().push) roctx().push(what);
    }
    ~StageRange()
    {
        if (roctx().pop) roctx().pop();
    }
    StageRange(const StageRange&) = delete;
    StageRange& operator=(const StageRange&) = delete;
};

// One sub-batch of a batch call: pairs p0 .. p0+n-1 of the workspace on stream
// s. dir = 1 is the backward pass of a bidirectional call: the same stages
// with the two frames' planes swapped (the pyramid builds both frames alike;
// everything after it reads them through P.img0 / P.img1), after a turn stage.
struct SubBatch {
    int sub, n, p0;
    Planes P;
    hipStream_t s;
    int dir;
    int* fb_count;  // this sub-batch's fallback counts (one per level)
};

SubBatch sub_batch(const dis_ctx* c, int sub, int n, int p0, hipStream_t s, int dir)
{
    return {sub, n, p0, context_planes(c->g, p0, dir ? c->img1 : c->img0, dir ? c->img0 : c->img1, c->dx, c->dy, c->pu,
                                       c->dense),
            s, dir, c->fb + (size_t)sub * kFbCounters};
}

// the search every level runs: the patch_size-8 kernels unless variant 1 asks for the generic one
bool fast_search(const dis_ctx* c) { return c->g.ps == 8 && c->variant != 1; }

// frame 0's gradient planes of every level, for the generic search and the debug dumps
dis_status enqueue_sobel(const dis_ctx* c, const SubBatch& v)
{
    for (int l = c->g.F; l <= c->g.C; ++l) DIS_HIP(launch_sobel(c->g, l, v.P.img0, v.P.dx, v.P.dy, v.n, v.s));
    return DIS_OK;
}

// The front end: colour frames to gray, then the pyramid of both frames.
dis_status enqueue_front(dis_ctx* c, const SubBatch& v, const uint8_t* I0, const uint8_t* I1, size_t stride,
                         size_t pair_stride)
{
    const Geometry& g = c->g;
    const bool fast = fast_search(c);
    if (v.dir != 0) return fail(DIS_ERR_INTERNAL, "the front stage runs once, in the forward direction");
    if (c->frame_format != DIS_FRAME_GRAY8) {
        // colour frames: one luma launch for both frames of this sub-batch's
        // pairs into its slice of the gray buffer, which everything below
        // reads in the caller's frames' place (both directions of a
        // bidirectional call: the front stage runs once)
        const size_t gs = c->gray_stride(), gi = gs * g.H;
        uint8_t* const g0 = c->gray + (size_t)v.p0 * gi;
        uint8_t* const g1 = c->gray + ((size_t)c->max_batch + v.p0) * gi;
        DIS_HIP(launch_frames_to_gray(I0, I1, stride, pair_stride, c->frame_format, v.n, g.W, g.H, g0, g1, gs, gi, v.s,
                                      timing(c, 7)));
        I0 = g0;
        I1 = g1;
        stride = gs;
        pair_stride = gi;
    }
    if (fast && g.C >= 1) {
        PyramidArgs pa = pyramid_args(g, v.P, I0, I1, stride, pair_stride, v.n);
        if (c->debug) pa.write_l0 = 1;
        pa.zero = v.fb_count;
        pa.nzero = g.C + 1;
        if (pa.levels >= 2)  // the two streaming kernels; C == 1: k_pyr1 (dis_pyramid.hip)
            DIS_HIP(launch_pyramid2(pa, v.n, v.s, timing(c, 0)));
        else
            DIS_HIP(launch_pyramid1(pa, v.n, v.s, timing(c, 0)));
        for (int l = pa.levels + 1; l <= g.C; ++l) DIS_HIP(launch_down2(g, l, v.P.img0, v.P.img1, v.n, v.s));
    } else {
        // (zeroed on every path: DIS_STAGE_FALLBACK reports them after any calc)
        DIS_HIP(hipMemsetAsync(v.fb_count, 0, sizeof(int) * (g.C + 1), v.s));
        DIS_HIP(launch_level0(I0, I1, stride, pair_stride, g, v.P.img0, v.P.img1, v.n, v.s));
        for (int l = 1; l <= g.C; ++l) DIS_HIP(launch_down2(g, l, v.P.img0, v.P.img1, v.n, v.s));
    }
    if (!fast || c->debug) return enqueue_sobel(c, v);  // the fast search computes its template gradients itself
    return DIS_OK;
}

// Between the passes of a bidirectional call. The searches append to lists
// sized for one pass (fb_list_blocks(level) x pairs) at a count only the front
// stage zeroes: the backward pass starts its lists at 0 again, in stream order
// after the forward pass's last search.
dis_status enqueue_turn(dis_ctx* c, const SubBatch& v)
{
    DIS_HIP(hipMemsetAsync(v.fb_count, 0, sizeof(int) * (c->g.C + 1), v.s));
    if (!fast_search(c) || c->debug) return enqueue_sobel(c, v);  // dx / dy held frame 0's gradients
    return DIS_OK;
}

// Variational refinement of level l's dense flow.
dis_status enqueue_var_refine(dis_ctx* c, const SubBatch& v, int l)
{
    VarRefArgs a = varref_args(c->g, l, v.P);
    a.ws = c->vr_ws + (size_t)v.p0 * kVarRefPlanes * c->vr_plane;
    a.ws_plane = c->vr_plane;
    a.ws_stride = kVarRefPlanes * c->vr_plane;
    a.iters = c->p.var_refine_iters;
    if (c->timing) {  // eager, events around the finest level's refinement launches
        auto tf = [](void* cc, int kind) { return timing(static_cast<dis_ctx*>(cc), 4 + kind); };
        DIS_HIP(launch_var_refine(a, v.n, v.s, l == c->g.F ? +tf : nullptr, c));
        return DIS_OK;
    }
    auto& G = c->vrg[v.dir ? 1 : 0][v.sub][l];  // the level's launches replayed as one HIP graph
    if (G.n != v.n || G.p0 != v.p0) {
        if (G.exec) hipGraphExecDestroy(G.exec);
        G.exec = nullptr;
        G.n = G.p0 = -1;
        hipGraph_t graph = nullptr;
        DIS_HIP(hipStreamBeginCapture(c->cap, hipStreamCaptureModeThreadLocal));
        const hipError_t e = launch_var_refine(a, v.n, c->cap);
        const hipError_t e2 = hipStreamEndCapture(c->cap, &graph);
        DIS_HIP(e);
        DIS_HIP(e2);
        const hipError_t e3 = hipGraphInstantiate(&G.exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        DIS_HIP(e3);
        G.n = v.n;
        G.p0 = v.p0;
    }
    DIS_HIP(hipGraphLaunch(G.exec, v.s));
    return DIS_OK;
}

// One level of the scale loop (src/optical_flow.cpp:67-91): the search, and
// densify + refinement when on.
dis_status enqueue_level(dis_ctx* c, const SubBatch& v, int l)
{
    const Geometry& g = c->g;
    const LevelGeom& L = g.lv[l];
    const bool fast = fast_search(c);
    const bool vr = c->p.var_refine_iters > 0;
    const bool paper = c->k.paper != 0;
    const Timing t = timing(c, 1, l == g.F ? 2 : -1);
    // warm start: the coarsest level starts from the context's init plane as
    // every finer level does from the dense flow above it
    const bool warm_level = c->warm && l == g.C;
    const long long init_stride = (long long)c->iw * c->ih;
    if (fast) {
        Search8Args b = search8_args(g, l, v.P, c->k);
        set_search8_lanes(&b, search8_lanes(c->variant, (long long)L.npw * L.nph * v.n));
        b.tile_cap = c->variant == 9 ? 24 : 0;  // variant 9: most blocks through the fallback list
        b.fb_count = v.fb_count + l;
        b.fb_list = c->fb + c->fb_list_off[v.sub][l];
        b.fma = (c->precision == DIS_PRECISION_FMA && !paper) ? 1 : 0;
        if (paper && l < g.C) {  // the weighted coarse-to-fine init reads the coarser level's planes
            b.c_plane_off = g.lv[l + 1].plane_off;
            b.c_W = g.lv[l + 1].W;
            b.c_H = g.lv[l + 1].H;
        }
        if (vr && l < g.C) {  // refined dense flows: init from the coarser level's dense field
            b.dense_coarse = v.P.dense + g.lv[l + 1].dense_off;
            b.dense_stride = g.dense_stride;
        }
        if (warm_level) {  // (paper mode too: no coarser patches, the plain dense-init branch)
            b.dense_coarse = c->init + (size_t)v.p0 * init_stride;
            b.dense_stride = init_stride;
            b.coarse_ld = c->iw;
        }
        if (b.lanes_per_patch == 64 && (paper || b.fma)) set_search8_lanes(&b, 2);  // exact, non-paper only
        DIS_HIP(launch_search8(b, v.n, v.s, t));
    } else {
        SearchArgs a = search_args(g, l, v.P, c->k);
        if (warm_level) {
            a.dense_coarse = c->init + (size_t)v.p0 * init_stride;
            a.dense_stride = init_stride;
            a.coarse_ld = c->iw;
        }
        DIS_HIP(launch_search_generic(a, g.ps, v.n, v.s, t));
    }
    // the fast path materialises dense fields only under refinement (the next
    // level initialises from the refined field); otherwise the search fuses
    // the coarser level's densification at its sampled pixels and the output
    // kernel densifies the finest level
    if (fast && !c->debug && !vr) return DIS_OK;
    DIS_HIP(launch_densify(densify_args(g, l, v.P, c->k), v.n, v.s));
    return vr ? enqueue_var_refine(c, v, l) : DIS_OK;
}

// The back end: the finest level's flow densified, upsampled and cropped into `flow`.
dis_status enqueue_back(dis_ctx* c, const SubBatch& v, float2* flow)
{
    const Geometry& g = c->g;
    const bool fast = fast_search(c);
    const bool vr = c->p.var_refine_iters > 0;
    if (fast) {
        const OutputArgs o = output_args(g, v.P, c->k, flow, c->f16());
        if (output_fits(o) && !vr) {  // refined: the finest dense field exists
            DIS_HIP(launch_output(o, v.n, v.s, timing(c, 3), c->f16()));
            return DIS_OK;
        }
        if (!c->debug && !vr)  // the level stage skipped the finest densify: do it here
            DIS_HIP(launch_densify(densify_args(g, g.F, v.P, c->k), v.n, v.s));
    }
    DIS_HIP(launch_upsample(upsample_args(g, v.P, c->k, flow), v.n, v.s, c->f16()));
    return DIS_OK;
}

// One stage of one sub-batch: the front end, the turn, one level, or the back
// end. run_batches issues the stages stage-major across the sub-batches, so
// every sub-batch's next kernels are queued early even when the host is slow
// to enqueue a long stage.
dis_status enqueue_stage(dis_ctx* c, const SubBatch& v, int stage, const uint8_t* I0, const uint8_t* I1, size_t stride,
                         size_t pair_stride, float2* flow)
{
    StageRange range(stage, v.sub);
    if (stage == kStageFront) return enqueue_front(c, v, I0, I1, stride, pair_stride);
    if (stage == kStageTurn) return enqueue_turn(c, v);
    if (stage == kStageBack) return enqueue_back(c, v, flow);
    return enqueue_level(c, v, stage);
}

// The end of every call's enqueue on `s`: the next call orders itself after
// `done` (dis_ctx::needs_wait). A captured enqueue records nothing: its replay does.
dis_status call_done(dis_ctx* c, int n, hipStream_t s, bool capturing = false)
{
    c->last_batch = n;
    if (capturing) return DIS_OK;
    DIS_HIP(hipEventRecord(c->done, s));
    c->done_pending = true;
    c->done_stream = s;
    return DIS_OK;
}

}  // namespace

// One mutex per device guards the device's pooled sub-batch streams
// (sub_streams): held across a context's eager enqueue of a forked batch call
// and across a graph capture (which puts the pooled streams into capture
// mode), so concurrent contexts on different host threads never interleave
// work on a shared stream while it is being captured.
std::mutex& pool_mutex(int device)
{
    static std::mutex mu;
    static std::map<int, std::mutex> per_device;
    std::lock_guard<std::mutex> lock(mu);
    return per_device[device];
}

// Sub-batch streams: one pool per device for the whole process, created
// back to back on first use and never destroyed. HIP maps each new stream
// onto one of its few hardware queues (GPU_MAX_HW_QUEUES = 4) by usage at
// creation time; streams created per context after earlier contexts were
// destroyed landed two sub-batches on one queue (measured: every context
// after the first ran 1080p MEDIUM at 16.5k instead of 20.5k pairs/s with
// 2 streams; 20.2k with 1). Contexts on a device share the pool: work of
// concurrent contexts is ordered within a shared stream, still correct.
bool sub_streams(int device, hipStream_t (&out)[dis_ctx::kMaxSub])
{
    static std::mutex mu;
    static std::map<int, std::vector<hipStream_t>> pools;
    std::lock_guard<std::mutex> lock(mu);
    auto& v = pools[device];
    if (v.empty()) {
        for (int k = 0; k < dis_ctx::kMaxSub; ++k) {
            hipStream_t st = nullptr;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
                for (hipStream_t x : v) hipStreamDestroy(x);
                v.clear();
                return false;
            }
            v.push_back(st);
        }
    }
    for (int k = 0; k < dis_ctx::kMaxSub; ++k) out[k] = v[k];
    return true;
}

// Split n pairs into sub-batches on the context's streams (fork from `s`,
// join back into `s`): pairs are independent, so the latency-bound phases of
// one sub-batch (coarse levels, kernel tails) overlap the others' work. The
// sub-batches run in lockstep (staggered starts, stream priorities and
// uneven splits measured 1-4.5 % slower: DESIGN.md 7), stages issued
// stage-major so every sub-batch's next kernels are queued early.
// flow_bw non-null (dis_calc_bidir_batch_u8, never captured): after the
// forward pass every sub-batch runs the turn stage, the levels and the back
// end once more with the frames swapped, into flow_bw -- one pyramid, the same
// workspace, split, fork and join.
dis_status run_batches(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, size_t stride, size_t pair_stride,
                       float2* flow, hipStream_t s, bool capturing, float2* flow_bw)
{
    // refinement: one stream. Its many short bandwidth-bound kernels stall
    // behind a co-running sub-batch's long search launches (measured on
    // 3840x2160 SLOW, batch 2: 36.3 ms with two streams, 24.1 ms with one).
    const int S = c->p.var_refine_iters > 0 ? 1 : std::min(c->nsub, n);
    c->last_nsub = std::max(S, 1);
    std::vector<int> stages = {kStageFront};
    for (int l = c->g.C; l >= c->g.F; --l) stages.push_back(l);
    stages.push_back(kStageBack);
    const size_t nfw = stages.size();  // stages from here on run backward
    if (flow_bw) {
        if (capturing) return fail(DIS_ERR_INTERNAL, "bidirectional calls are not captured");
        stages.push_back(kStageTurn);
        for (int l = c->g.C; l >= c->g.F; --l) stages.push_back(l);
        stages.push_back(kStageBack);
    }
    if (c->needs_wait(s) && !capturing) DIS_HIP(hipStreamWaitEvent(s, c->done, 0));  // the workspace is free
    if (S <= 1) {
        for (size_t i = 0; i < stages.size(); ++i) {
            const int dir = i >= nfw ? 1 : 0;
            dis_status r = enqueue_stage(c, sub_batch(c, 0, n, 0, s, dir), stages[i], I0, I1, stride, pair_stride,
                                         dir ? flow_bw : flow);
            if (r != DIS_OK) return r;
        }
        return call_done(c, n, s, capturing);
    }
    // Every sub-batch runs on a context-owned stream forked from and joined
    // back into the caller's stream. (Running sub-batch 0 on the caller's stream
    // saves a cross-queue hop, but HIP maps streams onto its few hardware
    // queues in creation order, so whether the caller's stream shares a queue
    // with sub[1] -- serialising the two sub-batches -- depended on how many
    // streams the process had created before: 15k vs 20k pairs/s at 1080p.
    // The context's own streams are created back to back, on distinct queues.)
    // The fork / stages / join sequence as a plan (dis_plan.h): checked against
    // the capture rules before a capture issues any of it -- a plan the HIP
    // runtime cannot capture (an unjoined stream) fails at EndCapture and
    // leaves a stream in capture mode and an invalid graph handle behind
    // (tools/capture_probe.hip) -- then executed op by op.
    const std::vector<PlanOp> plan = batch_plan(S, (int)stages.size());
    if (capturing) {
        const std::string why = check_capture_plan(plan.data(), (int)plan.size(), 1 + S, 1 + S);
        if (!why.empty()) return fail(DIS_ERR_INTERNAL, "batch stream plan cannot be captured: " + why);
    }
    auto stream_of = [&](int x) { return x == 0 ? s : c->sub[x - 1]; };
    auto event_of = [&](int e) { return e == 0 ? c->fork : c->join[e - 1]; };
    for (const PlanOp& o : plan) {
        if (o.kind == kOpRecord) {
            DIS_HIP(hipEventRecord(event_of(o.event), stream_of(o.stream)));
        } else if (o.kind == kOpWait) {
            DIS_HIP(hipStreamWaitEvent(stream_of(o.stream), event_of(o.event), 0));
            if (capturing) {  // the waiting stream must now be in the origin's capture
                hipStreamCaptureStatus cs0, cs1;
                unsigned long long id0 = 0, id1 = 0;
                DIS_HIP(hipStreamGetCaptureInfo(s, &cs0, &id0));
                DIS_HIP(hipStreamGetCaptureInfo(stream_of(o.stream), &cs1, &id1));
                if (cs0 != hipStreamCaptureStatusActive || cs1 != hipStreamCaptureStatusActive || id0 != id1)
                    return fail(DIS_ERR_DEVICE, "graph capture: a sub-batch stream did not join the call's capture");
            }
        } else {
            const int k = o.stream - 1;
            const int a = (int)((long long)n * k / S), b = (int)((long long)n * (k + 1) / S);
            const int dir = (size_t)o.stage >= nfw ? 1 : 0;
            dis_status r = enqueue_stage(c, sub_batch(c, k, b - a, a, stream_of(o.stream), dir), stages[o.stage],
                                         I0 + (size_t)a * pair_stride, I1 + (size_t)a * pair_stride, stride,
                                         pair_stride, c->flow_at(dir ? flow_bw : flow, (size_t)a));
            if (r != DIS_OK) return r;
        }
    }
    return call_done(c, n, s, capturing);
}

// run_batches as a replayed HIP graph (see dis_ctx::MainGraph). Eager when
// graphs are off, under kernel timing (per-dispatch events), debug dumps or
// variational refinement (its own per-level graphs).
dis_status run_batches_graph(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, size_t stride,
                             size_t pair_stride, float2* flow, hipStream_t s)
{
    // eager: graphs off, kernel timing, debug dumps, refinement (its own
    // per-level graphs)
    if (!c->graphs || c->timing || c->debug || c->p.var_refine_iters > 0 || !c->cap) {
        std::lock_guard<std::mutex> lock(pool_mutex(c->device));  // eager enqueue onto the pooled streams
        return run_batches(c, n, I0, I1, stride, pair_stride, flow, s);
    }
    auto key_is = [&](const dis_ctx::MainGraph& G) {
        return G.exec && G.n == n && G.i0 == I0 && G.i1 == I1 && G.flow == flow && G.stride == stride &&
               G.pair_stride == pair_stride && G.nsub == c->nsub && G.precision == c->precision &&
               G.variant == c->variant && G.format == c->flow_format && G.frame_format == c->frame_format;
    };
    dis_ctx::MainGraph* G = nullptr;
    for (auto& e : c->mg)
        if (key_is(e)) G = &e;
    if (!G) {
        // victim: an empty slot, else the least recently used exec
        G = &c->mg[0];
        for (auto& e : c->mg) {
            if (!e.exec) {
                G = &e;
                break;
            }
            if (e.used < G->used) G = &e;
        }
        if (G->launched) {  // its last replay may still be in flight: never update under it
            DIS_HIP(hipEventSynchronize(G->last));
            G->launched = false;
        }
        if (!G->last) DIS_HIP(hipEventCreateWithFlags(&G->last, hipEventDisableTiming));
        StageRange range("dis: graph capture");
        hipGraph_t graph = nullptr;
        dis_status r;
        hipError_t e, e0;
        {
            // the capture forks onto the device's pooled sub-batch streams:
            // no other context's eager work may enter them meanwhile
            std::lock_guard<std::mutex> lock(pool_mutex(c->device));
            e0 = hipStreamBeginCapture(c->cap, hipStreamCaptureModeThreadLocal);
            r = e0 == hipSuccess ? run_batches(c, n, I0, I1, stride, pair_stride, flow, c->cap, true) : DIS_OK;
            e = e0 == hipSuccess ? hipStreamEndCapture(c->cap, &graph) : e0;
            // HIP 7.2: a failed EndCapture writes a non-null handle that is not a
            // graph (instantiating it crashed tools/capture_probe, destroying it
            // returns hipErrorIllegalState) -- never touch it
            if (e != hipSuccess) graph = nullptr;
            // and a stream it left unjoined stays in capture mode (mode 5): no
            // later work may go to the pooled streams then
            for (int k = 0; k < dis_ctx::kMaxSub; ++k) {
                hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
                if (hipStreamIsCapturing(c->sub[k], &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
                    (void)hipGetLastError();
                    c->graphs = 0;
                    return fail(DIS_ERR_DEVICE, "graph capture left sub-batch stream " + std::to_string(k) +
                                                    " in capture mode (" + hipGetErrorName(e) + ")");
                }
            }
        }
        hipError_t e2 = hipErrorUnknown;
        if (r == DIS_OK && e == hipSuccess) {
            if (G->exec) {  // same topology (same n and sub-batches): update the parameters in place
                hipGraphExecUpdateResult res;
                hipGraphNode_t bad = nullptr;
                e2 = hipGraphExecUpdate(G->exec, graph, &bad, &res);
                if (e2 != hipSuccess) {
                    (void)hipGetLastError();
                    hipGraphExecDestroy(G->exec);
                    G->exec = nullptr;
                }
            }
            if (!G->exec) e2 = hipGraphInstantiate(&G->exec, graph, nullptr, nullptr, 0);
        }
        if (graph) hipGraphDestroy(graph);
        if (r != DIS_OK) {
            // a real error inside the captured enqueue (not an invalidated
            // capture): report it; no eager retry on sub-streams that may still
            // be in a bad capture state
            (void)hipGetLastError();
            if (G->exec) hipGraphExecDestroy(G->exec);
            G->exec = nullptr;
            G->n = -1;
            return r;
        }
        if (e2 != hipSuccess) {
            // The capture was invalidated (e.g. another thread synchronised the
            // device or used the legacy default stream meanwhile) or failed to
            // instantiate: this call runs eagerly -- same results -- and the
            // next call with this key tries to capture again.
            (void)hipGetLastError();
            if (G->exec) hipGraphExecDestroy(G->exec);
            G->exec = nullptr;
            G->n = -1;
            std::lock_guard<std::mutex> lock(pool_mutex(c->device));
            return run_batches(c, n, I0, I1, stride, pair_stride, flow, s);
        }
        G->n = n;
        G->i0 = I0;
        G->i1 = I1;
        G->flow = flow;
        G->stride = stride;
        G->pair_stride = pair_stride;
        G->nsub = c->nsub;
        G->precision = c->precision;
        G->variant = c->variant;
        G->format = c->flow_format;  // (a graph holds its kernels: never replayed for the other store type)
        G->frame_format = c->frame_format;  // (the luma launch is part of the captured call, or is not)
        G->subs = c->last_nsub;
    }
    G->used = ++c->graph_clock;
    c->last_nsub = G->subs;  // a replay runs the sub-batches it was captured with (DIS_STAGE_FALLBACK)
    if (c->needs_wait(s)) DIS_HIP(hipStreamWaitEvent(s, c->done, 0));  // the workspace is free
    {
        StageRange range("dis: graph launch");
        DIS_HIP(hipGraphLaunch(G->exec, s));
    }
    DIS_HIP(hipEventRecord(G->last, s));
    G->launched = true;
    return call_done(c, n, s);
}

}  // namespace dis
