// dis_ctx.h -- the context of the C-ABI (struct dis_ctx, include/dis_abi.h) and
// what its two translation units share: dis_runtime.hip (create / destroy, the
// entry points, the host-frame pipeline) and dis_enqueue.hip (the launch
// sequence).
#pragma once

#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "dis_host.h"
#include "dis_launch_args.h"

// per sub-batch: the levels' fallback list counts (k_search8_fb)
constexpr size_t kFbCounters = dis::kMaxLevels;

// Host-frame path state (dis_calc_batch_u8 with DIS_MEM_HOST), made on the
// first host call: the batch runs in chunks of `chunk` pairs through two
// device staging slots, so that the upload of chunk j+1, the computation of
// chunk j and the download of chunk j-1 overlap (the reference's own pattern
// is host frames in, host flow out per pair, src/main.cpp:115-116,184-189).
// The copies go straight between the caller's buffers and the device: a
// hipMemcpyAsync on pageable memory runs at the DMA rate but returns only when
// it is done (tools/host_xfer_probe.hip), so the downloads are issued by a
// thread of their own while the calling thread uploads and enqueues. Staging
// through page-locked buffers with threaded host copies, and host waits
// instead of stream waits in front of the copies, measured slower (DESIGN.md
// 4, host-frame path).
struct HostPipe {
    int chunk = 0;
    int format = 0;                   // flow format the output slots were sized for
    int frame_format = 0;             // frame format the input slots were sized for
    size_t frame = 0;                 // bytes of one frame (W * H * bytes per pixel of the frame format)
    uint8_t* din[2] = {};             // device: chunk I0 frames, then chunk I1 frames
    float2* dout[2] = {};             // device: chunk flows (format-typed)
    hipStream_t up = nullptr, down = nullptr;
    hipEvent_t up_done[2] = {}, comp_done[2] = {}, down_done[2] = {};
    bool comp_pending[2] = {}, down_pending[2] = {};
    // the download thread: jobs in chunk order; `issued` counts the jobs whose
    // copy has been issued and whose down_done event has been recorded
    struct Job {
        char* dst;
        const char* src;
        size_t bytes;
        int slot;
    };
    std::thread th;
    std::mutex mu;
    std::condition_variable cv, done_cv;
    std::vector<Job> q;
    long long posted = 0, issued = 0;
    hipError_t err = hipSuccess;
    bool stop = false;
    int device = 0;
    // what the last host call did (dis_host_pipeline_info)
    int last_chunks = 0, last_direct_in = 0, last_direct_out = 0;

    void run()
    {
        (void)hipSetDevice(device);
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return stop || !q.empty(); });
                if (q.empty()) return;
                j = q.front();
                q.erase(q.begin());
            }
            hipError_t e = hipStreamWaitEvent(down, comp_done[j.slot], 0);
            if (e == hipSuccess) e = hipMemcpyAsync(j.dst, j.src, j.bytes, hipMemcpyDeviceToHost, down);
            if (e == hipSuccess) e = hipEventRecord(down_done[j.slot], down);
            std::lock_guard<std::mutex> l(mu);
            if (e != hipSuccess && err == hipSuccess) err = e;
            ++issued;
            done_cv.notify_all();
        }
    }
    void post(const Job& j)
    {
        {
            std::lock_guard<std::mutex> l(mu);
            q.push_back(j);
            ++posted;
        }
        cv.notify_one();
    }
    // wait until the first `k` posted jobs are issued; the first error seen
    hipError_t wait_issued(long long k)
    {
        std::unique_lock<std::mutex> l(mu);
        done_cv.wait(l, [&] { return issued >= k; });
        const hipError_t e = err;
        err = hipSuccess;
        return e;
    }
    ~HostPipe()
    {
        if (th.joinable()) {
            {
                std::lock_guard<std::mutex> l(mu);
                stop = true;
            }
            cv.notify_all();
            th.join();
        }
        // copies of a call that failed part-way may still be in flight
        if (up) (void)hipStreamSynchronize(up);
        if (down) (void)hipStreamSynchronize(down);
        for (int s = 0; s < 2; ++s) {
            hipFree(din[s]);
            hipFree(dout[s]);
            for (hipEvent_t e : {up_done[s], comp_done[s], down_done[s]})
                if (e) hipEventDestroy(e);
        }
        if (up) hipStreamDestroy(up);
        if (down) hipStreamDestroy(down);
    }
};

struct dis_ctx {
    dis_params p;
    dis::Geometry g;
    dis::LaunchConsts k;  // of g and p, made by dis_create
    int device = 0;
    int max_batch = 1;
    int debug = 0;
    int variant = 0;  // 0 auto, 1 generic only, 2/3/4/5/6: patch_size-8 search with 4/2/8/1/64 lanes per patch
    int last_batch = 0;
    int last_nsub = 1;  // sub-batches of the last calc (their fallback counters, DIS_STAGE_FALLBACK)
    hipStream_t own = nullptr;
    static constexpr int kMaxSub = 8;
    int nsub = 2;                        // sub-batch streams per calc (dis_set_concurrency)
    int precision = 0;                   // dis_set_precision: DIS_PRECISION_EXACT / _FMA
    int flow_format = 0;                 // dis_set_flow_format: DIS_FLOW_F32 / _F16
    bool f16() const { return flow_format == DIS_FLOW_F16; }
    // bytes of one (u, v) vector of a full-resolution flow in the context's format
    size_t vec_bytes() const { return f16() ? 2 * sizeof(uint16_t) : sizeof(float2); }
    // `pairs` flows after a format-typed flow pointer
    float2* flow_at(float2* flow, size_t pairs) const
    {
        return reinterpret_cast<float2*>(reinterpret_cast<char*>(flow) + pairs * g.W * g.H * vec_bytes());
    }
    int frame_format = 0;                // dis_set_frame_format: DIS_FRAME_GRAY8 / a colour dis_frame_format
    // bytes of one pixel of the frames the calc calls take
    int pixel_bytes() const { return dis::frame_format_channels(frame_format); }
    // Colour frames are reduced to gray by the front stage (dis_luma.hip) into
    // this buffer, which the unchanged pyramid path then reads: max_batch first
    // frames, then max_batch second frames, each gray_stride() x H bytes with
    // rows of W rounded up to 16. Made by dis_set_frame_format on the first
    // colour format, kept from then on.
    uint8_t* gray = nullptr;
    size_t gray_stride() const { return ((size_t)g.W + 15) & ~size_t(15); }
    hipStream_t sub[kMaxSub] = {};
    hipEvent_t fork = nullptr;
    // end of the previous call's work on its stream: every call first orders
    // its stream after it, so calls on different streams (calc_device on a
    // caller stream, then calc_batch on `own`) never overlap on the workspace
    hipEvent_t done = nullptr;
    bool done_pending = false;
    hipStream_t done_stream = nullptr;  // the stream `done` was recorded on
    // the next call must wait for `done` unless it is on that same stream
    // (stream order already serialises it; skipping the wait packet saves the
    // inter-call gap)
    bool needs_wait(hipStream_t s) const { return done_pending && s != done_stream; }
    hipEvent_t join[kMaxSub] = {};
    // variational refinement: its ~16 launches per fixed-point iteration per level
    // are replayed as one HIP graph per (sub-batch, level), captured on first use
    // (all pointers are context workspace; re-captured when the slice changes)
    // and one per direction: a bidirectional call's backward pass swaps the frames
    struct VrGraph {
        hipGraphExec_t exec = nullptr;
        int n = -1, p0 = -1;
    } vrg[2][kMaxSub][dis::kMaxLevels];
    hipStream_t cap = nullptr;  // capture-only stream
    // The whole batch call (both sub-batches' pyramid, level searches and
    // output, with the fork/join) replayed as one HIP graph: dis_set_graphs,
    // default on. A small LRU of executable graphs keyed by the call (buffers,
    // batch size, sub-batches, precision, variant): a caller that ping-pongs
    // a few buffer sets replays without re-capturing. A miss re-captures into
    // the least recently used slot and updates its exec in place -- only after
    // that exec's last replay has finished (`last`): the update rewrites the
    // kernel arguments an unstarted node of that replay would still read.
    int graphs = 1;
    static constexpr int kGraphCache = 4;
    struct MainGraph {
        hipGraphExec_t exec = nullptr;
        hipEvent_t last = nullptr;  // recorded after this exec's latest launch
        bool launched = false;
        unsigned long long used = 0;  // LRU clock
        int n = -1, nsub = -1, precision = -1, variant = -1, format = -1, frame_format = -1;
        int subs = 1;  // sub-batches the captured call ran (last_nsub on replay)
        const void *i0 = nullptr, *i1 = nullptr;
        void* flow = nullptr;
        size_t stride = 0, pair_stride = 0;
    } mg[kGraphCache];
    unsigned long long graph_clock = 0;
    // workspace (device)
    float* img0 = nullptr;
    float* img1 = nullptr;
    float* dx = nullptr;
    float* dy = nullptr;
    float2* pu = nullptr;
    float2* dense = nullptr;
    float* vr_ws = nullptr;  // variational refinement workspace (kVarRefPlanes planes per pair)
    long long vr_plane = 0;
    // patch-search fallback lists (dis_search8.hip k_search8_fb): per sub-batch
    // k, kFbCounters list counts (one per level) at fb + k * kFbCounters, then
    // per (k, level) a list of up to fb_list_blocks(level) * pairs entries at
    // fb + fb_list_off[k][level]
    int* fb = nullptr;
    size_t fb_list_off[8][dis::kMaxLevels] = {};
    // host-frame path (DIS_MEM_HOST): device slots, streams and the download
    // thread made on the first host call; dis_set_host_pipeline sets the chunk
    // (0 = auto)
    std::unique_ptr<HostPipe> hp;
    int host_chunk = 0;
    // dis_calc_bidir_batch_u8 and dis_calc_batch_init_u8 with DIS_MEM_HOST
    // (synchronous calls: one at a time): device staging for max_batch pairs,
    // both frames in stage_in (stage_in_px bytes per pixel: 1, or 4 once a
    // call came under a colour frame format) and two float flows in stage_out
    // (both directions, or the flow and the init input), made on the first such call
    uint8_t* stage_in = nullptr;
    int stage_in_px = 0;
    float2* stage_out = nullptr;
    // warm start (dis_calc_batch_init_u8): the context's init planes, iw x ih
    // float2 per pair for max_batch pairs; `warm` is set for the duration of a
    // warm-started call's enqueue (the coarsest level then starts from them)
    float2* init = nullptr;
    int iw = 0, ih = 0;
    bool warm = false;
    // kernel timing
    int timing = 0;
    struct Rec {
        int kind;
        hipEvent_t a, b;
    };
    std::vector<hipEvent_t> pool;
    std::vector<Rec> recs;
    size_t pool_next = 0;
    static constexpr int kKinds = 8;  // dis_kernel_time classes
    int launches[kKinds] = {};
    double total_ms[kKinds] = {};
    long long dropped = 0;  // records lost to a failed event creation (dis_kernel_time fails then)
};

namespace dis {

// Per-launch timing: when enabled, hands out an event pair from the pool to be
// attached to the next dispatch (hipExtLaunchKernelGGL) and books it under
// `kind` (and `kind2` if >= 0). (dis_runtime.hip)
Timing timing(dis_ctx* c, int kind, int kind2 = -1);

// the launch sequence (dis_enqueue.hip)
std::mutex& pool_mutex(int device);
bool sub_streams(int device, hipStream_t (&out)[dis_ctx::kMaxSub]);
dis_status run_batches(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, size_t stride, size_t pair_stride,
                       float2* flow, hipStream_t s, bool capturing = false, float2* flow_bw = nullptr);
dis_status run_batches_graph(dis_ctx* c, int n, const uint8_t* I0, const uint8_t* I1, size_t stride,
                             size_t pair_stride, float2* flow, hipStream_t s);

}  // namespace dis
