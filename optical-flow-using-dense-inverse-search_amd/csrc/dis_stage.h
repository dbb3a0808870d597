// dis_stage.h -- the buffers of an entry point that takes host or device
// pointers. On host pointers the call is synchronous: device copies of the
// inputs, device buffers for the outputs, the launch on them, the downloads
// and the wait, with everything freed on every path. On device pointers
// (`staged` false) every pointer passes through and finish() only launches.
#pragma once

#include <vector>

#include "dis_host.h"

namespace dis {

class HostStage {
public:
    explicit HostStage(hipStream_t s, bool staged = true) : s_(s), staged_(staged) {}
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    ~HostStage()
    {
        for (const Buf& b : bufs_) hipFree(b.dev);  // (waits for whatever a failed call left in flight)
    }
    // the device copy of `bytes` at `host`, its upload enqueued; null for a null pointer
    template <class T>
    const T* in(const T* host, size_t bytes)
    {
        if (!staged_ || !host) return host;
        void* d = alloc(bytes, nullptr);
        if (d) note(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, s_));
        return static_cast<const T*>(d);
    }
    // a device buffer that finish() downloads to `host`; null for a null pointer
    template <class T>
    T* out(T* host, size_t bytes)
    {
        return staged_ && host ? static_cast<T*>(alloc(bytes, host)) : host;
    }
    void* scratch(size_t bytes) { return alloc(bytes, nullptr); }
    // `launch` (if all went well so far), the downloads, the wait; the status
    template <class Launch>
    dis_status finish(Launch&& launch, const char* what)
    {
        if (oom_) return fail(DIS_ERR_OUT_OF_MEMORY, "device allocation failed");
        if (err_ == hipSuccess) note(launch());
        for (const Buf& b : bufs_)
            if (b.host && err_ == hipSuccess) note(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, s_));
        if (staged_ && err_ == hipSuccess) note(hipStreamSynchronize(s_));
        if (err_ != hipSuccess) return fail(DIS_ERR_DEVICE, std::string(what) + " failed: " + hipGetErrorString(err_));
        return DIS_OK;
    }

private:
    struct Buf {
        void* dev;
        void* host;  // where finish() downloads it, or null
        size_t bytes;
    };
    void* alloc(size_t bytes, void* host)
    {
        void* d = nullptr;
        if (oom_ || !bytes) return nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) {
            (void)hipGetLastError();  // (the error is sticky)
            oom_ = true;
            return nullptr;
        }
        bufs_.push_back({d, host, bytes});
        return d;
    }
    void note(hipError_t e) { err_ = err_ == hipSuccess ? e : err_; }  // the first failure stands
    hipStream_t s_;
    bool staged_, oom_ = false;
    hipError_t err_ = hipSuccess;
    std::vector<Buf> bufs_;
};

}  // namespace dis
