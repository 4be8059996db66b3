// abi_scope.hpp -- the host-side scaffold of a C-ABI entry point: the stream scope that keeps a call from returning while
// the device still uses the caller's arrays, the upload that goes with it, the event timers and the 1-D launch shape.
// Host code only.  (gridder.hip includes it too: its plan creation and all of its entries run under synced().)
#pragma once
#include <algorithm>
#include <vector>

#include "common.hpp"

namespace pfbhip {

// 1-D grid of `threads`-wide workgroups over n items; an empty launch still gets one workgroup (its kernel guards i < n)
inline dim3 blocks1d(int64_t n, int threads = 256) { return dim3(uint32_t(std::max<int64_t>(ceil_div(n, threads), 1))); }

// buf <- host[0, n) on st (buf grows as needed, at least one element); NULL host: nothing, returns NULL
template <class T>
const T *upload(DevBuf<T> &buf, const T *host, size_t n, hipStream_t st)
{
    if (!host) return nullptr;
    buf.ensure(std::max<size_t>(n, 1));
    if (n) PFB_HIP(hipMemcpyAsync(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice, st));
    return buf.p;
}

// Runs body(), then waits for st -- also when body() throws (the original exception goes on unchanged): no call returns
// while the device still reads or writes the caller's arrays, or buffers and staging vectors that unwinding would free.
// Everything an entry point enqueues goes inside one synced(); argument validation stays in front of it, and so do the
// declarations of such buffers and vectors (what body() itself declares is destroyed before the wait).
template <class F>
void synced(hipStream_t st, F &&body)
{
    try {
        body();
    } catch (...) {
        (void)hipStreamSynchronize(st);
        throw;
    }
    PFB_HIP(hipStreamSynchronize(st));
}

// Elapsed device time between start() and stop() on one stream, when the caller asked for it.
struct EventTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool on;
    explicit EventTimer(bool enable) : on(enable)
    {
        if (!on) return;
        PFB_HIP(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) {
            (void)hipEventDestroy(e0);
            throw std::runtime_error("hipEventCreate failed");
        }
    }
    EventTimer(const EventTimer &) = delete;
    EventTimer &operator=(const EventTimer &) = delete;
    ~EventTimer()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void start(hipStream_t st) { if (on) PFB_HIP(hipEventRecord(e0, st)); }
    void stop(hipStream_t st) { if (on) PFB_HIP(hipEventRecord(e1, st)); }
    double ms()  // after the stream has been synchronised
    {
        float t = 0.f;
        if (on) PFB_HIP(hipEventElapsedTime(&t, e0, e1));
        return double(t);
    }
};

// HIP events around the stages of a pipeline on one stream.  Off, nothing is created or recorded; events are reused
// across collect() calls.
struct StageTimer {
    bool enabled;
    hipStream_t stream;
    struct Rec {
        int stage;
        hipEvent_t a, b;
    };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    explicit StageTimer(hipStream_t st = nullptr, bool on = false) : enabled(on), stream(st) {}
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    hipEvent_t get()
    {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        PFB_HIP(hipEventCreate(&e));
        return e;
    }
    void begin(int stage)
    {
        if (!enabled) return;
        Rec r{stage, get(), get()};
        PFB_HIP(hipEventRecord(r.a, stream));
        recs.push_back(r);
    }
    void end()
    {
        if (!enabled) return;
        PFB_HIP(hipEventRecord(recs.back().b, stream));
    }
    // waits for the bracketed stages and adds their times to ms[stage] / calls[stage]
    void collect(double *ms, int64_t *calls)
    {
        for (auto &r : recs) {
            PFB_HIP(hipEventSynchronize(r.b));
            float t = 0;
            PFB_HIP(hipEventElapsedTime(&t, r.a, r.b));
            ms[r.stage] += t;
            calls[r.stage] += 1;
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
        recs.clear();
    }
    ~StageTimer()
    {
        for (auto &r : recs) {
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

}  // namespace pfbhip
