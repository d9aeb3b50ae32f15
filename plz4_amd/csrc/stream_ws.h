// Device memory that belongs to one job at a time and is ordered across the callers' streams on the device.
// StreamOrder: the event behind the last job and the stream it ran on.  A job on another stream waits for that event on the device
// (no host block); whoever frees or regrows the memory waits for it on the host first.  MarkOnExit records the event on every way
// out of the function that enqueues a job: whatever was enqueued before an early return still uses the memory.
// DeviceBuffer: pointer + size; what is held is only ever freed behind a drain.
// Included behind <hip/hip_runtime.h> (tests/emu/emu_stream_ws.cpp: behind a recording stand-in for the few calls used here).
#pragma once

struct StreamOrder {
    hipEvent_t  done = nullptr;
    hipStream_t stream = nullptr;          // of the last job
    bool        pending = false;           // a job was marked and nobody has waited for it on the host since

    // before a job is enqueued on s / behind it
    hipError_t wait(hipStream_t s) { return pending && stream != s ? hipStreamWaitEvent(s, done, 0) : hipSuccess; }
    hipError_t mark(hipStream_t s)
    {
        hipError_t e = done ? hipSuccess : hipEventCreateWithFlags(&done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(done, s);
        if (e == hipSuccess) { pending = true; stream = s; }
        return e;
    }
    hipError_t drain()                     // host wait for the last job
    {
        const hipError_t e = pending ? hipEventSynchronize(done) : hipSuccess;
        if (e == hipSuccess) pending = false;
        return e;
    }
    bool idle()                            // the last job is over (asked without waiting)
    {
        if (!pending || hipEventQuery(done) == hipSuccess) return true;
        (void)hipGetLastError();           // (hipErrorNotReady of the query)
        return false;
    }
    void destroy()
    {
        (void)drain();
        if (done) hipEventDestroy(done);
        done = nullptr; stream = nullptr; pending = false;
    }
};

struct MarkOnExit {
    StreamOrder* order = nullptr;
    hipStream_t  s = nullptr;
    MarkOnExit() = default;
    MarkOnExit(const MarkOnExit&) = delete;
    void arm(StreamOrder& o, hipStream_t st) { order = &o; s = st; }
    // the regular way out, for callers that report a failed mark; every other way out marks from the destructor
    hipError_t leave() { StreamOrder* o = order; order = nullptr; return o ? o->mark(s) : hipSuccess; }
    ~MarkOnExit() { (void)leave(); }
};

struct DeviceBuffer {
    uint8_t* d = nullptr;
    size_t   bytes = 0;

    // At least `need` bytes (exactly `need` when it has to allocate).  What is held is freed behind drained(); when that fails its
    // error is returned and nothing has changed.  A refused allocation is no error: *refused is set, the HIP error cleared, the
    // buffer left empty, and the caller decides what that means.
    template <class Drain> hipError_t reserve_behind(size_t need, bool* refused, Drain&& drained)
    {
        *refused = false;
        if (need <= bytes) return hipSuccess;
        if (d) { const hipError_t e = drained(); if (e != hipSuccess) return e; }
        release();
        if (hipMalloc((void**)&d, need) != hipSuccess) { (void)hipGetLastError(); d = nullptr; *refused = true; }
        else bytes = need;
        return hipSuccess;
    }
    hipError_t reserve(size_t need, StreamOrder& o, bool* refused) { return reserve_behind(need, refused, [&] { return o.drain(); }); }
    // (a staging slot's workspace: ordered by the slot's own stream)
    hipError_t reserve(size_t need, hipStream_t s, bool* refused) { return reserve_behind(need, refused, [&] { return hipStreamSynchronize(s); }); }
    // drain and free (also when the drain fails: its error is returned); the order forgets its stream
    hipError_t release(StreamOrder& o) { const hipError_t e = o.drain(); o.stream = nullptr; release(); return e; }
    // (nothing in flight uses it: the caller has waited)
    void release() { if (d) hipFree(d); d = nullptr; bytes = 0; }
};
