// CPU driver for plz4_amd/csrc/stream_ws.h (tests/test_stream_ws.py): the header compiled against a recording stand-in for the
// handful of HIP calls it uses.  Every call is logged in order; hipMalloc can be told to refuse, hipEventQuery to say "not ready".
// One StreamOrder and one DeviceBuffer, driven call by call from the test.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorNotReady = 600, hipErrorUnknown = 999 };
typedef struct FakeEvent*  hipEvent_t;
typedef struct FakeStream* hipStream_t;
enum { hipEventDisableTiming = 2 };

namespace {
std::string g_log;
int g_lastErr = hipSuccess, g_refuse = 0, g_notReady = 0, g_syncFails = 0, g_events = 0, g_live = 0;

void note(const char* what, const void* a = nullptr, const void* b = nullptr)
{
    char buf[96];
    snprintf(buf, sizeof buf, "%s %ld %ld\n", what, (long)(intptr_t)a, (long)(intptr_t)b);
    g_log += buf;
}
hipError_t done(hipError_t e) { if (e != hipSuccess) g_lastErr = e; return e; }
}

hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags)
{
    *e = (hipEvent_t)(intptr_t)(++g_events);
    note(flags == hipEventDisableTiming ? "hipEventCreateWithFlags" : "hipEventCreateWithFlags(timing)", *e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { note("hipEventRecord", e, s); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { note("hipEventSynchronize", e); return done(g_syncFails ? hipErrorUnknown : hipSuccess); }
hipError_t hipEventQuery(hipEvent_t e) { note("hipEventQuery", e); return done(g_notReady ? hipErrorNotReady : hipSuccess); }
hipError_t hipEventDestroy(hipEvent_t e) { note("hipEventDestroy", e); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { note("hipStreamWaitEvent", s, e); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { note("hipStreamSynchronize", s); return hipSuccess; }
hipError_t hipGetLastError() { note("hipGetLastError"); const int e = g_lastErr; g_lastErr = hipSuccess; return e; }
hipError_t hipMalloc(void** p, size_t n)
{
    note("hipMalloc", (const void*)(intptr_t)n);
    if (g_refuse > 0) { --g_refuse; *p = (void*)(intptr_t)0xBAD; return done(hipErrorOutOfMemory); }   // (the pointer is not to be trusted)
    *p = malloc(n ? n : 1); ++g_live;
    return hipSuccess;
}
hipError_t hipFree(void* p) { note("hipFree"); free(p); --g_live; return hipSuccess; }

#include "../../plz4_amd/csrc/stream_ws.h"

namespace {
StreamOrder  g_order;
DeviceBuffer g_buf;
hipStream_t stream_of(int s) { return (hipStream_t)(intptr_t)s; }

// a launch function in the shape of the product's: the job is marked on every way out once the guard is armed
hipError_t launch(hipStream_t s, bool arm, bool early)
{
    MarkOnExit job;
    if (arm) job.arm(g_order, s);
    note("enqueue", s);
    if (early) return hipErrorUnknown;
    return job.leave();
}
}

extern "C" {
void ws_reset() { free(g_buf.d); g_live = 0; g_order = StreamOrder(); g_buf = DeviceBuffer(); g_log.clear(); g_lastErr = hipSuccess; g_refuse = g_notReady = g_syncFails = 0; }
void ws_clear_log() { g_log.clear(); }
const char* ws_log() { return g_log.c_str(); }
void ws_refuse_mallocs(int n) { g_refuse = n; }
void ws_query_not_ready(int on) { g_notReady = on; }
void ws_sync_fails(int on) { g_syncFails = on; }
int  ws_last_error() { return g_lastErr; }
int  ws_live_allocations() { return g_live; }

int  ws_wait(int s) { return g_order.wait(stream_of(s)); }
int  ws_mark(int s) { return g_order.mark(stream_of(s)); }
int  ws_drain() { return g_order.drain(); }
int  ws_idle() { return g_order.idle() ? 1 : 0; }
void ws_destroy() { g_order.destroy(); }
int  ws_pending() { return g_order.pending ? 1 : 0; }
long ws_stream() { return (long)(intptr_t)g_order.stream; }
long ws_event() { return (long)(intptr_t)g_order.done; }

// >= 0: 0 reserved, 1 refused; < 0: minus the error of the drain
int  ws_reserve(long need) { bool refused = true; const hipError_t e = g_buf.reserve((size_t)need, g_order, &refused); return e != hipSuccess ? -e : (refused ? 1 : 0); }
int  ws_reserve_on_stream(long need, int s) { bool refused = true; const hipError_t e = g_buf.reserve((size_t)need, stream_of(s), &refused); return e != hipSuccess ? -e : (refused ? 1 : 0); }
int  ws_release() { return g_buf.release(g_order); }
long ws_bytes() { return (long)g_buf.bytes; }
int  ws_has_memory() { return g_buf.d != nullptr ? 1 : 0; }
int  ws_launch(int s, int arm, int early) { return launch(stream_of(s), arm != 0, early != 0); }
}
