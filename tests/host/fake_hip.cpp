// fake_hip.cpp -- a legal but adversarial HIP runtime for the CPU-only pipeline harness (tests/host/pipeline_sanitize.cpp).
//
// Linked INSTEAD of libamdhip64 under the host code of the product (srcnn_capi.cpp, srcnn_pipeline.cpp ...): every hip*
// function that code calls is defined here, on plain host memory and host threads, so that ASan / UBSan / TSan see the
// stager, copier, fanner and pre-fault threads, the lanes, the bounce slots and the graph capture run for real.
//
//   memory    hipMalloc = malloc of exactly the requested size (ASan's redzone sits at the true end), filled with 0xFF and
//             entered in a registry (base, size, device / page-locked).  hipFree / hipHostFree drain every stream first, as
//             the real ones synchronise, poison the block again and free it.  hipHostRegister enters a range, and
//             hipPointerGetAttributes answers from the registry.
//   streams   an in-order queue of closures with a worker thread each: TSan sees the real concurrency between streams and
//             host threads.  The NULL stream is one more such queue (the code under test orders bounced copies on it).
//   events    a marker in a queue.  hipEventQuery answers hipErrorNotReady until the marker has run; hipStreamWaitEvent
//             blocks the waiting stream's worker on the marker.
//   copies    "no pageable pointer reaches a HIP copy" (DESIGN 1): every byte of the host side of a copy must lie in
//             page-locked registry blocks, the device side inside ONE device block -- when the copy is queued and again
//             when it runs (a range unregistered or freed under a pending copy).  The host source of a pending copy must
//             not change between the call and the copy (a staging slot reused too early): checked by a checksum.
//   capture   between hipStreamBeginCapture and hipStreamEndCapture closures are recorded, not run; hipGraphLaunch queues
//             copies.  An allocation by the capturing thread, a synchronising call or a query on the capturing stream, or
//             a query of an event that belongs to it, is a violation.
//   schedule  FAKE_HIP_SCHEDULE=asap: workers run operations as they arrive.  =lazy: a worker starts an operation only
//             when somebody DEMANDS it: a synchronise / query of its stream, hipDeviceSynchronize and hipFree (everything),
//             hipEventSynchronize / hipEventQuery (the event's stream up to the marker), transitively through
//             hipStreamWaitEvent.  The library's waits poll hipEventQuery, so lazy is the latest legal schedule: host code
//             that reads a result, reuses a slot or frees a buffer without having waited meets 0xFF bytes or a pending
//             closure every time, not one run in a thousand.
//   faults    FAKE_HIP_FAIL=<function>:<n> makes the n-th call of that function return hipErrorUnknown, once.
//   devices   one gfx950-named device with 256 CUs; peer calls succeed trivially.
//
// Every breach of the contract is COUNTED (fakehip::violations()) and said on stderr; the harness requires 0 at exit and an
// empty registry after srcnn_shutdown.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace fakehip {

void violation(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
unsigned long violations();
unsigned long pageable_copies();
size_t live_blocks();
size_t live_handles();
bool in_block(const void* p, size_t bytes, int kind);
void enqueue(hipStream_t s, std::function<void()> fn);
void finish();

namespace {

std::atomic<unsigned long> g_violations{0}, g_pageable{0};
bool g_lazy = false;
std::string g_fail_fn;
long g_fail_n = 0;
std::atomic<long> g_fail_seen{0};
thread_local hipError_t tl_err = hipSuccess;
thread_local int tl_capturing = 0;      // captures this thread has open (hipStreamCaptureModeThreadLocal)

struct Init {
    Init()
    {
        const char* s = getenv("FAKE_HIP_SCHEDULE");
        g_lazy = s && !strcmp(s, "lazy");
        if (const char* f = getenv("FAKE_HIP_FAIL")) {
            const char* c = strchr(f, ':');
            g_fail_fn.assign(f, c ? (size_t)(c - f) : strlen(f));
            g_fail_n = c ? atol(c + 1) : 1;
        }
    }
} g_init;

bool inject(const char* fn)
{
    if (g_fail_n <= 0 || g_fail_fn != fn) return false;
    return g_fail_seen.fetch_add(1) + 1 == g_fail_n;
}
hipError_t ret(hipError_t e) { if (e != hipSuccess) tl_err = e; return e; }
#define FAKE_INJECT(name) do { if (inject(name)) return ret(hipErrorUnknown); } while (0)

// ---- registry ----
enum { kDevice = 0, kPinned = 1, kRegistered = 2 };
struct Block { size_t size; int kind; };
std::mutex g_mu;                                  // registry, stream and event tables
std::map<uintptr_t, Block> g_blocks;

bool find_block_locked(const void* p, uintptr_t& base, Block& b)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    auto it = g_blocks.upper_bound(a);
    if (it == g_blocks.begin()) return false;
    --it;
    if (a >= it->first + it->second.size) return false;
    base = it->first; b = it->second;
    return true;
}

// every byte of [p, p+n) page-locked (adjacent blocks may join up)
bool all_page_locked(const void* p, size_t n)
{
    std::lock_guard<std::mutex> lk(g_mu);
    uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uintptr_t e = a + n;
    while (a < e) {
        uintptr_t base; Block b;
        if (!find_block_locked(reinterpret_cast<const void*>(a), base, b) || b.kind == kDevice) return false;
        a = base + b.size;
    }
    return true;
}

struct Event;
struct Op {
    std::function<void()> fn;
    std::shared_ptr<Event> marker; uint64_t gen = 0;      // hipEventRecord
    std::shared_ptr<Event> wait; uint64_t wgen = 0;       // hipStreamWaitEvent
    bool record_at_launch = false;                        // a record captured into a graph
};

struct Stream {
    std::mutex m;
    std::condition_variable cv;
    std::deque<Op> q;
    uint64_t enq = 0, done = 0, demand = 0;
    bool stop = false, capturing = false;
    std::vector<Op> captured;
    std::thread th;
};
struct Event {
    std::mutex m;
    std::condition_variable cv;
    uint64_t gen = 0, done_gen = 0;
    Stream* st = nullptr;      // stream of the latest record, and the operation count that covers its marker
    uint64_t pos = 0;
};
struct GraphRec { std::vector<Op> ops; };

std::map<Stream*, std::shared_ptr<Stream>> g_streams;
std::map<Event*, std::shared_ptr<Event>> g_events;
std::shared_ptr<Stream> g_null;

void demand_stream(Stream& s, uint64_t upto)
{
    { std::lock_guard<std::mutex> lk(s.m); if (s.demand < upto) s.demand = upto; }
    s.cv.notify_all();
}
void demand_event(Event& e)
{
    Stream* st; uint64_t pos;
    { std::lock_guard<std::mutex> lk(e.m); st = e.st; pos = e.pos; }
    if (st) demand_stream(*st, pos);
}

void worker(Stream* s)
{
    for (;;) {
        Op op;
        {
            std::unique_lock<std::mutex> lk(s->m);
            s->cv.wait(lk, [&] { return s->stop || (!s->q.empty() && (!g_lazy || s->done < s->demand)); });
            if (s->q.empty()) return;            // stopped, and nothing left
            op = std::move(s->q.front());
            s->q.pop_front();
        }
        if (op.wait) {
            demand_event(*op.wait);              // demands pass through hipStreamWaitEvent
            std::unique_lock<std::mutex> lk(op.wait->m);
            op.wait->cv.wait(lk, [&] { return op.wait->done_gen >= op.wgen; });
        }
        if (op.fn) op.fn();
        if (op.marker) {
            { std::lock_guard<std::mutex> lk(op.marker->m); if (op.marker->done_gen < op.gen) op.marker->done_gen = op.gen; }
            op.marker->cv.notify_all();
        }
        op = Op{};                               // what the closure holds goes before the operation counts as done
        { std::lock_guard<std::mutex> lk(s->m); ++s->done; }
        s->cv.notify_all();
    }
}

std::shared_ptr<Stream> make_stream()
{
    auto s = std::make_shared<Stream>();
    s->th = std::thread(worker, s.get());
    return s;
}

std::shared_ptr<Stream> stream_of(hipStream_t h)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!h) {
        if (!g_null) g_null = make_stream();
        return g_null;
    }
    auto it = g_streams.find(reinterpret_cast<Stream*>(h));
    if (it == g_streams.end()) return nullptr;
    return it->second;
}
std::shared_ptr<Event> event_of(hipEvent_t h)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_events.find(reinterpret_cast<Event*>(h));
    return it == g_events.end() ? nullptr : it->second;
}

void push(Stream& s, Op op)
{
    { std::lock_guard<std::mutex> lk(s.m); if (s.capturing) { s.captured.push_back(std::move(op)); return; } s.q.push_back(std::move(op)); ++s.enq; }
    s.cv.notify_all();
}

// everything queued on the stream so far has run
void drain(Stream& s)
{
    std::unique_lock<std::mutex> lk(s.m);
    const uint64_t target = s.enq;
    if (s.demand < target) s.demand = target;
    s.cv.notify_all();
    s.cv.wait(lk, [&] { return s.done >= target; });
}
void drain_all()
{
    std::vector<std::shared_ptr<Stream>> all;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        for (auto& kv : g_streams) all.push_back(kv.second);
        if (g_null) all.push_back(g_null);
    }
    for (auto& s : all) {
        bool cap;
        { std::lock_guard<std::mutex> lk(s->m); cap = s->capturing; }
        if (!cap) drain(*s);
    }
}

bool capturing(Stream& s) { std::lock_guard<std::mutex> lk(s.m); return s.capturing; }

uint64_t checksum(const void* p, size_t n)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t sum = 0x9e3779b97f4a7c15ull;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t v; memcpy(&v, b + i, 8); sum = (sum ^ v) * 0x100000001b3ull + (sum >> 29); }
    for (; i < n; ++i) sum = (sum ^ b[i]) * 0x100000001b3ull;
    return sum;
}

void* alloc_block(size_t bytes, int kind)
{
    void* p = malloc(bytes ? bytes : 1);
    if (!p) return nullptr;
    memset(p, 0xFF, bytes);
    std::lock_guard<std::mutex> lk(g_mu);
    g_blocks[reinterpret_cast<uintptr_t>(p)] = Block{bytes, kind};
    return p;
}
hipError_t free_block(void* p, bool device, const char* fn)
{
    if (!p) return hipSuccess;
    drain_all();                                 // the real call synchronises the device
    size_t size = 0;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_blocks.find(reinterpret_cast<uintptr_t>(p));
        if (it == g_blocks.end() || (it->second.kind == kDevice) != device || it->second.kind == kRegistered) {
            violation("%s(%p): not a live block of that kind", fn, p);
            return ret(hipErrorInvalidValue);
        }
        size = it->second.size;
        g_blocks.erase(it);
    }
    memset(p, 0xFF, size);
    free(p);
    return hipSuccess;
}

// the checks of one side of a copy; what = "queued" / "runs"
bool check_host_side(const void* p, size_t n, const char* fn, const char* what)
{
    if (all_page_locked(p, n)) return true;
    ++g_pageable;
    violation("%s: host range [%p, +%zu) is not page-locked in every byte when the copy %s", fn, p, n, what);
    return false;
}
bool check_device_side(const void* p, size_t n, const char* fn, const char* what)
{
    if (in_block(p, n, kDevice)) return true;
    violation("%s: device range [%p, +%zu) leaves its block when the copy %s", fn, p, n, what);
    return false;
}

hipError_t copy(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t stream, bool sync, const char* fn)
{
    auto s = stream_of(stream);
    if (!s) { violation("%s on a stream that does not exist", fn); return ret(hipErrorInvalidHandle); }
    if (n == 0) return hipSuccess;
    const bool host_src = kind == hipMemcpyHostToDevice, host_dst = kind == hipMemcpyDeviceToHost;
    if (kind != hipMemcpyHostToDevice && kind != hipMemcpyDeviceToHost && kind != hipMemcpyDeviceToDevice) {
        violation("%s: copy kind %d is not modelled", fn, (int)kind);
        return ret(hipErrorInvalidValue);
    }
    bool ok = host_src ? check_host_side(src, n, fn, "is queued") : check_device_side(src, n, fn, "is queued");
    ok = (host_dst ? check_host_side(dst, n, fn, "is queued") : check_device_side(dst, n, fn, "is queued")) && ok;
    if (!ok) return ret(hipErrorInvalidValue);
    const uint64_t sum = host_src ? checksum(src, n) : 0;
    std::string name = fn;
    push(*s, Op{[=] {
        bool live = host_src ? check_host_side(src, n, name.c_str(), "runs") : check_device_side(src, n, name.c_str(), "runs");
        live = (host_dst ? check_host_side(dst, n, name.c_str(), "runs") : check_device_side(dst, n, name.c_str(), "runs")) && live;
        if (!live) return;
        if (host_src && checksum(src, n) != sum)
            violation("%s: the host source [%p, +%zu) changed while the copy was pending", name.c_str(), src, n);
        memmove(dst, src, n);
    }});
    if (sync) drain(*s);
    return hipSuccess;
}

hipError_t fill(void* dst, int value, size_t n, hipStream_t stream, bool sync, const char* fn)
{
    auto s = stream_of(stream);
    if (!s) { violation("%s on a stream that does not exist", fn); return ret(hipErrorInvalidHandle); }
    if (!check_device_side(dst, n, fn, "is queued")) return ret(hipErrorInvalidValue);
    std::string name = fn;
    push(*s, Op{[=] { if (check_device_side(dst, n, name.c_str(), "runs")) memset(dst, value, n); }});
    if (sync) drain(*s);
    return hipSuccess;
}

}  // namespace

void violation(const char* fmt, ...)
{
    ++g_violations;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fprintf(stderr, "fake_hip VIOLATION: %s\n", buf);
}
unsigned long violations() { return g_violations.load(); }
unsigned long pageable_copies() { return g_pageable.load(); }
size_t live_blocks() { std::lock_guard<std::mutex> lk(g_mu); return g_blocks.size(); }
// streams and events created and not destroyed (the NULL stream is the runtime's own)
size_t live_handles() { std::lock_guard<std::mutex> lk(g_mu); return g_streams.size() + g_events.size(); }

// [p, p+bytes) lies inside ONE live block (kind: 0 device, 1 page-locked, -1 either)
bool in_block(const void* p, size_t bytes, int kind)
{
    std::lock_guard<std::mutex> lk(g_mu);
    uintptr_t base; Block b;
    if (!find_block_locked(p, base, b)) return false;
    if (kind == kDevice && b.kind != kDevice) return false;
    if (kind == kPinned && b.kind == kDevice) return false;
    return reinterpret_cast<uintptr_t>(p) + bytes <= base + b.size;
}

// a kernel launch: one closure on the stream (recorded, not run, inside a capture)
void enqueue(hipStream_t h, std::function<void()> fn)
{
    auto s = stream_of(h);
    if (!s) { violation("launch on a stream that does not exist"); return; }
    push(*s, Op{std::move(fn)});
}

// end of the process: the NULL stream's worker is joined (every other stream was destroyed by its owner)
void finish()
{
    std::shared_ptr<Stream> n;
    { std::lock_guard<std::mutex> lk(g_mu); n.swap(g_null); }
    if (!n) return;
    drain(*n);
    { std::lock_guard<std::mutex> lk(n->m); n->stop = true; }
    n->cv.notify_all();
    n->th.join();
}

}  // namespace fakehip

using namespace fakehip;

extern "C" {

// ---- devices ----
hipError_t hipGetDeviceCount(int* n) { FAKE_INJECT("hipGetDeviceCount"); *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { FAKE_INJECT("hipSetDevice"); return d == 0 ? hipSuccess : ret(hipErrorInvalidDevice); }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int d)
{
    FAKE_INJECT("hipGetDeviceProperties");
    if (d != 0) return ret(hipErrorInvalidDevice);
    memset(prop, 0, sizeof *prop);
    snprintf(prop->name, sizeof prop->name, "fake MI355X");
    snprintf(prop->gcnArchName, sizeof prop->gcnArchName, "gfx950:sramecc+:xnack-");
    prop->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipDeviceGetPCIBusId(char* bdf, int len, int) { snprintf(bdf, (size_t)len, "ffff:ff:1f.7"); return hipSuccess; }
hipError_t hipDeviceCanAccessPeer(int* can, int, int) { *can = 1; return hipSuccess; }
hipError_t hipDeviceEnablePeerAccess(int, unsigned) { return hipSuccess; }
hipError_t hipGetLastError(void) { const hipError_t e = tl_err; tl_err = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e)
{
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorNotReady: return "device not ready";
    case hipErrorUnknown: return "unknown error (injected)";
    case hipErrorInvalidValue: return "invalid argument";
    default: return "fake HIP error";
    }
}
hipError_t hipDeviceSynchronize(void)
{
    FAKE_INJECT("hipDeviceSynchronize");
    if (tl_capturing) violation("hipDeviceSynchronize by a thread that is capturing a stream");
    drain_all();
    return hipSuccess;
}

// ---- memory ----
hipError_t hipMalloc(void** p, size_t bytes)
{
    FAKE_INJECT("hipMalloc");
    if (tl_capturing) violation("hipMalloc(%zu) inside a stream capture", bytes);
    *p = alloc_block(bytes, kDevice);
    return *p ? hipSuccess : ret(hipErrorOutOfMemory);
}
hipError_t hipFree(void* p) { return free_block(p, true, "hipFree"); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned)
{
    FAKE_INJECT("hipHostMalloc");
    if (tl_capturing) violation("hipHostMalloc(%zu) inside a stream capture", bytes);
    *p = alloc_block(bytes, kPinned);
    return *p ? hipSuccess : ret(hipErrorOutOfMemory);
}
hipError_t hipHostFree(void* p) { return free_block(p, false, "hipHostFree"); }
hipError_t hipHostRegister(void* p, size_t bytes, unsigned)
{
    FAKE_INJECT("hipHostRegister");
    std::lock_guard<std::mutex> lk(g_mu);
    uintptr_t base; Block b;
    if (!p || !bytes || find_block_locked(p, base, b)) return ret(hipErrorHostMemoryAlreadyRegistered);
    g_blocks[reinterpret_cast<uintptr_t>(p)] = Block{bytes, kRegistered};
    return hipSuccess;
}
hipError_t hipHostUnregister(void* p)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_blocks.find(reinterpret_cast<uintptr_t>(p));
    if (it == g_blocks.end() || it->second.kind != kRegistered) { violation("hipHostUnregister(%p): not a registered range", p); return ret(hipErrorHostMemoryNotRegistered); }
    g_blocks.erase(it);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* a, const void* p)
{
    std::lock_guard<std::mutex> lk(g_mu);
    uintptr_t base; Block b;
    if (!find_block_locked(p, base, b)) return ret(hipErrorInvalidValue);
    memset(a, 0, sizeof *a);
    a->type = b.kind == kDevice ? hipMemoryTypeDevice : hipMemoryTypeHost;
    a->device = 0;
    a->devicePointer = const_cast<void*>(p);
    a->hostPointer = b.kind == kDevice ? nullptr : const_cast<void*>(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind)
{
    FAKE_INJECT("hipMemcpy");
    if (tl_capturing) violation("hipMemcpy by a thread that is capturing a stream");
    return copy(dst, src, n, kind, nullptr, true, "hipMemcpy");
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
    FAKE_INJECT("hipMemcpyAsync");
    return copy(dst, src, n, kind, s, false, "hipMemcpyAsync");
}
hipError_t hipMemcpyPeerAsync(void* dst, int, const void* src, int, size_t n, hipStream_t s)
{
    FAKE_INJECT("hipMemcpyPeerAsync");
    return copy(dst, src, n, hipMemcpyDeviceToDevice, s, false, "hipMemcpyPeerAsync");
}
hipError_t hipMemset(void* dst, int v, size_t n)
{
    FAKE_INJECT("hipMemset");
    return fill(dst, v, n, nullptr, true, "hipMemset");
}
hipError_t hipMemsetAsync(void* dst, int v, size_t n, hipStream_t s)
{
    FAKE_INJECT("hipMemsetAsync");
    return fill(dst, v, n, s, false, "hipMemsetAsync");
}

// ---- streams ----
hipError_t hipStreamCreateWithFlags(hipStream_t* out, unsigned)
{
    FAKE_INJECT("hipStreamCreateWithFlags");
    auto s = make_stream();
    { std::lock_guard<std::mutex> lk(g_mu); g_streams[s.get()] = s; }
    *out = reinterpret_cast<hipStream_t>(s.get());
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t h)
{
    auto s = h ? stream_of(h) : nullptr;
    if (!s) { violation("hipStreamDestroy(%p): no such stream", (void*)h); return ret(hipErrorInvalidHandle); }
    if (capturing(*s)) violation("hipStreamDestroy of a capturing stream");
    else drain(*s);                              // (the real call returns at once and lets the queue finish)
    { std::lock_guard<std::mutex> lk(g_mu); g_streams.erase(s.get()); }
    { std::lock_guard<std::mutex> lk(s->m); s->stop = true; }
    s->cv.notify_all();
    s->th.join();
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t h)
{
    FAKE_INJECT("hipStreamSynchronize");
    auto s = stream_of(h);
    if (!s) { violation("hipStreamSynchronize(%p): no such stream", (void*)h); return ret(hipErrorInvalidHandle); }
    if (capturing(*s)) { violation("hipStreamSynchronize on a capturing stream"); return ret(hipErrorStreamCaptureUnsupported); }
    drain(*s);
    return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t h)
{
    FAKE_INJECT("hipStreamQuery");
    auto s = stream_of(h);
    if (!s) { violation("hipStreamQuery(%p): no such stream", (void*)h); return ret(hipErrorInvalidHandle); }
    if (capturing(*s)) { violation("hipStreamQuery on a capturing stream"); return ret(hipErrorStreamCaptureUnsupported); }
    bool ready;
    { std::lock_guard<std::mutex> lk(s->m); s->demand = s->enq; ready = s->done >= s->enq; }
    s->cv.notify_all();
    return ready ? hipSuccess : ret(hipErrorNotReady);
}
hipError_t hipStreamWaitEvent(hipStream_t h, hipEvent_t eh, unsigned)
{
    FAKE_INJECT("hipStreamWaitEvent");
    auto s = stream_of(h);
    auto e = event_of(eh);
    if (!s || !e) { violation("hipStreamWaitEvent: no such stream or event"); return ret(hipErrorInvalidHandle); }
    Op op;
    op.wait = e;
    { std::lock_guard<std::mutex> lk(e->m); op.wgen = e->gen; }
    push(*s, std::move(op));
    return hipSuccess;
}

// ---- events ----
hipError_t hipEventCreateWithFlags(hipEvent_t* out, unsigned)
{
    FAKE_INJECT("hipEventCreateWithFlags");
    auto e = std::make_shared<Event>();
    { std::lock_guard<std::mutex> lk(g_mu); g_events[e.get()] = e; }
    *out = reinterpret_cast<hipEvent_t>(e.get());
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* out) { FAKE_INJECT("hipEventCreate"); return hipEventCreateWithFlags(out, 0); }
hipError_t hipEventDestroy(hipEvent_t h)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_events.erase(reinterpret_cast<Event*>(h))) { violation("hipEventDestroy(%p): no such event", (void*)h); return ret(hipErrorInvalidHandle); }
    return hipSuccess;               // (markers and waits still queued keep the record alive, as the real runtime does)
}
hipError_t hipEventRecord(hipEvent_t eh, hipStream_t h)
{
    FAKE_INJECT("hipEventRecord");
    auto s = stream_of(h);
    auto e = event_of(eh);
    if (!s || !e) { violation("hipEventRecord: no such stream or event"); return ret(hipErrorInvalidHandle); }
    std::lock_guard<std::mutex> lk(s->m);
    Op op;
    op.marker = e;
    if (s->capturing) { op.record_at_launch = true; s->captured.push_back(std::move(op)); return hipSuccess; }
    {
        std::lock_guard<std::mutex> le(e->m);
        op.gen = ++e->gen;
        e->st = s.get();
        e->pos = s->enq + 1;
    }
    s->q.push_back(std::move(op));
    ++s->enq;
    s->cv.notify_all();
    return hipSuccess;
}
static bool event_belongs_to_capture(Event& e)
{
    Stream* st;
    { std::lock_guard<std::mutex> lk(e.m); st = e.st; }
    if (!st) return false;
    std::shared_ptr<Stream> keep;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_streams.find(st);
        if (it == g_streams.end()) return false;
        keep = it->second;
    }
    return capturing(*keep);
}
hipError_t hipEventQuery(hipEvent_t eh)
{
    FAKE_INJECT("hipEventQuery");
    auto e = event_of(eh);
    if (!e) { violation("hipEventQuery(%p): no such event", (void*)eh); return ret(hipErrorInvalidHandle); }
    if (event_belongs_to_capture(*e)) violation("hipEventQuery of an event of a stream that is being captured");
    demand_event(*e);
    std::lock_guard<std::mutex> lk(e->m);
    return e->done_gen >= e->gen ? hipSuccess : ret(hipErrorNotReady);
}
hipError_t hipEventSynchronize(hipEvent_t eh)
{
    FAKE_INJECT("hipEventSynchronize");
    auto e = event_of(eh);
    if (!e) { violation("hipEventSynchronize(%p): no such event", (void*)eh); return ret(hipErrorInvalidHandle); }
    if (event_belongs_to_capture(*e)) violation("hipEventSynchronize on an event of a stream that is being captured");
    demand_event(*e);
    std::unique_lock<std::mutex> lk(e->m);
    const uint64_t g = e->gen;
    e->cv.wait(lk, [&] { return e->done_gen >= g; });
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    if (!event_of(a) || !event_of(b)) return ret(hipErrorInvalidHandle);
    *ms = 0.25f;
    return hipSuccess;
}

// ---- capture and graphs ----
hipError_t hipStreamBeginCapture(hipStream_t h, hipStreamCaptureMode)
{
    FAKE_INJECT("hipStreamBeginCapture");
    auto s = h ? stream_of(h) : nullptr;
    if (!s) { violation("hipStreamBeginCapture: no such stream (or the NULL stream)"); return ret(hipErrorInvalidHandle); }
    std::lock_guard<std::mutex> lk(s->m);
    if (s->capturing) { violation("hipStreamBeginCapture on a capturing stream"); return ret(hipErrorIllegalState); }
    s->capturing = true;
    s->captured.clear();
    ++tl_capturing;
    return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t h, hipGraph_t* out)
{
    auto s = h ? stream_of(h) : nullptr;
    *out = nullptr;
    if (!s) return ret(hipErrorInvalidHandle);
    std::lock_guard<std::mutex> lk(s->m);
    if (!s->capturing) return ret(hipErrorIllegalState);
    s->capturing = false;
    --tl_capturing;
    auto* g = new GraphRec;
    g->ops.swap(s->captured);
    *out = reinterpret_cast<hipGraph_t>(g);
    return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t h, hipStreamCaptureStatus* st)
{
    auto s = stream_of(h);
    *st = (s && h && capturing(*s)) ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t* out, hipGraph_t g, hipGraphNode_t*, char*, size_t)
{
    FAKE_INJECT("hipGraphInstantiate");
    if (!g) return ret(hipErrorInvalidValue);
    *out = reinterpret_cast<hipGraphExec_t>(new GraphRec(*reinterpret_cast<GraphRec*>(g)));
    return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t x, hipStream_t h)
{
    FAKE_INJECT("hipGraphLaunch");
    auto s = stream_of(h);
    if (!s || !x) return ret(hipErrorInvalidHandle);
    for (const Op& o : reinterpret_cast<GraphRec*>(x)->ops) {
        if (o.record_at_launch) {
            std::lock_guard<std::mutex> lk(s->m);
            Op op;
            op.marker = o.marker;
            { std::lock_guard<std::mutex> le(o.marker->m); op.gen = ++o.marker->gen; o.marker->st = s.get(); o.marker->pos = s->enq + 1; }
            s->q.push_back(std::move(op));
            ++s->enq;
        } else {
            Op op = o;
            if (op.wait) { std::lock_guard<std::mutex> le(op.wait->m); op.wgen = op.wait->gen; }
            push(*s, std::move(op));
        }
    }
    s->cv.notify_all();
    return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t g) { delete reinterpret_cast<GraphRec*>(g); return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t g) { delete reinterpret_cast<GraphRec*>(g); return hipSuccess; }

}  // extern "C"
