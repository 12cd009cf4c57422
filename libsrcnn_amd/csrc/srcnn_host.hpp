// srcnn_host.hpp -- host-side state shared by the C-ABI translation units (srcnn_capi.cpp: contexts, plumbing,
// the device-resident hot path; srcnn_pipeline.cpp: the host-pointer pipelines and the node-level calls; srcnn_frames.cpp: the
// YUV / RGB frame calls).
// Internal; the public surface is include/srcnn_amd.h.
//
// One process may drive several CONTEXTS.  A context is one device binding with everything that lives in that
// device's memory: the uploaded weights, the contribution-table cache, per-stream workspaces, the host-stream slots
// and the ProcessSRCNN lanes.  srcnn_init(device) creates context 0 (the round-1/2 behaviour: one device per process);
// srcnn_init_devices(list) creates one context per list entry -- the same physical device may appear several times
// ("virtual contexts"), which is how a 1-GPU box exercises the node-level paths.  The reference's single ProcessSRCNN
// call saturates its whole machine through OpenMP (src/libsrcnn.cpp:665,791-798,817-824); with several contexts the
// large-image path of srcnn_process_u8 does the same with the node's GPUs.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstddef>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "../../include/srcnn_amd.h"
#include "../../include/srcnn_amd_debug.h"
#include "srcnn_kernels.h"
#include "srcnn_owned.hpp"
#include "srcnn_settings.hpp"
#include "srcnn_y_path_geom.hpp"

namespace srcnn {

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void set_last_error(const char* msg);
const char* last_error();

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return ::srcnn::fail(SRCNN_E_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct Ctx;
void* pinned_alloc(Ctx& cx, size_t bytes);      // page-locked, visible to every device, on the context's NUMA node

// ---- ownership: srcnn_owned.hpp bound to HIP.  Every HIP resource of the host layer is a member of one of these. ----
struct EventTraits { static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); } };
struct StreamTraits { static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); } };
struct GraphTraits { static void destroy(hipGraph_t g) { (void)hipGraphDestroy(g); } };
struct GraphExecTraits { static void destroy(hipGraphExec_t g) { (void)hipGraphExecDestroy(g); } };
using Event = Owned<hipEvent_t, EventTraits>;
using Stream = Owned<hipStream_t, StreamTraits>;
using Graph = Owned<hipGraph_t, GraphTraits>;
using GraphExec = Owned<hipGraphExec_t, GraphExecTraits>;

struct DevAlloc {
    static void drain() { (void)hipDeviceSynchronize(); }      // kernels launched earlier (any stream) may still be using the old block
    static int alloc(void** p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? SRCNN_OK : fail(SRCNN_E_DEVMEM, "hipMalloc(%zu bytes) failed", bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {          // grow(want, cx): page-locked memory is placed by the context's NUMA node
    static void drain() { (void)hipDeviceSynchronize(); }
    static int alloc(void** p, size_t bytes, Ctx& cx) { return (*p = pinned_alloc(cx, bytes)) ? SRCNN_OK : SRCNN_E_DEVMEM; }
    static void free(void* p) { (void)hipHostFree(p); }
};
struct BounceAlloc : PinnedAlloc { static void drain() {} };      // (grown under HostBounce::mu: no copy is in flight)
template <class T> using DevBuf = GrowBuf<T, DevAlloc>;
using PinnedBuf = GrowBuf<unsigned char, PinnedAlloc>;

struct DeviceTable {          // one uploaded AxisTable; freed only when the last reference goes
    DevBuf<int> first, taps;
    DevBuf<double> weight;
    int stride = 0;
    int max_taps = 0;
    unsigned long long stamp = 0;      // LRU clock of the cache
    // host copies (tiny) so that band planners can ask "which source rows does destination range [a,b) read"
    std::vector<int> h_first, h_taps;
    bool monotone = false;             // first[] and first[]+taps[] both non-decreasing: a tile's span is given by its ends
    DevAxisTable view() const { return DevAxisTable{first.data(), taps.data(), weight.data(), stride, max_taps, monotone ? 1 : 0, h_first.data(), h_taps.data()}; }
    unsigned src_len = 0;              // of the axis the taps read
    // source index range [lo, hi) read by destination indices [a, b)
    void source_span(unsigned a, unsigned b, unsigned& lo, unsigned& hi) const { taps_span(h_first.data(), h_taps.data(), src_len, a, b, lo, hi); }
};
using TableRef = std::shared_ptr<DeviceTable>;

struct Scratch {            // the buffers of a Workspace: movable, so that a workspace that lives on is emptied by assignment
    DevBuf<float> tmp;      // first resampler pass
    DevBuf<float> up;       // upscaled Y (band)
    DevBuf<float> c2;       // 32 layer-2 planes (band)
    DevBuf<float> planes;   // colour shell: split planes / Y' / resized chroma planes
    DevBuf<float> win;      // rect call: the layer-3 result of a window (band), tight, before its interior is stored
    DevBuf<unsigned char> bytes;
    DevBuf<unsigned char> list;   // rect list call: the descriptor tables of a call's atlases (written in stream order)
    DevBuf<unsigned> delta_spans;        // delta call: the span tables of the grid DeltaStage::key names
    DevBuf<unsigned char> delta_flags;   // delta call: the tile flags of srcnn_y_path_delta_f32_dev
    size_t footprint() const
    {
        return sizeof(float) * (tmp.size() + up.size() + c2.size() + planes.size() + win.size()) + bytes.size() + list.size() +
               sizeof(unsigned) * delta_spans.size() + delta_flags.size();
    }
};
// What the delta call keeps beside Scratch::delta_spans / delta_flags.  The span tables depend on the geometry alone, so they
// are uploaded when `key` or `owner` changes and not again (a stream of frames: once).  `pin` receives the flags of a whole
// delta operation, which waits for them before it returns, under the workspace's mutex: one buffer is enough.
// owner: the delta calls share these buffers and build their tables by different rules (srcnn_delta.hpp, srcnn_rgb_delta.hpp),
// so one call's tables must not answer for the other's.  Defensive: at every geometry compared so far the two rules gave the
// same tables, so no test can tell a confused owner; nothing promises that they always will.
enum class DeltaSpanOwner { YPlane, Rgb };
struct DeltaStage {
    PinnedBuf pin;
    bool valid = false;
    DeltaSpanOwner owner = DeltaSpanOwner::YPlane;
    unsigned key[7] = {0, 0, 0, 0, 0, 0, 0};         // w, h, dw, dh, filter, tile_w, tile_h
};
// Page-locked staging of the rect list call's descriptor tables.  A call fills the next slot of the ring on the host, queues the
// copy to Scratch::list on its stream and records the slot's event behind it; a slot is written again only after that event has
// passed.  So a call never waits for the stream (unless four calls' copies are still queued), and calls queued back to back
// cannot disturb each other's tables: each has a slot of its own on the host, and the device copy is rewritten in stream order.
struct ListStaging {
    static constexpr int kSlots = 4;
    struct Slot { PinnedBuf pin; Event ev; bool pending = false; } slot[kSlots];
    unsigned next = 0;
};
struct Workspace : Scratch {          // scratch of one stream / graph / lane; grow-only
    std::mutex mu;          // held while a call enqueues work that uses this scratch
    // raw, and freed here by hand: run_conv12 allocates it, and that function's text is part of the kernel fingerprint (build.py)
    unsigned* queue = nullptr;                   // two words: the tile queue of k_conv12_mfma launches on this workspace's stream
    bool queue_dirty = false;                    // a call failed after launching: zero the counters before the next launch
    bool frozen = false;    // a captured graph has these pointers baked in: growing is an error
    ListStaging list_stage;
    DeltaStage delta_stage;
    template <class T>
    int grow(DevBuf<T>& b, size_t want)          // b: one of this workspace's buffers
    {
        if (want > b.size() && frozen) return fail(SRCNN_E_ARG, "workspace of a captured graph cannot grow (%zu > %zu elements)", want, b.size());
        return b.grow(want);
    }
    void clear() { static_cast<Scratch&>(*this) = {}; list_stage = {}; delta_stage = {}; (void)hipFree(queue); queue = nullptr; }
    ~Workspace() { (void)hipFree(queue); }
};

// One invocation of the path: on which context and stream it runs, on which scratch, with which numerics.  The mode is
// read ONCE at the public entry point, so a concurrent srcnn_set_mode never changes a call half way through, and
// `timing` is how a graph capture tells the stage timers to stay out (event pairs cannot be timed inside a capture).
// `hold` keeps every contribution table the call launches with referenced: for an eager call until the call returns
// (the cache itself only frees after a device sync), for a graph until the graph is destroyed.
struct Call {
    Ctx* cx = nullptr;
    hipStream_t s = nullptr;
    Workspace* ws = nullptr;
    int mode = SRCNN_MODE_STRICT;       // SRCNN_MODE_* in the low byte; for SRCNN_MODE_RELAXED the SRCNN_RELAX_* mask in bits 8..11
    bool timing = true;
    std::vector<TableRef>* hold = nullptr;
    bool strict() const { return mode == SRCNN_MODE_STRICT; }
    int tier() const { return mode & 0xff; }
    // the roundings this call gives up, as RELAX_* bits for the layer launchers (0 = strict)
    int relax() const
    {
        switch (mode & 0xff) {
        case SRCNN_MODE_STRICT: return 0;
        case SRCNN_MODE_RELAXED: return (mode >> 8) & 0xf;
        default: return RELAX_FAST;
        }
    }
};

struct StageSpan { Event a, b; int stage; };

struct StreamSlot {         // one lane of the host-stream path; lives until srcnn_shutdown
    Stream st;                         // kernels (slot 0's stream carries the kernels of BOTH slots)
    Stream cst;                        // this slot's copies, in both directions
    Event e_in, e_k, e_out;            // frame landed / kernels done / result copied out
    DevBuf<float> din, dout;
    Workspace ws;                      // private: the captured graph has its pointers baked in
    std::vector<TableRef> tables;      // references taken by eager runs (trimmed by the runs themselves)
    struct Frozen {                    // retired as one: graph = {} (and ws.frozen = false)
        GraphExec exec;                // captured kernel sequence for (gw, gh, gmode)
        std::vector<TableRef> tables;  // references baked into `exec`: live exactly as long as the graph
    } graph;
    unsigned gw = 0, gh = 0; int gmode = -1;
    unsigned uses = 0;                 // eager runs at the current shape (capture needs one first)
    int graph_verdict = 0;             // use_graph == 1 ("auto"): 0 = not measured yet, 1 = replay is cheap, 2 = replay burns host CPU: plain launches
};

// One lane of srcnn_process_u8 (the ProcessSRCNN surface).  The reference's ProcessSRCNN allocates everything per
// call and is therefore re-entrant (src/libsrcnn.cpp:628-923); here a call leases a lane -- its own compute and
// copy streams, scratch, page-locked staging and events -- on every context it uses, for its whole duration, so
// concurrent calls from several host threads never share a buffer.  Lanes are created on demand up to kMaxLanes per
// context; further callers wait for one.
struct ProcLane {
    bool busy = false;
    Stream st, copy_st, in_st;                // kernels / results out (D2H) / source rows in (H2D)
    Workspace ws;
    struct Staging { PinnedBuf in, out; } pin;
    std::vector<Event> band_events;           // per band: kernels done, result landed, source rows in
    void trim() { ws.clear(); pin = {}; }     // an idle lane gives its memory back (the caller has waited for its streams)
};
constexpr size_t kDefaultMaxLanes = 4;   // per context; env SRCNN_MAX_LANES (1..64) overrides
constexpr unsigned kClockSlots = 8192;   // layer-1+2 launches the clock probe can hold before it wraps
constexpr size_t kMaxTables = 64;      // cache bound per context; only unreferenced tables are ever evicted

// Per-context buffers of the node-level tiled frame (srcnn_y_upscale2x_f32_node_dev): the slab of the source frame this
// context's band reads, and the band it produces before it is copied to the root device.
struct NodeLane {
    Stream st, copy_st;
    Workspace ws;
    DevBuf<float> in, band;
    std::vector<Event> events;
};

// Pageable host memory never goes to a HIP copy.  Above 128 KB the runtime pins the caller's pages IN PLACE for the transfer
// (a userptr mapping, 32 MB at a time); when the range lies in the malloc heap and the C library trims that heap -- any free()
// on any thread can -- the mapping is invalidated under the copy engine and the process dies with "Memory access fault by GPU
// ... on address <a heap address>" (round 6: the GPU suite, 4 runs of 4, until MALLOC_TRIM_THRESHOLD_ was raised).  So every
// copy between the device and memory the library did not page-lock itself bounces through these two page-locked slots:
// memcpy + DMA, double-buffered, at memcpy speed -- which is what the runtime's own staging path costs too.
struct HostBounce {
    std::mutex mu;                      // one bounced copy at a time per context
    struct Slots {                      // srcnn_trim: s = {}
        GrowBuf<unsigned char, BounceAlloc> pin;   // 2 slots, allocated on first use.  A slot grows with the largest copy seen,
                                        // 1 MB ... kSlot: page-locking 32 MB costs 5-80 ms, and the first copy of a process is the
                                        // 50 KB weight image of srcnn_init
        Event ev[2];
    } s;
    size_t slot() const { return s.pin.size() / 2; }
    static constexpr size_t kSlot = 16u << 20;
};
// device buffers of the host-pointer convenience calls (srcnn_y_path_f32 and what is built on it): grow-only; a call holds
// `mu` from its H2D to its D2H, so such calls are serialised per context (they shared the NULL stream before as well)
struct HostCallBuffers {
    std::mutex mu;
    struct Bufs { DevBuf<float> in, out; } d;      // srcnn_trim: d = {}
};

struct Ctx {
    int index = 0;          // position in Global::ctxs
    int device = 0;         // physical HIP device
    int numa_node = -1;     // host NUMA node next to the device (-1: unknown)
    std::mutex mu;          // tables, ws map, spans, event pool
    std::vector<StageSpan> spans;          // recorded, not yet read
    std::vector<Event> event_pool;         // recycled events
    double stage_ms[SRCNN_STAGE_COUNT] = {0, 0, 0};
    unsigned long long stage_n[SRCNN_STAGE_COUNT] = {0, 0, 0};
    int num_cus = 256;
    // raw like Workspace::queue, and for the same reason (run_conv12 reads it): freed by ~Ctx
    unsigned long long* clock_buf = nullptr;   // srcnn_debug_clock_probe: kClockSlots x (cycles, ticks), one slot per conv12 launch
    std::atomic<unsigned> clock_n{0};
    DevBuf<FusedF16Weights> fused_w;      // device copy of the fused fp16 kernel's weight image
    std::map<std::tuple<int, unsigned, unsigned>, TableRef> tables;
    unsigned long long table_clock = 0;
    std::map<hipStream_t, std::unique_ptr<Workspace>> ws;
    StreamSlot slots[2];
    std::mutex stream_mu;               // the host-stream path is serialised per context
    std::mutex lane_mu;                 // ProcessSRCNN lanes
    std::condition_variable lane_cv;
    std::vector<std::unique_ptr<ProcLane>> lanes;
    std::mutex node_mu;                 // the node-level tiled frame is serialised per context
    NodeLane node;
    HostBounce bounce;
    HostCallBuffers host_call;
    ~Ctx() { (void)hipFree(clock_buf); }
};

struct Global {
    std::mutex mu;                                   // guards ctxs (creation / shutdown) and stream_ctx
    std::vector<std::unique_ptr<Ctx>> ctxs;
    std::atomic<int> nctx{0};                        // == ctxs.size(), readable without the lock
    std::map<hipStream_t, int> stream_ctx;           // streams made by srcnn_stream_create -> owning context
    std::atomic<bool> profiling{false};
    std::atomic<bool> clock_probe{false};            // srcnn_debug_clock_probe
    std::atomic<int> mode{SRCNN_MODE_STRICT};        // as Call::mode (tier in the low byte, relaxation mask above it)
    std::atomic<unsigned> relax_mask{SRCNN_RELAX_L3_X64};   // what SRCNN_MODE_RELAXED relaxes (srcnn_set_relaxation)
    std::atomic<size_t> ws_budget;
    size_t max_lanes = kDefaultMaxLanes;   // concurrent ProcessSRCNN calls per context before callers queue
    Global();
};
extern Global& G;

// ---- tracing: named ranges for rocprofv3 --marker-trace (the reference only has a wall-clock ms counter) ----
// Off unless SRCNN_ROCTX=1: then librocprofiler-sdk-roctx is dlopen'ed once and every ProcessSRCNN call, band and stage of the
// path pushes / pops a range, so a marker trace shows the host-side pipeline next to the kernels.
class TraceRange {
public:
    explicit TraceRange(const char* fmt, ...) __attribute__((format(printf, 2, 3)));
    ~TraceRange();
    TraceRange(const TraceRange&) = delete;
    TraceRange& operator=(const TraceRange&) = delete;
private:
    bool on_;
};

// RAII bracket: records an event pair around one stage on the launch stream when profiling is on.
struct StageTimer {
    Ctx& cx; hipStream_t s; int stage; Event a, b; bool on;
    Event take()
    {
        Event e;
        if (!cx.event_pool.empty()) { e = std::move(cx.event_pool.back()); cx.event_pool.pop_back(); }
        else if (hipEventCreate(e.put()) != hipSuccess) e.reset();
        return e;
    }
    StageTimer(int stage_, const Call& c) : cx(*c.cx), s(c.s), stage(stage_), on(c.timing && G.profiling.load(std::memory_order_relaxed))
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(cx.mu);
        a = take(); b = take();
        if (!a || !b) { on = false; return; }
        (void)hipEventRecord(a.get(), s);
    }
    ~StageTimer()
    {
        if (!on) return;
        (void)hipEventRecord(b.get(), s);
        std::lock_guard<std::mutex> lk(cx.mu);
        cx.spans.push_back(StageSpan{std::move(a), std::move(b), stage});
    }
};

// ---- contexts ----
int ensure_init();                       // at least context 0 exists (lazy: device 0, or env SRCNN_DEVICES)
Ctx* cur_ctx();                          // the calling thread's current context, device bound; nullptr + error if init fails
Ctx* ctx_for_stream(void* stream);       // the context that owns `stream` (srcnn_stream_create), else the current one
int bind(Ctx& cx);                       // hipSetDevice(cx.device) for the calling thread
int context_count();
Ctx* context_at(int k);

// ---- scratch / tables ----
int get_table(Call& c, int filter, unsigned dst_len, unsigned src_len, TableRef& out);
Workspace* workspace_for(Ctx& cx, hipStream_t s);
bool pinned_by_library(const void* p, size_t n);   // [p, p+n) lies inside a block from srcnn_host_alloc_pinned
bool host_is_page_locked(const void* p, size_t n); // [p, p+n) is hipHostMalloc / hipHostRegister memory (asks the runtime about both ends)
// Blocking copies between device memory and ANY host memory (see HostBounce): page-locked host memory goes straight to the copy
// engine, everything else through the context's bounce slots.  `after` (may be NULL): work already queued on that stream
// is finished first, so the call is ordered on it like the hipMemcpyAsync it replaces.
int copy_h2d_any(Ctx& cx, void* d_dst, const void* h_src, size_t bytes, hipStream_t after);
int copy_d2h_any(Ctx& cx, void* h_dst, const void* d_src, size_t bytes, hipStream_t after);

// An eager call on a caller-visible stream: the stream's own scratch, locked while this call enqueues.
struct StreamCall {
    std::vector<TableRef> tables;
    Call c;
    std::unique_lock<std::mutex> lk;
    int rc = SRCNN_OK;
    explicit StreamCall(void* stream)
    {
        c.cx = ctx_for_stream(stream);
        if (!c.cx) { rc = SRCNN_E_NODEVICE; return; }
        c.s = (hipStream_t)stream;
        c.ws = workspace_for(*c.cx, c.s);
        c.mode = G.mode.load();
        c.hold = &tables;
        lk = std::unique_lock<std::mutex>(c.ws->mu);
    }
};

// ---- the path (srcnn_capi.cpp) ----
int check_plane(const void* in, unsigned w, unsigned h, const void* out);
int check_y_path_args(const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const float* d_out);
int resample_rows_range(Call& c, const float* d_in, unsigned sw, unsigned sh, unsigned dw, unsigned dh, int filter,
                        unsigned r0, unsigned r1, float* d_dst);
int y_path_rows(Call& c, const YSource& src, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                unsigned r0, unsigned r1, float* d_out);
int y_path_range(Call& c, const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                 unsigned r0, unsigned r1, float* d_out);
int y_path_frame(Call& c, const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, float* d_out);
// Output samples [x0,x1) x [y0,y1) of the (dw x dh) result only, at the cost of a window around them.  in_stride / out_stride
// are in floats; d_out is where sample (x0, y0) goes.  d_in begins at sample (in_x0, in_y0) of the w x h plane and holds at least
// the rect's source rectangle; whole_plane: it holds all h rows of the plane.
int y_path_rect(Call& c, const float* d_in, size_t in_stride, unsigned in_x0, unsigned in_y0, unsigned w, unsigned h, unsigned dw,
                unsigned dh, int filter, unsigned x0, unsigned y0, unsigned x1, unsigned y1, float* d_out, size_t out_stride,
                bool whole_plane = true);
// what the rect entry points refuse about the geometry, in the order include/srcnn_amd_rect.h gives, and the Y path's size limits
int check_rect_geometry(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned x0, unsigned y0, unsigned rw, unsigned rh);
int check_rect_limits(unsigned w, unsigned h, unsigned dw, unsigned dh, unsigned rh);
// layers 1+2 over rows of a (W x H) plane, as every path launches them (kernel instance, tile queue of the workspace, clock probe)
void run_conv12(const Call& c, const float* Y, int W, int H, int y_row_base, int y_rows, float* C2, size_t plane, int row0, int rows);
// rows of `rows` one pass of the Y path produces over a window W floats wide (y_path_band_rows under the workspace budget): the
// band y_path_range (W = dw) and y_path_rect (W = the width of the rect's halo) cut their ranges into
unsigned y_path_pass_rows(const Call& c, unsigned W, unsigned rows);
// Columns [c0,c1) x rows [r0,r1) of the resampled (dw x dh) plane, tight, at the cost of that window, with the bits of
// resample_rows_range; d_in (in_stride floats per row) begins at sample (in_x0, in_y0) of the sw x sh source plane.
int resample_window(Call& c, const float* d_in, size_t in_stride, unsigned in_x0, unsigned in_y0, unsigned sw, unsigned sh,
                    unsigned dw, unsigned dh, int filter, unsigned c0, unsigned c1, unsigned r0, unsigned r1, float* d_dst);
// The RGB(A) rect call behind srcnn_rgb_upscale_rect_dev (srcnn_frames.cpp), arguments checked (srcnn_frame_args.hpp): output
// pixels [x0,x1) x [y0,y1) into out[] and conv, the rect's own planes; conv.lo == NULL: no truncated Y' plane.
struct RgbRule;
struct YuvPlane;
int rgb_rect(Call& c, const RgbRule& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const YuvPlane in[4],
             const YuvPlane out[4], const YuvPlane& conv, unsigned x0, unsigned y0, unsigned x1, unsigned y1);
// The YUV rect call behind srcnn_yuv_upscale_rect_dev (srcnn_frames.cpp), arguments checked: the luma rect [x0,x1) x [y0,y1) and
// the chroma samples that cover it into out[], the rect's own planes.
struct YuvGeom;
int yuv_rect(Call& c, const YuvGeom& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const YuvPlane in[3],
             const YuvPlane out[3], unsigned x0, unsigned y0, unsigned x1, unsigned y1);
// The packed YUV rect call behind srcnn_yuv_packed_upscale_rect_dev (srcnn_frames.cpp), arguments checked: luma columns [x0,x1)
// (under the unit rule) of rows [y0,y1) into out, the rect's own row segments of out.row_bytes bytes.
struct YuvPackedGeom;
int yuv_packed_rect(Call& c, const YuvPackedGeom& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const YuvPlane& in,
                    const YuvPlane& out, unsigned x0, unsigned y0, unsigned x1, unsigned y1);
// (axis_source_span, the source span of a range of an axis without a device, is srcnn_rect_source.hpp)
// source rows [lo, hi) of a (w x h) plane that output rows [r0, r1) of the Y path (resample + 3 layers) depend on
int y_path_source_rows(Call& c, unsigned h, unsigned dh, int filter, unsigned r0, unsigned r1, unsigned& lo, unsigned& hi);
// rows of layer-2 scratch one band may hold under the workspace budget (>= 16), for a dw-wide output
unsigned budget_band_rows(unsigned dw);
// cut [R0,R1) into pieces of about frac[i] of the range, each moved to where it fills whole rounds of the layer-1+2 grid
std::vector<unsigned> plan_cuts(unsigned R0, unsigned R1, unsigned dw, unsigned dh, const double* frac, int nfrac, int grid, int tile_rows);
// pieces of one rank's band of a tiled 2x frame (srcnn_tiled_piece): cut points, first = band start, last = band end
std::vector<unsigned> tiled_cuts(unsigned out_w, unsigned out_h, int rank, int nranks, int npieces);

// memcpy split over a few host threads: the destination is usually a fresh new[] block whose pages fault in on first
// touch, which a single thread does at only a few GB/s.
void parallel_memcpy(void* dst, const void* src, size_t n);
void async_chain_reset();     // srcnn_shutdown: forget the chain links of asynchronous ProcessSRCNN jobs (they own events)

// Host waits.  On this runtime hipEventSynchronize / hipStreamSynchronize hold a core at 100 % for the whole wait, whatever the
// event's flags -- hipEventBlockingSync included; only the process-wide hipDeviceScheduleBlockingSync changes that, and that
// flag is the host application's to set (tools/ubench/wait_cost.hip, profiles/r03_wait_cost.txt: a 5 ms wait costs 5.0 ms of
// CPU either way, 0.03 ms when polled).  The library's threads wait for milliseconds at a time, several of them per call, so
// they poll: a burst of queries for waits that are (almost) over, then sleep-and-query in 20..100 us naps.
// SRCNN_SPIN_WAIT=1 restores the runtime's own waits (A/B runs).
// query_guard: held around every query.  A thread that captures a stream into a graph takes the same mutex for the span of
// the capture: an event query that lands inside another thread's capture of the stream the event belongs to ends that capture.
hipError_t wait_event(hipEvent_t e, std::mutex* query_guard = nullptr);
hipError_t wait_stream(hipStream_t s);

// An ordered hand-off between a producer and ONE consumer thread (replaces the round-2 yield() spin loops): the producer
// publishes "items [0, n) are ready", the consumer blocks in wait_for(i) until item i is ready or the hand-off is
// cancelled.  Nobody spins.
class Handoff {
public:
    void publish(unsigned n) { { std::lock_guard<std::mutex> lk(m_); ready_ = n; } cv_.notify_all(); }
    void cancel() { { std::lock_guard<std::mutex> lk(m_); cancelled_ = true; } cv_.notify_all(); }
    bool wait_for(unsigned i)
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return ready_ > i || cancelled_; });
        return ready_ > i;
    }
private:
    std::mutex m_;
    std::condition_variable cv_;
    unsigned ready_ = 0;
    bool cancelled_ = false;
};

// Lease of one ProcessSRCNN lane of a context for the duration of a call.
struct LaneLease {
    Ctx* cx = nullptr;
    ProcLane* lane = nullptr;
    int rc = SRCNN_OK;
    explicit LaneLease(Ctx& cx);
    ~LaneLease();
    LaneLease(const LaneLease&) = delete;
    LaneLease& operator=(const LaneLease&) = delete;
};

}  // namespace srcnn
