// srcnn_capi.cpp -- the extern "C" boundary (include/srcnn_amd.h) over the gfx950 kernels: contexts, plumbing and the
// device-resident hot path.  The host-pointer pipelines (frame stream, ProcessSRCNN surface, node-level calls) are in
// srcnn_pipeline.cpp, the YUV / RGB frame calls around the Y path in srcnn_frames.cpp; the state all share is srcnn_host.hpp.
//
// Host-side orchestration only: argument validation with the reference's return codes
// (src/libsrcnn.cpp:951-966), lazily built + cached contribution tables
// (src/frawscale.cpp:8-112 -> resample_table.hpp), grow-only per-stream device workspaces, and the
// launch sequence that stands in for the body of libsrcnn::doSRCNN (src/libsrcnn.cpp:628-923).
// There is deliberately no CPU compute path in this file: if HIP is unusable the calls fail.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <sys/prctl.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "resample_table.hpp"
#include <chrono>
#include <sys/auxv.h>
#include <unistd.h>

#include "../../include/srcnn_amd_rect.h"
#include "srcnn_frame_args.hpp"
#include "srcnn_host.hpp"
#include "srcnn_rect_source.hpp"
#include "srcnn_window.h"

namespace srcnn {

namespace {
thread_local char g_err[512] = "";
thread_local int t_ctx = 0;            // the calling thread's current context (srcnn_set_context)
}  // namespace

void set_last_error(const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); }
const char* last_error() { return g_err; }

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        if (!settings().roctx) return;
        void* h = nullptr;
        for (const char* n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) push = nullptr;
    }
};
const Roctx& roctx() { static const Roctx r; return r; }
}  // namespace

TraceRange::TraceRange(const char* fmt, ...) : on_(roctx().push != nullptr)
{
    if (!on_) return;
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (void)roctx().push(buf);
}

TraceRange::~TraceRange() { if (on_) (void)roctx().pop(); }

// ---- settings: every SRCNN_* switch, read once (srcnn_settings.hpp) ----
Settings Settings::from_env()
{
    Settings st;
    // A switch that is set but not understood used to be dropped in silence (SRCNN_TRACE=yes read as 0; a retired switch of an
    // earlier round measured the production path and reported it as a variant): every such case is now said once, on stderr.
    auto warn = [](const char* fmt, const char* a, const char* b) { fprintf(stderr, fmt, a, b); };
    auto get = [](const char* name) -> const char* { const char* v = getenv(name); return (v && *v) ? v : nullptr; };
    auto parse_b = [&](const char* env, const char* v, bool& dst) {
        for (const char* t : {"1", "true", "yes", "on", "TRUE", "YES", "ON"}) if (!strcmp(v, t)) { dst = true; return; }
        for (const char* t : {"0", "false", "no", "off", "FALSE", "NO", "OFF"}) if (!strcmp(v, t)) { dst = false; return; }
        char* end = nullptr;
        const long n = strtol(v, &end, 10);
        if (end != v && *end == 0) { dst = n != 0; return; }
        warn("libsrcnn_amd: %s=%s is not a boolean (0/1, yes/no, on/off, true/false): the default stays\n", env, v);
    };
    auto parse_i = [&](const char* env, const char* v, long& dst) {
        char* end = nullptr;
        const long n = strtol(v, &end, 10);
        if (end != v && *end == 0) dst = n;
        else warn("libsrcnn_amd: %s=%s is not an integer: the default stays\n", env, v);
    };
    // SRCNN_RCCL_LIB names code to load into the process: like LD_PRELOAD it is not honoured under secure execution
    const bool secure = getauxval(AT_SECURE) != 0;
#define SRCNN_GET_B(m) parse_b(name, v, st.m);
#define SRCNN_GET_I(m) parse_i(name, v, st.m);
#define SRCNN_GET_S(m) if (secure && !strcmp(name, "SRCNN_RCCL_LIB")) warn("libsrcnn_amd: %s=%s ignored: secure-execution (set-uid / set-gid / capabilities) process\n", name, v); else st.m = v;
#define X(kind, member, env, def, values, effect) if (const char* v = get(env)) { const char* name = env; (void)name; SRCNN_GET_##kind(member) }
    SRCNN_SETTINGS(X)
#undef X
#undef SRCNN_GET_B
#undef SRCNN_GET_I
#undef SRCNN_GET_S
    // anything else that looks like one of ours: said once (names the tests, the bench and the build recipes use are not switches
    // of the library and pass)
    for (char** e = environ; e && *e; ++e) {
        if (strncmp(*e, "SRCNN_", 6) != 0) continue;
        const char* eq = strchr(*e, '=');
        const std::string name(*e, eq ? (size_t)(eq - *e) : strlen(*e));
        bool known = false;
#define X(kind, member, env, def, values, effect) if (name == env) known = true;
        SRCNN_SETTINGS(X)
#undef X
        if (known || name == "SRCNN_TEST_SEED" || name == "SRCNN_AMD_LIB" || name == "SRCNN_FUSED_CFLAGS" || name.rfind("SRCNN_BENCH_", 0) == 0) continue;
        warn("libsrcnn_amd: %s is not a switch of this library (see srcnn_debug_settings / DESIGN.md 6)%s: ignored\n", name.c_str(), "");
    }
    st.max_workspace_mb = std::max(st.max_workspace_mb, 1L);
    st.max_lanes = std::min(64L, std::max(1L, st.max_lanes));
    st.comm_timeout_ms = std::max(0L, st.comm_timeout_ms);
    st.prefault_threads = std::max(1L, st.prefault_threads);
    st.rs_tpb = std::min(16L, std::max(0L, st.rs_tpb));
    st.async_chain = std::min(2L, std::max(0L, st.async_chain));
    return st;
}

std::string Settings::describe(bool markdown) const
{
    std::string out;
    char line[768];
    auto val_b = [](bool b) { return std::string(b ? "1" : "0"); };
    auto val_i = [](long i) { return std::to_string(i); };
    auto val_s = [](const std::string& t) { return t.empty() ? std::string("(unset)") : t; };
    const Settings defaults;
#define SRCNN_VAL_B(m) val_b(m)
#define SRCNN_VAL_I(m) val_i(m)
#define SRCNN_VAL_S(m) val_s(m)
#define X(kind, member, env, def, values, effect)                                                                                 \
    if (markdown) snprintf(line, sizeof line, "| `%s` | **%s**; %s | %s |\n", env, SRCNN_VAL_##kind(defaults.member).c_str(), values, effect); \
    else snprintf(line, sizeof line, "%s=%s (default %s)  -- %s\n", env, SRCNN_VAL_##kind(member).c_str(), SRCNN_VAL_##kind(defaults.member).c_str(), effect); \
    out += line;
    SRCNN_SETTINGS(X)
#undef X
#undef SRCNN_VAL_B
#undef SRCNN_VAL_I
#undef SRCNN_VAL_S
    return out;
}

const Settings& settings()
{
    static const Settings* st = new Settings(Settings::from_env());      // (never destroyed, like Global)
    return *st;
}

Global::Global()
{
    const Settings& st = settings();
    ws_budget.store((size_t)st.max_workspace_mb << 20);
    max_lanes = (size_t)st.max_lanes;
}

// Never destroyed: at process exit the HIP runtime may already be gone when static destructors run, and the
// tables' destructors call hipFree.  srcnn_shutdown() is the orderly way to release everything.
Global& G = *new Global;

namespace {

const uint32_t kWeightBits[kWeightCount] = {
#include "srcnn_weights.inc"
};

// w: 8129 floats in the blob order b1, W1, b2, W2, b3, W3 -- the product's, or a caller's (srcnn_debug_fused_f16)
void build_dev_weights(DevWeights& d, const float* w = reinterpret_cast<const float*>(kWeightBits))
{
    const float* b1 = w;
    const float* w1 = b1 + 64;          // [k][i][j]      (src/convdata.h:32-674)
    const float* b2 = w1 + 64 * 81;
    const float* w2 = b2 + 32;          // [m][f]         (src/convdata.h:686-976)
    const float* b3 = w2 + 32 * 64;
    const float* w3 = b3 + 1;           // [m][x][y], x = column offset (src/libsrcnn.cpp:512)
    memset(&d, 0, sizeof d);
    for (int k = 0; k < 64; ++k) {
        d.b1[k] = b1[k];
        for (int t = 0; t < 81; ++t) d.w1t[t][k] = w1[k * 81 + t];
    }
    for (int m = 0; m < 32; ++m) {
        d.b2[m] = b2[m];
        for (int f = 0; f < 64; ++f) d.w2[m][f] = w2[m * 64 + f];
        for (int dy = 0; dy < 5; ++dy)
            for (int dx = 0; dx < 5; ++dx) d.w3[m][dy * 5 + dx] = w3[m * 25 + dx * 5 + dy];
        for (int dy = 0; dy < 5; ++dy)
            for (int dx = 0; dx < 6; ++dx) d.w3p[m * 30 + dy * 6 + dx] = dx < 5 ? d.w3[m][dy * 5 + dx] : 0.f;
    }
    d.b3 = *b3;
}

// fp32 -> (hi, lo) fp16 bit patterns of v * 2^8, the same split the device uses for activations
void split_f16_bits(float v, unsigned short& hi, unsigned short& lo)
{
    const _Float16 h = (_Float16)(v * 256.f);
    const _Float16 l = (_Float16)(v * 256.f - (float)h);
    memcpy(&hi, &h, 2);
    memcpy(&lo, &l, 2);
}

[[maybe_unused]] void build_fused_f16_weights(const DevWeights& d, FusedF16Weights& f)
{
    memset(&f, 0, sizeof f);
    for (int s = 0; s < FU_NK; ++s)
        for (int blk = 0; blk < 2; ++blk)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int ch = 32 * blk + (l & 31), h = l >> 5;
                    int dy = -1, dx = -1;                      // tap carried by this slot (none: weight 0)
                    if (s < 4) { dy = 2 * s + h; dx = j; }
                    else { if (h == 0) { dy = 8; dx = j; } else { dy = j; dx = 8; } }
                    const float w = dy >= 0 ? d.w1t[dy * 9 + dx][ch] : 0.f;
                    split_f16_bits(w, f.w1[s][blk][0][l][j], f.w1[s][blk][1][l][j]);
                }
    for (int blk = 0; blk < 2; ++blk)
        for (int ks = 0; ks < 2; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int m = l & 31, h = l >> 5;
                    const int c = 32 * blk + 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3);
                    split_f16_bits(d.w2[m][c], f.w2[blk][ks][0][l][j], f.w2[blk][ks][1][l][j]);
                }
    for (int ks = 0; ks < 2; ++ks)
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
                const int t = l & 31, h = l >> 5;
                const int m = 16 * ks + 8 * (j >> 2) + 4 * h + (j & 3);
                split_f16_bits(t < 25 ? d.w3[m][t] : 0.f, f.w3[ks][0][l][j], f.w3[ks][1][l][j]);
            }
    for (int hf = 0; hf < 2; ++hf) {
        for (int r = 0; r < 32; ++r) f.b1[hf * 32 + r] = 256.f * d.b1[32 * (r >> 4) + 8 * ((r & 15) >> 2) + 4 * hf + (r & 3)];
        for (int r = 0; r < 16; ++r) f.b2[hf * 16 + r] = 256.f * d.b2[8 * (r >> 2) + 4 * hf + (r & 3)];
        for (int r = 0; r < 32; ++r) f.w88[hf * 32 + r] = 256.f * d.w1t[80][32 * (r >> 4) + 8 * ((r & 15) >> 2) + 4 * hf + (r & 3)];
    }
    f.b3 = d.b3;
}


// Host NUMA node next to a device: /sys/bus/pci/devices/<bdf>/numa_node (-1 when the platform does not say).
int device_numa_node(int device)
{
    char bdf[64] = "";
    if (hipDeviceGetPCIBusId(bdf, sizeof bdf, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char* p = bdf; *p; ++p) *p = (char)tolower(*p);
    const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/numa_node";
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

// Create and initialise one context on `device` (caller holds G.mu).
int make_context_locked(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(SRCNN_E_NODEVICE, "no HIP device visible (%s); this library has no CPU path",
                    e == hipSuccess ? "count=0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(SRCNN_E_ARG, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SRCNN_E_NODEVICE, "device %d is %s; this build only carries gfx950 code", device, prop.gcnArchName);
    auto cx = std::make_unique<Ctx>();
    cx->index = (int)G.ctxs.size();
    cx->device = device;
    cx->num_cus = prop.multiProcessorCount;
    cx->numa_node = device_numa_node(device);      // (before the first bounced copy: the bounce slots are placed by it)
    // Not published yet: every failure below destroys it with all it has acquired by then, bounce slots included.
    // SRCNN_TRACE: where the time of creating a context goes (the first one also pays for loading the code object)
    const auto tr0 = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what) {
        if (settings().trace)
            fprintf(stderr, "srcnn_init ctx %d: %-28s at %7.2f ms\n", cx->index, what,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count());
    };
    // __constant__ weights, the kernels' dynamic-LDS attributes and the fused tier's weight image are per DEVICE; a second
    // (virtual) context on the same device re-uploads identical bytes
    auto dw = std::make_unique<DevWeights>();
    build_dev_weights(*dw);
    stamp("weights built on the host");
    HIP_TRY(upload_weights(*dw));
    stamp("weights uploaded (module load)");
    HIP_TRY(conv12_mfma_prepare());
    stamp("layer-1+2 kernel attributes");
#ifndef SRCNN_STRICT_ONLY
    auto fw = std::make_unique<FusedF16Weights>();
    build_fused_f16_weights(*dw, *fw);
    if (cx->fused_w.grow(1)) return fail(SRCNN_E_HIP, "hipMalloc of the fp16 tier's weight image failed");
    stamp("fp16 tier weights built");
    if (int rc = copy_h2d_any(*cx, cx->fused_w.data(), fw.get(), sizeof(FusedF16Weights), nullptr)) return rc;
    stamp("fp16 tier weights uploaded");
    HIP_TRY(fused_f16_prepare());
    stamp("fp16 tier kernel attributes");
    HIP_TRY(rs2d_prepare());
    stamp("resampler kernel attributes");
#else
    HIP_TRY(rs2d_prepare());
    stamp("resampler kernel attributes");
#endif
    // direct copies between the devices of a node (the node-level tiled frame moves its bands with hipMemcpyPeerAsync)
    for (auto& other : G.ctxs) {
        if (other->device == device) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device, other->device) == hipSuccess && can) {
            (void)hipSetDevice(device); (void)hipDeviceEnablePeerAccess(other->device, 0);
            (void)hipSetDevice(other->device); (void)hipDeviceEnablePeerAccess(device, 0);
            (void)hipGetLastError();               // "already enabled" is fine
            (void)hipSetDevice(device);
        }
    }
    G.ctxs.push_back(std::move(cx));
    G.nctx.store((int)G.ctxs.size());
    return SRCNN_OK;
}

// env SRCNN_DEVICES for a process that never calls srcnn_init*: "all", or a comma list of device ids (an id may repeat:
// virtual contexts on one device).  Unset: device 0.
int lazy_init_locked()
{
    if (!G.ctxs.empty()) return SRCNN_OK;
    const char* env = settings().devices.c_str();
    std::vector<int> devs;
    if (*env) {
        if (strcmp(env, "all") == 0) {
            int n = 0;
            if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
            for (int d = 0; d < n; ++d) devs.push_back(d);
        } else {
            for (const char* p = env; *p;) {
                char* end = nullptr;
                const long v = strtol(p, &end, 10);
                if (end == p) return fail(SRCNN_E_ARG, "SRCNN_DEVICES=%s: expected \"all\" or a comma list of device ids", env);
                devs.push_back((int)v);
                p = (*end == ',') ? end + 1 : end;
            }
        }
    }
    if (devs.empty()) devs.push_back(0);
    for (int d : devs) {
        int rc = make_context_locked(d);
        if (rc) return rc;
    }
    return SRCNN_OK;
}

}  // namespace

int ensure_init()
{
    if (G.nctx.load(std::memory_order_acquire) > 0) return SRCNN_OK;
    std::lock_guard<std::mutex> lk(G.mu);
    return lazy_init_locked();
}

int context_count() { return G.nctx.load(std::memory_order_acquire); }

Ctx* context_at(int k)
{
    std::lock_guard<std::mutex> lk(G.mu);
    return (k >= 0 && k < (int)G.ctxs.size()) ? G.ctxs[k].get() : nullptr;
}

int bind(Ctx& cx)
{
    hipError_t e = hipSetDevice(cx.device);
    if (e != hipSuccess) return fail(SRCNN_E_HIP, "hipSetDevice(%d) -> %s", cx.device, hipGetErrorString(e));
    return SRCNN_OK;
}

Ctx* cur_ctx()
{
    if (ensure_init()) return nullptr;
    Ctx* cx = context_at(t_ctx);
    if (!cx) cx = context_at(0);
    if (!cx) { fail(SRCNN_E_NODEVICE, "no context"); return nullptr; }
    if (bind(*cx)) return nullptr;                 // a thread other than the one that called srcnn_init still needs the device selected
    return cx;
}

Ctx* ctx_for_stream(void* stream)
{
    if (ensure_init()) return nullptr;
    Ctx* cx = nullptr;
    if (stream) {
        std::lock_guard<std::mutex> lk(G.mu);
        auto it = G.stream_ctx.find((hipStream_t)stream);
        if (it != G.stream_ctx.end() && it->second < (int)G.ctxs.size()) cx = G.ctxs[it->second].get();
    }
    if (!cx) return cur_ctx();
    if (bind(*cx)) return nullptr;
    return cx;
}

// Look up / build / upload the contribution table of one axis.  The cache holds one reference, the caller gets
// another (and parks it in c.hold), and a table is only ever freed when nobody but the cache references it: a
// lookup can therefore never invalidate a table handed out earlier -- not the first of the two tables of a
// resample, not one another thread is about to launch with, not one baked into a captured graph.
int get_table(Call& c, int filter, unsigned dst_len, unsigned src_len, TableRef& out)
{
    Ctx& cx = *c.cx;
    std::lock_guard<std::mutex> lk(cx.mu);
    const auto key = std::make_tuple(filter, dst_len, src_len);
    auto it = cx.tables.find(key);
    if (it == cx.tables.end()) {
        const AxisTable t = build_axis_table(filter, dst_len, src_len);
        auto d = std::make_shared<DeviceTable>();
        d->stride = t.stride;
        d->max_taps = t.max_taps;
        d->src_len = src_len;
        d->h_first.assign(t.first.begin(), t.first.end());
        d->h_taps.assign(t.taps.begin(), t.taps.end());
        d->monotone = true;
        for (unsigned u = 1; u < dst_len; ++u)
            if (t.first[u] < t.first[u - 1] || t.first[u] + t.taps[u] < t.first[u - 1] + t.taps[u - 1]) { d->monotone = false; break; }
        if (d->first.grow(dst_len) || d->taps.grow(dst_len) || d->weight.grow(t.weight.size()))
            return fail(SRCNN_E_HIP, "hipMalloc of a contribution table (%u entries) failed", dst_len);
        // (heap vectors: through the bounce slots like every other pageable source -- a tall frame's weight table is 400 KB)
        if (int rc = copy_h2d_any(cx, d->first.data(), t.first.data(), sizeof(int) * dst_len, nullptr)) return rc;
        if (int rc = copy_h2d_any(cx, d->taps.data(), t.taps.data(), sizeof(int) * dst_len, nullptr)) return rc;
        if (int rc = copy_h2d_any(cx, d->weight.data(), t.weight.data(), sizeof(double) * t.weight.size(), nullptr)) return rc;
        if (cx.tables.size() >= kMaxTables) {
            // evict the least recently used tables that only the cache still references, down to half the bound.
            // Kernels launched by calls that already returned may still be reading them, hence the drain first.
            std::vector<std::pair<unsigned long long, std::tuple<int, unsigned, unsigned>>> idle;
            for (auto& kv : cx.tables)
                if (kv.second.use_count() == 1) idle.emplace_back(kv.second->stamp, kv.first);
            std::sort(idle.begin(), idle.end());
            if (!idle.empty()) (void)hipDeviceSynchronize();
            for (auto& e : idle) {
                if (cx.tables.size() < kMaxTables / 2) break;
                cx.tables.erase(e.second);
            }
        }
        it = cx.tables.emplace(key, std::move(d)).first;
    }
    it->second->stamp = ++cx.table_clock;
    out = it->second;
    if (c.hold) c.hold->push_back(out);
    return SRCNN_OK;
}

Workspace* workspace_for(Ctx& cx, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(cx.mu);
    auto& p = cx.ws[s];
    if (!p) p = std::make_unique<Workspace>();
    return p.get();
}

// Page-locked host memory for a context's staging: portable (every device of the node may DMA to it -- the node-level
// ProcessSRCNN shares one output staging), and placed on the NUMA node next to the device when the platform tells us
// which one that is (hipHostMallocNumaUser: the allocation follows the calling thread's memory policy, which is set to
// "prefer that node" around the call).  SRCNN_NUMA=0 disables the placement.
// The blocks handed out by srcnn_host_alloc_pinned: how srcnn_process_u8 recognises caller buffers it can copy from / into
// directly (asking the runtime about a pageable pointer works too, but logs an error line per question under AMD_LOG_LEVEL >= 1).
std::mutex g_pinned_mu;
std::map<uintptr_t, size_t>& pinned_blocks()
{
    static auto* m = new std::map<uintptr_t, size_t>;
    return *m;
}
bool pinned_by_library(const void* p, size_t n)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    auto& m = pinned_blocks();
    auto it = m.upper_bound(a);
    if (it == m.begin()) return false;
    --it;
    return a >= it->first && a + n <= it->first + it->second;
}

void* pinned_alloc(Ctx& cx, size_t bytes)
{
    void* p = nullptr;
    const bool want_place = settings().numa && cx.numa_node >= 0 && cx.numa_node < 1024;
    constexpr unsigned long kMaxNode = 1024;
    unsigned long mask[kMaxNode / (8 * sizeof(unsigned long))] = {0};
    // The policy is the CALLING thread's (an application thread inside ProcessSRCNN): whatever it was -- numactl --membind /
    // --interleave, or one the application set itself -- is read first and put back exactly; if it cannot be read, the
    // allocation is simply not placed.
    int saved_mode = 0;
    unsigned long saved_mask[kMaxNode / (8 * sizeof(unsigned long))] = {0};
    bool placed = false;
    if (want_place && syscall(SYS_get_mempolicy, &saved_mode, saved_mask, kMaxNode, nullptr, 0ul) == 0) {
        mask[cx.numa_node / (8 * sizeof(unsigned long))] |= 1ul << (cx.numa_node % (8 * sizeof(unsigned long)));
        placed = syscall(SYS_set_mempolicy, 1 /* MPOL_PREFERRED */, mask, kMaxNode) == 0;
    }
    unsigned flags = hipHostMallocPortable | (placed ? hipHostMallocNumaUser : 0u);
    if (hipHostMalloc(&p, bytes ? bytes : 1, flags) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
    }
    if (placed) {
        bool any = false;
        for (unsigned long m : saved_mask) any = any || m != 0;
        // MPOL_DEFAULT (and MPOL_LOCAL) take an empty node set; the others get the set they had
        if (syscall(SYS_set_mempolicy, saved_mode, any ? saved_mask : nullptr, any ? kMaxNode : 0ul) != 0)
            (void)syscall(SYS_set_mempolicy, 0 /* MPOL_DEFAULT */, nullptr, 0ul);
    }
    if (!p) fail(SRCNN_E_DEVMEM, "hipHostMalloc(%zu) failed", bytes);
    return p;
}

// The first AND the last byte: a buffer that is page-locked only in its front part (a registered block followed by pageable
// memory, a range registered in part) must not reach the runtime's in-place pinning path whole (HostBounce in srcnn_host.hpp).
bool host_is_page_locked(const void* p, size_t n)
{
    auto locked = [](const void* q) {
        hipPointerAttribute_t a;
        const bool yes = hipPointerGetAttributes(&a, q) == hipSuccess && a.type == hipMemoryTypeHost;
        (void)hipGetLastError();
        return yes;
    };
    return locked(p) && (n <= 1 || locked(static_cast<const unsigned char*>(p) + (n - 1)));
}

namespace {
int bounce_ready(Ctx& cx, HostBounce& b, size_t bytes)          // b.mu held; no copy of this context is in flight
{
    size_t want = 1u << 20;
    while (want < bytes && want < HostBounce::kSlot) want <<= 1;
    if (int rc = b.s.pin.grow(2 * want, cx)) return rc;
    for (Event& e : b.s.ev)
        if (!e) HIP_TRY(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    return SRCNN_OK;
}

// Waits, on every way out of a bounced copy, for the slot events recorded and not waited for yet: no return leaves DMA in
// flight on a slot that the next caller (b.mu is released on return) would overwrite.  A copy that succeeds has waited itself.
struct SlotGuard {
    HostBounce& b;
    bool pending[2] = {false, false};
    hipError_t record(int k, hipStream_t s) { const hipError_t e = hipEventRecord(b.s.ev[k].get(), s); pending[k] = e == hipSuccess; return e; }
    hipError_t wait(int k) { const bool was = pending[k]; pending[k] = false; return was ? wait_event(b.s.ev[k].get()) : hipSuccess; }
    ~SlotGuard() { for (int k = 0; k < 2; ++k) (void)wait(k); }
};
}  // namespace

// The bounced copies run on the stream the caller named (NULL: the default stream) -- NOT on a stream of their own: the
// runtime maps streams onto a handful of hardware queues, and one more stream per context made the frame stream's copy and
// kernel streams share a queue (host-stream rate 3.48 -> 3.05 GPix/s until it was taken out again, round 6).
int copy_h2d_any(Ctx& cx, void* d_dst, const void* h_src, size_t bytes, hipStream_t after)
{
    if (bytes == 0) return SRCNN_OK;
    if (pinned_by_library(h_src, bytes) || host_is_page_locked(h_src, bytes)) {
        if (after) HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, after));
        else HIP_TRY(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
        return SRCNN_OK;
    }
    HostBounce& b = cx.bounce;
    std::lock_guard<std::mutex> lk(b.mu);
    if (int rc = bounce_ready(cx, b, bytes)) return rc;
    const size_t SLOT = b.slot();
    unsigned char* const pin = b.s.pin.data();
    const unsigned char* src = static_cast<const unsigned char*>(h_src);
    unsigned char* dst = static_cast<unsigned char*>(d_dst);
    SlotGuard slots{b};
    for (size_t off = 0, i = 0; off < bytes; off += SLOT, ++i) {
        const int k = (int)(i & 1);
        const size_t len = std::min(SLOT, bytes - off);
        if (slots.wait(k) != hipSuccess) return fail(SRCNN_E_HIP, "bounced H2D copy failed");
        parallel_memcpy(pin + k * SLOT, src + off, len);
        HIP_TRY(hipMemcpyAsync(dst + off, pin + k * SLOT, len, hipMemcpyHostToDevice, after));
        HIP_TRY(slots.record(k, after));
    }
    for (int k = 0; k < 2; ++k)                      // the slots are free again (and the data is on the device) on return
        if (slots.wait(k) != hipSuccess) return fail(SRCNN_E_HIP, "bounced H2D copy failed");
    return SRCNN_OK;
}

int copy_d2h_any(Ctx& cx, void* h_dst, const void* d_src, size_t bytes, hipStream_t after)
{
    if (bytes == 0) return SRCNN_OK;
    if (pinned_by_library(h_dst, bytes) || host_is_page_locked(h_dst, bytes)) {
        if (after) HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, after));
        else HIP_TRY(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
        return SRCNN_OK;
    }
    HostBounce& b = cx.bounce;
    std::lock_guard<std::mutex> lk(b.mu);
    if (int rc = bounce_ready(cx, b, bytes)) return rc;
    const size_t SLOT = b.slot();
    unsigned char* const pin = b.s.pin.data();
    unsigned char* dst = static_cast<unsigned char*>(h_dst);
    const unsigned char* src = static_cast<const unsigned char*>(d_src);
    SlotGuard slots{b};
    // chunk i+1 is on the copy engine while chunk i is copied out of its slot
    const size_t nchunks = (bytes + SLOT - 1) / SLOT;
    auto queue = [&](size_t i) -> int {
        const int k = (int)(i & 1);
        const size_t off = i * SLOT, len = std::min(SLOT, bytes - off);
        HIP_TRY(hipMemcpyAsync(pin + k * SLOT, src + off, len, hipMemcpyDeviceToHost, after));
        HIP_TRY(slots.record(k, after));
        return SRCNN_OK;
    };
    if (int rc = queue(0)) return rc;
    for (size_t i = 0; i < nchunks; ++i) {
        const int k = (int)(i & 1);
        const size_t off = i * SLOT, len = std::min(SLOT, bytes - off);
        if (slots.wait(k) != hipSuccess) return fail(SRCNN_E_HIP, "bounced D2H copy failed");
        if (i + 1 < nchunks) { if (int rc = queue(i + 1)) return rc; }
        parallel_memcpy(dst + off, pin + k * SLOT, len);
    }
    return SRCNN_OK;
}

namespace {
// The naps are 20 us (50 us after the first 2 ms).  The kernel rounds a sleep up by the thread's timer slack, 50 us by default,
// which would make every nap 70+ us; the slack is lowered for the duration of the wait only and put back afterwards.
template <class Q>
hipError_t poll_until_ready(Q&& query)
{
    hipError_t r;
    for (int i = 0; i < 64; ++i)
        if ((r = query()) != hipErrorNotReady) return r;
    const int slack = prctl(PR_GET_TIMERSLACK);
    if (slack > 1000) (void)prctl(PR_SET_TIMERSLACK, 1000UL);
    for (int n = 0;; ++n) {
        std::this_thread::sleep_for(std::chrono::microseconds(n < 100 ? 20 : 50));
        if ((r = query()) != hipErrorNotReady) break;
    }
    if (slack > 1000) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)slack);
    return r;
}
bool spin_waits() { return settings().spin_wait; }
}  // namespace

hipError_t wait_event(hipEvent_t e, std::mutex* query_guard)
{
    if (spin_waits()) return hipEventSynchronize(e);
    const hipError_t r = poll_until_ready([&] {
        if (!query_guard) return hipEventQuery(e);
        std::lock_guard<std::mutex> lk(*query_guard);
        return hipEventQuery(e);
    });
    (void)hipGetLastError();               // the "not ready" answers are not errors
    return r;
}

hipError_t wait_stream(hipStream_t s)
{
    if (spin_waits()) return hipStreamSynchronize(s);
    const hipError_t r = poll_until_ready([&] { return hipStreamQuery(s); });
    (void)hipGetLastError();
    return r;
}

void parallel_memcpy(void* dst, const void* src, size_t n)
{
    const size_t kChunk = 4u << 20;
    unsigned nt = (unsigned)std::min<size_t>(8, n / kChunk);
    if (nt <= 1) { memcpy(dst, src, n); return; }
    std::vector<std::thread> th;
    const size_t per = ((n / nt) + 4095) & ~size_t(4095);
    size_t done = 0;                    // bytes handed to threads that actually started
    try {
        for (unsigned t = 1; t < nt; ++t) {
            const size_t off = (size_t)t * per;
            if (off >= n) break;
            const size_t len = std::min(per, n - off);
            th.emplace_back([=] { memcpy((char*)dst + off, (const char*)src + off, len); });
            done = off + len;
        }
    } catch (...) {                     // thread creation failed: the rest is copied here
        done = th.empty() ? 0 : done;
    }
    // this thread takes the first chunk (and whatever could not be handed out)
    memcpy(dst, src, std::min(per, n));
    const size_t covered = th.empty() ? std::min(per, n) : done;
    if (covered < n) memcpy((char*)dst + covered, (const char*)src + covered, n - covered);
    for (auto& t : th) t.join();
}

LaneLease::LaneLease(Ctx& c) : cx(&c)
{
    std::unique_lock<std::mutex> lk(c.lane_mu);
    for (;;) {
        for (auto& l : c.lanes)
            if (!l->busy) { lane = l.get(); break; }
        if (lane) break;
        if (c.lanes.size() < G.max_lanes) {
            auto l = std::make_unique<ProcLane>();
            if (hipStreamCreateWithFlags(l->st.put(), hipStreamNonBlocking) != hipSuccess ||
                hipStreamCreateWithFlags(l->copy_st.put(), hipStreamNonBlocking) != hipSuccess ||
                hipStreamCreateWithFlags(l->in_st.put(), hipStreamNonBlocking) != hipSuccess) {
                rc = fail(SRCNN_E_HIP, "could not create the streams of a ProcessSRCNN lane");
                return;
            }
            c.lanes.push_back(std::move(l));
            lane = c.lanes.back().get();
            break;
        }
        c.lane_cv.wait(lk);
    }
    lane->busy = true;
}

LaneLease::~LaneLease()
{
    if (!lane) return;
    // nothing of this call may still be running on the lane when the next caller takes it
    (void)hipSetDevice(cx->device);
    (void)hipStreamSynchronize(lane->st.get());
    (void)hipStreamSynchronize(lane->copy_st.get());
    (void)hipStreamSynchronize(lane->in_st.get());
    { std::lock_guard<std::mutex> lk(cx->lane_mu); lane->busy = false; }
    cx->lane_cv.notify_one();
}

// Layers 1+2 as every caller runs them.  Y holds rows [y_row_base, y_row_base + y_rows) of the (W x H) upscaled plane; the
// kernel clamps its halo reads to that range as well as to the image (tile rows past the end of a band are computed but never
// stored).
void run_conv12(const Call& c, const float* Y, int W, int H, int y_row_base, int y_rows, float* C2, size_t plane, int row0,
                int rows)
{
    // The production strict instance chooses layer 2's body among nested zero tiers (SRCNN_CONV12_TIERS); it is the strict
    // LDS-DMA instance with pruning on, so every other mode, SRCNN_CONV12_DMA=0 and SRCNN_CONV12_PRUNE=0 run without the tiers.
    const bool tiers = c.relax() == 0 && settings().conv12_dma && settings().conv12_prune && settings().conv12_tiers;
    unsigned long long* clk = nullptr;
    if (G.clock_probe.load(std::memory_order_relaxed) && c.cx->clock_buf)
        clk = c.cx->clock_buf + 2 * (size_t)(c.cx->clock_n.fetch_add(1) % kClockSlots);
    // the tile queue lives with the workspace: one per stream, so launches that share it are ordered
    unsigned* queue = nullptr;
    // A capture that is not one of the library's own (those freeze a PRIVATE workspace first): the caller may replay the graph
    // on any stream, beside eager calls that share this workspace's counters, and the probe slot would be baked in as well --
    // such launches deal their tiles with the static stride and stamp nothing.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool foreign_capture = c.s && c.ws && !c.ws->frozen && hipStreamIsCapturing(c.s, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive;
    if (foreign_capture) clk = nullptr;
    if (c.ws && settings().conv12_queue && !foreign_capture) {
        if (c.ws->queue && c.ws->queue_dirty) {
            // a call on this workspace failed after launching: a launch that never finished leaves its draws behind
            if (hipMemsetAsync(c.ws->queue, 0, 2 * sizeof(unsigned), c.s) == hipSuccess) c.ws->queue_dirty = false;
            else (void)hipGetLastError();
        }
        if (!c.ws->queue && !c.ws->frozen) {
            void* q = nullptr;
            // zeroed ON THE LAUNCH STREAM: lane streams are non-blocking, so a null-stream hipMemset is not ordered before
            // the first kernel that draws from the queue (seen as wrong tiles in the first call of a fresh lane)
            if (hipMalloc(&q, 2 * sizeof(unsigned)) == hipSuccess && hipMemsetAsync(q, 0, 2 * sizeof(unsigned), c.s) == hipSuccess) c.ws->queue = static_cast<unsigned*>(q);
            else { (void)hipFree(q); (void)hipGetLastError(); }
        }
        queue = c.ws->queue;
    }
    launch_conv12_mfma(Y, W, H, y_row_base, y_rows, C2, plane, row0, rows, c.relax(), tiers, c.cx->num_cus, c.s, clk, queue);
}

namespace {

// (StageTimer, the RAII bracket of one stage on the launch stream, is srcnn_host.hpp: srcnn_rect_list_call.cpp uses it too)

void drain_spans_locked(Ctx& cx)
{
    for (auto& sp : cx.spans) {
        float ms = 0.f;
        if (hipEventSynchronize(sp.b.get()) == hipSuccess && hipEventElapsedTime(&ms, sp.a.get(), sp.b.get()) == hipSuccess) {
            cx.stage_ms[sp.stage] += ms;
            cx.stage_n[sp.stage] += 1;
        }
        cx.event_pool.push_back(std::move(sp.a));
        cx.event_pool.push_back(std::move(sp.b));
    }
    cx.spans.clear();
}

DevAxisTable view_of(const TableRef& t) { return t->view(); }

// FRAWResizeEngine::scale (src/frawscale.cpp:162-286) for destination rows [r0,r1) only, from either kind of source.
// dst holds rows [r0,r1) (row r0 at offset 0).  tmp is scratch from the call's workspace.
int resample_src_rows(Call& c, const YSource& src, unsigned sw, unsigned sh, unsigned dw, unsigned dh, int filter,
                      unsigned r0, unsigned r1, float* d_dst)
{
    Workspace& ws = *c.ws;
    hipStream_t s = c.s;
    const float* d_in = src.plane;
    if (sw == dw && sh == dh) {
        // The reference's identity branch copies sizeof(unsigned short) bytes per pixel into an
        // uninitialised buffer (src/frawscale.cpp:185-193), i.e. half the plane is garbage.  We copy the
        // whole plane (the evident intent); documented in DESIGN.md as the one deliberate deviation and pinned by
        // tests/test_gpu_parity.py::test_identity_size_deviation_is_pinned.
        if (!d_in) return fail(SRCNN_E_UNSUPPORTED, "identity-size resample needs a float plane");
        HIP_TRY(hipMemcpyAsync(d_dst, d_in + (size_t)r0 * sw, sizeof(float) * (size_t)(r1 - r0) * sw,
                               hipMemcpyDeviceToDevice, s));
        return SRCNN_OK;
    }
    TableRef tv, th;
    int rc;
    if (dw > sw && sh != dh) {
        // up-scale in both axes: vertical first, then horizontal (src/frawscale.cpp:238-278), both in one kernel
        if ((rc = get_table(c, filter, dw, sw, th))) return rc;
        if ((rc = get_table(c, filter, dh, sh, tv))) return rc;
        if (!settings().resample_2pass &&
            launch_rs2d(src, sw, sh, d_dst, dw, dh, r0, r1 - r0, view_of(tv), view_of(th), s)) return SRCNN_OK;
    }
    if (!d_in) return fail(SRCNN_E_UNSUPPORTED, "this resample shape needs a float source plane");
    if (dw <= sw) {
        // horizontal first over all source rows, then vertical (src/frawscale.cpp:195-237)
        const float* mid = d_in;
        int mid_row_base = 0;
        if (sw != dw) {
            if ((rc = get_table(c, filter, dw, sw, th))) return rc;
            if (sh != dh) {
                // only the source rows the vertical taps of rows [r0, r1) read (a banded call used to redo the pass over ALL
                // source rows for every band -- and over rows of a split plane that had not been staged yet)
                if ((rc = get_table(c, filter, dh, sh, tv))) return rc;
                unsigned lo = 0, hi = sh;
                tv->source_span(r0, r1, lo, hi);
                if (hi <= lo) return fail(SRCNN_E_UNSUPPORTED, "empty source span for rows [%u,%u)", r0, r1);
                if ((rc = ws.grow(ws.tmp, (size_t)dw * (hi - lo)))) return rc;
                launch_resample_rows(d_in + (size_t)lo * sw, sw, ws.tmp.data(), dw, hi - lo, view_of(th), s);
                mid = ws.tmp.data();
                mid_row_base = (int)lo;
            } else {
                launch_resample_rows(d_in + (size_t)r0 * sw, sw, d_dst, dw, r1 - r0, view_of(th), s);
                return SRCNN_OK;
            }
        }
        if (!tv && (rc = get_table(c, filter, dh, sh, tv))) return rc;
        launch_resample_cols(mid, dw, mid_row_base, d_dst, r0, r1 - r0, view_of(tv), s);
    } else {
        // vertical first, then horizontal (src/frawscale.cpp:238-278)
        if (!th && (rc = get_table(c, filter, dw, sw, th))) return rc;
        const float* mid = d_in + (size_t)r0 * sw;
        if (sh != dh) {
            if (!tv && (rc = get_table(c, filter, dh, sh, tv))) return rc;
            if ((rc = ws.grow(ws.tmp, (size_t)sw * (r1 - r0)))) return rc;
            launch_resample_cols(d_in, sw, 0, ws.tmp.data(), r0, r1 - r0, view_of(tv), s);
            mid = ws.tmp.data();
        }
        launch_resample_rows(mid, sw, d_dst, dw, r1 - r0, view_of(th), s);
    }
    return SRCNN_OK;
}

}  // namespace

// Columns [c0,c1) x rows [r0,r1) of what resample_src_rows produces for a float plane, bit for bit, at the cost of that window:
// d_dst is tight (c1 - c0 floats per row), the source has in_stride floats per row.  Same pass order, same skipped passes
// and the same identity copy as above; the intermediate image (fp32, like the reference's) covers only the source span the
// contribution tables give for the window.  The generic one-sample-per-thread kernels serve every shape: k_rs2d computes the
// same bits (tests/test_gpu_resample_dispatch.py), so no dispatch is needed for parity.  d_in may itself be a window of the
// sw x sh plane: its first float is sample (in_x0, in_y0), and it holds every sample the taps of the window read.
int resample_window(Call& c, const float* d_in, size_t in_stride, unsigned in_x0, unsigned in_y0, unsigned sw, unsigned sh,
                    unsigned dw, unsigned dh, int filter, unsigned c0, unsigned c1, unsigned r0, unsigned r1, float* d_dst)
{
    Workspace& ws = *c.ws;
    hipStream_t s = c.s;
    const int nc = (int)(c1 - c0), nr = (int)(r1 - r0);
    if (sw == dw && sh == dh) {      // the pinned identity-size deviation: the window is copied
        launch_window_copy(d_in + (size_t)(r0 - in_y0) * in_stride + (c0 - in_x0), in_stride, d_dst, (size_t)nc, nc, nr, s);
        return SRCNN_OK;
    }
    TableRef tv, th;
    int rc;
    if (sw != dw && (rc = get_table(c, filter, dw, sw, th))) return rc;
    if (sh != dh && (rc = get_table(c, filter, dh, sh, tv))) return rc;
    if (!tv) {                       // rows keep their size: the horizontal pass alone
        launch_window_rows(d_in + (size_t)(r0 - in_y0) * in_stride, in_stride, (int)in_x0, d_dst, (int)c0, nc, nr, view_of(th), s);
        return SRCNN_OK;
    }
    if (!th) {                       // columns keep their size: the vertical pass alone
        launch_window_cols(d_in + (c0 - in_x0), in_stride, (int)in_y0, d_dst, nc, (int)r0, nr, view_of(tv), s);
        return SRCNN_OK;
    }
    if (dw <= sw) {
        // horizontal first, over the source rows the vertical taps of rows [r0, r1) read, then vertical
        unsigned lo = 0, hi = sh;
        tv->source_span(r0, r1, lo, hi);
        if (hi <= lo) return fail(SRCNN_E_UNSUPPORTED, "empty source span for rows [%u,%u)", r0, r1);
        if ((rc = ws.grow(ws.tmp, (size_t)nc * (hi - lo)))) return rc;
        launch_window_rows(d_in + (size_t)(lo - in_y0) * in_stride, in_stride, (int)in_x0, ws.tmp.data(), (int)c0, nc, (int)(hi - lo), view_of(th), s);
        launch_window_cols(ws.tmp.data(), (size_t)nc, (int)lo, d_dst, nc, (int)r0, nr, view_of(tv), s);
    } else {
        // vertical first, over the source columns the horizontal taps of columns [c0, c1) read, then horizontal
        unsigned lo = 0, hi = sw;
        th->source_span(c0, c1, lo, hi);
        if (hi <= lo) return fail(SRCNN_E_UNSUPPORTED, "empty source span for columns [%u,%u)", c0, c1);
        if ((rc = ws.grow(ws.tmp, (size_t)(hi - lo) * nr))) return rc;
        launch_window_cols(d_in + (lo - in_x0), in_stride, (int)in_y0, ws.tmp.data(), (int)(hi - lo), (int)r0, nr, view_of(tv), s);
        launch_window_rows(ws.tmp.data(), (size_t)(hi - lo), (int)lo, d_dst, (int)c0, nc, nr, view_of(th), s);
    }
    return SRCNN_OK;
}

int resample_rows_range(Call& c, const float* d_in, unsigned sw, unsigned sh, unsigned dw, unsigned dh, int filter,
                        unsigned r0, unsigned r1, float* d_dst)
{
    return resample_src_rows(c, YSource::from_plane(d_in), sw, sh, dw, dh, filter, r0, r1, d_dst);
}

int check_plane(const void* in, unsigned w, unsigned h, const void* out)
{
    if (!in || !out || w == 0 || h == 0) return fail(SRCNN_E_ARG, "NULL pointer or zero dimension");
    if ((unsigned long long)w * h > 0x7fffffffULL) return fail(SRCNN_E_UNSUPPORTED, "plane too large");
    return SRCNN_OK;
}

namespace {

static_assert(kLayer2Planes == (unsigned)C2N, "srcnn_y_path_geom.hpp sizes the layer-2 scratch");

// The one pass of the Y path: resample + conv12 + conv3 for output rows [r0,r1) of a window of the upscaled plane that is W
// floats wide and dh rows high (the whole plane, or a rect's columns with their halo), into d_out (W floats per row, row r0
// first).  resample(ua, ub) fills ws.up with rows [ua,ub) of that window; store() launches what the route still owes its caller,
// outside the stage timers and before the error check; `who` names the route in the error text, label... is the printf-style
// trace label of the strict sequence (the fused tier opens none).  Every buffer is grown before the first launch: growing drains
// the device.
// (list_batched of srcnn_rect_list_call.hpp runs the same three stages with launch_list_replicate between them: it stays apart)
template <class Resample, class Store, class... Label>
int y_path_pass(Call& c, const char* who, unsigned W, unsigned dh, unsigned r0, unsigned r1, float* d_out, Resample resample, Store store,
                Label... label)
{
    Workspace& ws = *c.ws;
    const HaloSpan v = y_path_halo(dh, r0, r1);
    int rc;
    if ((rc = ws.grow(ws.up, (size_t)W * (v.ub - v.ua)))) return rc;
#ifndef SRCNN_STRICT_ONLY
    if (c.mode == SRCNN_MODE_FAST_F16) {
        // non-parity tier: one kernel for all three layers, no layer-2 planes at all
        {
            StageTimer t(SRCNN_STAGE_RESAMPLE, c);
            if ((rc = resample(v.ua, v.ub))) return rc;
        }
        {
            StageTimer t(SRCNN_STAGE_CONV12, c);
            launch_fused_f16(ws.up.data(), (int)W, (int)dh, (int)v.ua, (int)(v.ub - v.ua), d_out, (int)r0, (int)(r1 - r0), c.cx->fused_w.data(),
                             c.cx->num_cus, c.s);
        }
        store();
        HIP_TRY(hipGetLastError());
        return SRCNN_OK;
    }
#endif
    const size_t plane = (size_t)W * (v.cb - v.ca);
    if ((rc = ws.grow(ws.c2, (size_t)C2N * plane))) return rc;
    TraceRange tr(label...);
    {
        StageTimer t(SRCNN_STAGE_RESAMPLE, c);
        if ((rc = resample(v.ua, v.ub))) return rc;
    }
    {
        StageTimer t(SRCNN_STAGE_CONV12, c);
        run_conv12(c, ws.up.data(), (int)W, (int)dh, (int)v.ua, (int)(v.ub - v.ua), ws.c2.data(), plane, (int)v.ca, (int)(v.cb - v.ca));
    }
    {
        StageTimer t(SRCNN_STAGE_CONV3, c);
        launch_conv3(ws.c2.data(), plane, (int)W, (int)dh, (int)v.ca, (int)(v.cb - v.ca), d_out, (int)r0, (int)(r1 - r0), c.relax(), c.s);
    }
    store();
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
        ws.queue_dirty = true;                         // re-zeroed on the launch stream before the next launch trusts it
        return fail(SRCNN_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    return SRCNN_OK;
}

}  // namespace

// The pass over whole rows: output rows [r0,r1) of the (dw x dh) result.
int y_path_rows(Call& c, const YSource& src, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                unsigned r0, unsigned r1, float* d_out)
{
    if (r1 > dh || r0 >= r1) return fail(SRCNN_E_ARG, "row range [%u,%u) outside 0..%u", r0, r1, dh);
    if (!y_path_fits(0, h, dw, dh, r1 - r0)) return fail(SRCNN_E_UNSUPPORTED, "output %ux%u too large", dw, dh);
    return y_path_pass(
        c, "y_path_rows", dw, dh, r0, r1, d_out,
        [&](unsigned ua, unsigned ub) { return resample_src_rows(c, src, w, h, dw, dh, filter, ua, ub, c.ws->up.data()); }, [] {},
        "srcnn y_path rows [%u,%u) of %ux%u", r0, r1, dw, dh);
}

// Source rows [lo,hi) of the (w x h) input that output rows [r0,r1) of the Y path depend on: +-2 rows of layer-2
// activations, +-4 rows of upscaled Y for those, and the vertical taps of the resampler for that range -- read off the
// contribution table itself, so it is exact for every filter and ratio.
int y_path_source_rows(Call& c, unsigned h, unsigned dh, int filter, unsigned r0, unsigned r1, unsigned& lo, unsigned& hi)
{
    const HaloSpan v = y_path_halo(dh, r0, r1);
    if (h == dh) { lo = v.ua; hi = v.ub; return SRCNN_OK; }
    TableRef tv;
    int rc = get_table(c, filter, dh, h, tv);
    if (rc) return rc;
    tv->source_span(v.ua, v.ub, lo, hi);
    return SRCNN_OK;
}

// (1 << 20 rows: the most a band ever has, and what the function returns when even they fit)
unsigned budget_band_rows(unsigned dw) { return y_path_band_rows(G.ws_budget.load(), false, dw, 1u << 20); }

unsigned y_path_pass_rows(const Call& c, unsigned W, unsigned rows)
{
    return y_path_band_rows(G.ws_budget.load(), c.mode == SRCNN_MODE_FAST_F16, W, rows);
}

// Cut output rows [R0,R1) of a (dw x dh) frame into pieces of about frac[0], frac[1], ... of the range (the last piece takes the
// rest).  The layer-1+2 kernel is persistent: `grid` resident workgroups walk a piece's 64 x tile_rows tiles with a static
// stride, so a piece whose tile count is not a multiple of the grid wastes part of its last round (a plain percentage split
// of an 8K frame into 5 bands cost 68 rounds instead of 64, +6 % of the dominant kernel; four equal quarters of one rank's
// band of a 16K frame 36 instead of 32).  Each cut is therefore moved, within +-30 % of its target height, to where the
// layer-2 rows the piece computes (its rows + 2 halo rows per interior side) fill their rounds best.  Pure function of its
// arguments: every rank of a tiled frame derives the same table.
std::vector<unsigned> plan_cuts(unsigned R0, unsigned R1, unsigned dw, unsigned dh, const double* frac, int nfrac, int grid, int tile_rows)
{
    const unsigned rows = R1 - R0;
    std::vector<unsigned> cuts{R0};
    const unsigned tiles_x = (dw + 63) / 64;
    unsigned a = R0;
    for (int i = 0; i < nfrac; ++i) {
        const unsigned want = std::max(32u, (unsigned)(rows * frac[i]));
        unsigned b = a + (want & ~15u);
        if (grid > 0 && tile_rows > 0) {
            // layer-2 rows of piece [a, b) = [max(a-2,0), min(b+2,dh)): choose their tile-row count near the target
            const unsigned top = a >= 2 ? 2 : a;
            const unsigned t_want = (want + top + 2 + tile_rows - 1) / tile_rows;
            const unsigned t_lo = std::max(1u, (unsigned)(t_want * 0.7)), t_hi = std::max(t_lo, (unsigned)(t_want * 1.3));
            double best = -1.0;
            unsigned best_t = t_want;
            for (unsigned t = t_lo; t <= t_hi; ++t) {
                const unsigned long long tiles = (unsigned long long)t * tiles_x;
                const unsigned long long rounds = (tiles + grid - 1) / grid;
                const double fill = (double)tiles / (double)(rounds * grid);
                const double score = fill - 1e-4 * (t > t_want ? t - t_want : t_want - t);      // ties: closest to the target
                if (score > best) { best = score; best_t = t; }
            }
            if (best_t * tile_rows > top + 2) b = a + best_t * tile_rows - top - 2;
        }
        if (b <= a || b >= R1 || R1 - b < 32) break;
        cuts.push_back(b);
        a = b;
    }
    cuts.push_back(R1);
    return cuts;
}

// Output rows [r0,r1).  The 32 layer-2 planes are the big scratch (128 B per output pixel).  A range whose planes
// would exceed the workspace budget (default 4.5 GiB, SRCNN_MAX_WORKSPACE_MB) is produced in horizontal bands --
// bit-identical to the whole range -- so a 16K x 16K output needs the same scratch as an 8K one.
int y_path_range(Call& c, const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                 unsigned r0, unsigned r1, float* d_out)
{
    if (r1 > dh || r0 >= r1) return fail(SRCNN_E_ARG, "row range [%u,%u) outside 0..%u", r0, r1, dh);
    const YSource src = YSource::from_plane(d_in);
    const unsigned band = y_path_pass_rows(c, dw, r1 - r0);      // (all of them: one pass)
    for (unsigned a = r0; a < r1; a += band) {
        const unsigned b = std::min(r1, a + band);
        int rc = y_path_rows(c, src, w, h, dw, dh, filter, a, b, d_out + (size_t)(a - r0) * dw);
        if (rc) return rc;
    }
    return SRCNN_OK;
}

int y_path_frame(Call& c, const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, float* d_out)
{
    return y_path_range(c, d_in, w, h, dw, dh, filter, 0, dh, d_out);
}

namespace {

// Output samples [x0,x1) x [r0,r1) in one pass.  A pixel's arithmetic does not depend on where its tile lies, so a window of
// the upscaled plane goes through the unchanged layer kernels as if it were a Ww-wide frame of dh rows: the columns of
// y_path_halo(dw, x0, x1), the rect + 2 (layer 3) + 4 (layer 1), cut short at the true borders.  The kernels' clamp-to-edge is
// then wrong only inside that halo, which the store leaves behind; where the window ends at a true border the clamp is the
// frame's own.  Rows are the pass's, as for y_path_rows (H and the row bases are the true ones).  (in_x0, in_y0): the sample of
// the w x h plane at which d_in begins.
int y_path_rect_rows(Call& c, const float* d_in, size_t in_stride, unsigned in_x0, unsigned in_y0, unsigned w, unsigned h,
                     unsigned dw, unsigned dh, int filter, unsigned x0, unsigned x1, unsigned r0, unsigned r1, float* d_out,
                     size_t out_stride)
{
    Workspace& ws = *c.ws;
    const HaloSpan hx = y_path_halo(dw, x0, x1);
    const unsigned Ww = hx.width();
    if (int rc = ws.grow(ws.win, (size_t)Ww * (r1 - r0))) return rc;
    return y_path_pass(
        c, "y_path_rect", Ww, dh, r0, r1, ws.win.data(),
        [&](unsigned ua, unsigned ub) { return resample_window(c, d_in, in_stride, in_x0, in_y0, w, h, dw, dh, filter, hx.ua, hx.ub, ua, ub, ws.up.data()); },
        [&] { launch_window_copy(ws.win.data() + (x0 - hx.ua), Ww, d_out, out_stride, (int)(x1 - x0), (int)(r1 - r0), c.s); },
        "srcnn y_path rect [%u,%u)x[%u,%u) of %ux%u", x0, x1, r0, r1, dw, dh);
}

}  // namespace

// The rect [x0,x1) x [y0,y1).  A rect that is a row range of tight planes is one (y_path_range); every other is produced from
// windows, in row bands when the 32 layer-2 planes of the window would exceed the workspace budget -- with identical bits.
// d_in begins at sample (in_x0, in_y0) of the w x h plane and holds at least what the rect depends on; whole_plane: it holds all
// h rows (the row-range path reads through the frame resamplers, which are not bounded by the rect's source rectangle).
int y_path_rect(Call& c, const float* d_in, size_t in_stride, unsigned in_x0, unsigned in_y0, unsigned w, unsigned h, unsigned dw,
                unsigned dh, int filter, unsigned x0, unsigned y0, unsigned x1, unsigned y1, float* d_out, size_t out_stride, bool whole_plane)
{
    if (x1 > dw || x0 >= x1 || y1 > dh || y0 >= y1) return fail(SRCNN_E_ARG, "rect [%u,%u)x[%u,%u) outside %ux%u", x0, x1, y0, y1, dw, dh);
    if (!y_path_fits(0, h, dw, dh, y1 - y0)) return fail(SRCNN_E_UNSUPPORTED, "output %ux%u too large", dw, dh);
    if (x0 == 0 && x1 == dw && whole_plane && in_x0 == 0 && in_y0 == 0 && in_stride == w && out_stride == dw)
        return y_path_range(c, d_in, w, h, dw, dh, filter, y0, y1, d_out);
    const unsigned band = y_path_pass_rows(c, y_path_halo(dw, x0, x1).width(), y1 - y0);
    for (unsigned a = y0; a < y1; a += band) {
        const unsigned b = std::min(y1, a + band);
        int rc = y_path_rect_rows(c, d_in, in_stride, in_x0, in_y0, w, h, dw, dh, filter, x0, x1, a, b, d_out + (size_t)(a - y0) * out_stride, out_stride);
        if (rc) return rc;
    }
    return SRCNN_OK;
}

int check_y_path_args(const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const float* d_out)
{
    int rc = check_plane(d_in, w, h, d_out);
    if (rc) return rc;
    if (dw == 0 || dh == 0) return fail(SRCNN_E_SCALE, "scaled size %ux%u", dw, dh);
    if (filter < 0 || filter > 4) return fail(SRCNN_E_ARG, "bad filter %d", filter);
    return SRCNN_OK;
}

namespace {

int batch_frames(Call& c, const float* d_in, unsigned w, unsigned h, unsigned nframes, float* d_out)
{
    const size_t in_n = (size_t)w * h, out_n = in_n * 4;
    for (unsigned f = 0; f < nframes; ++f) {
        int rc = y_path_frame(c, d_in + f * in_n, w, h, 2 * w, 2 * h, SRCNN_FILTER_BICUBIC, d_out + f * out_n);
        if (rc) return rc;
    }
    return SRCNN_OK;
}

// A captured batch owns everything its kernel nodes point at: its scratch and its contribution tables live exactly
// as long as the handle, whatever happens to the stream's own workspace or to the table cache in the meantime.
struct BatchGraph {
    Ctx* cx = nullptr;
    int device = 0;         // of cx: srcnn_batch_graph_destroy binds it, and the handle may outlive srcnn_shutdown (and with it *cx)
    hipStream_t stream = nullptr;
    Workspace ws;
    std::vector<TableRef> tables;
    GraphExec exec;         // (last: destroyed before the scratch and the tables its nodes point at)
};

// What must happen before a context's members free themselves (srcnn_shutdown destroys the Ctx right after, on this thread,
// with this device still bound): the device is idle, no call is left inside one of the context's sections, and the last
// stage timings are read.  Graphs still alive keep their own references to their tables.
void release_context(Ctx& cx)
{
    (void)hipSetDevice(cx.device);
    (void)hipDeviceSynchronize();
    std::scoped_lock all(cx.lane_mu, cx.mu, cx.bounce.mu, cx.host_call.mu);
    drain_spans_locked(cx);
}

}  // namespace

}  // namespace srcnn

using namespace srcnn;

// ================================================================================================
extern "C" {

int srcnn_abi_version(void) { return SRCNN_AMD_ABI_VERSION; }

const char* srcnn_last_error(void) { return srcnn::last_error(); }

int srcnn_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int srcnn_init(int device)
{
    std::lock_guard<std::mutex> lk(G.mu);
    if (!G.ctxs.empty()) {
        if (device >= 0 && device != G.ctxs[0]->device)
            return fail(SRCNN_E_ARG, "srcnn_init: already bound to device %d (asked for %d)", G.ctxs[0]->device, device);
        return SRCNN_OK;
    }
    if (device < 0) return lazy_init_locked();
    return make_context_locked(device);
}

int srcnn_init_devices(const int* devices, int n)
{
    std::lock_guard<std::mutex> lk(G.mu);
    std::vector<int> want;
    if (!devices || n <= 0) {
        int have = 0;
        if (hipGetDeviceCount(&have) != hipSuccess || have <= 0) return fail(SRCNN_E_NODEVICE, "no HIP device visible; this library has no CPU path");
        for (int d = 0; d < have; ++d) want.push_back(d);
    } else {
        if (n > 64) return fail(SRCNN_E_ARG, "srcnn_init_devices: at most 64 contexts");
        want.assign(devices, devices + n);
    }
    if (!G.ctxs.empty()) {
        // idempotent for the same list; a prefix may be extended (srcnn_init(0) followed by srcnn_init_devices({0,1,..}))
        for (size_t k = 0; k < G.ctxs.size(); ++k)
            if (k >= want.size() || want[k] != G.ctxs[k]->device)
                return fail(SRCNN_E_ARG, "srcnn_init_devices: context %zu is already bound to device %d; call srcnn_shutdown first",
                            k, G.ctxs[k]->device);
    }
    for (size_t k = G.ctxs.size(); k < want.size(); ++k) {
        int rc = make_context_locked(want[k]);
        if (rc) return rc;
    }
    return SRCNN_OK;
}

int srcnn_context_count(void) { return context_count(); }

int srcnn_context_device(int k)
{
    Ctx* cx = context_at(k);
    return cx ? cx->device : fail(SRCNN_E_ARG, "no context %d", k);
}

int srcnn_set_context(int k)
{
    if (int rc = ensure_init()) return rc;
    if (k < 0 || k >= context_count()) return fail(SRCNN_E_ARG, "no context %d (have %d)", k, context_count());
    const int prev = t_ctx;
    t_ctx = k;
    Ctx* cx = context_at(k);
    if (cx) (void)bind(*cx);
    return prev;
}

int srcnn_get_context(void) { return t_ctx; }

void srcnn_shutdown(void)
{
    srcnn_comm_destroy();
    async_chain_reset();
    std::vector<std::unique_ptr<Ctx>> dying;
    {
        std::lock_guard<std::mutex> lk(G.mu);
        if (G.ctxs.empty()) return;
        G.nctx.store(0);
        dying.swap(G.ctxs);
        G.stream_ctx.clear();
    }
    for (auto& cx : dying) { release_context(*cx); cx.reset(); }
    t_ctx = 0;
}

// Release what idle lanes and unreferenced cache entries hold (scratch, page-locked staging, contribution tables) without
// shutting the library down: a long-lived process that once handled a very large image gets its memory back.
int srcnn_trim(void)
{
    if (int rc = ensure_init()) return rc;
    for (int k = 0; k < context_count(); ++k) {
        Ctx* cx = context_at(k);
        if (!cx) continue;
        if (int rc = bind(*cx)) return rc;
        {
            std::lock_guard<std::mutex> lk(cx->lane_mu);
            for (auto& l : cx->lanes)
                if (!l->busy) { (void)hipStreamSynchronize(l->st.get()); (void)hipStreamSynchronize(l->copy_st.get()); l->trim(); }
        }
        {
            std::lock_guard<std::mutex> bl(cx->bounce.mu);
            (void)hipDeviceSynchronize();
            cx->bounce.s = {};
        }
        {
            std::lock_guard<std::mutex> hl(cx->host_call.mu);      // (a convenience call in flight holds it: trim waits for it)
            (void)hipDeviceSynchronize();
            cx->host_call.d = {};
        }
        std::lock_guard<std::mutex> lk(cx->mu);
        bool any = false;
        for (auto it = cx->tables.begin(); it != cx->tables.end();) {
            if (it->second.use_count() == 1) {
                if (!any) { (void)hipDeviceSynchronize(); any = true; }
                it = cx->tables.erase(it);
            } else ++it;
        }
    }
    return SRCNN_OK;
}

int srcnn_set_mode(int mode)
{
    if (mode != SRCNN_MODE_STRICT && mode != SRCNN_MODE_FAST && mode != SRCNN_MODE_FAST_F16 && mode != SRCNN_MODE_RELAXED)
        return fail(SRCNN_E_ARG, "bad mode %d", mode);
#ifdef SRCNN_STRICT_ONLY
    if (mode != SRCNN_MODE_STRICT) return fail(SRCNN_E_UNSUPPORTED, "this is a strict-only build (make STRICT_ONLY=1): mode %d is not compiled in", mode);
#endif
    if (mode == SRCNN_MODE_RELAXED) mode |= (int)(G.relax_mask.load() & 0xfu) << 8;
    return G.mode.exchange(mode) & 0xff;
}

int srcnn_get_mode(void) { return G.mode.load() & 0xff; }

int srcnn_set_relaxation(unsigned mask)
{
    if (mask & ~0xfu) return fail(SRCNN_E_ARG, "bad relaxation mask 0x%x", mask);
    if ((mask & SRCNN_RELAX_L3_X64) && (mask & SRCNN_RELAX_L3_F32)) return fail(SRCNN_E_ARG, "layer 3 can be relaxed one way at a time");
    const unsigned prev = G.relax_mask.exchange(mask);
    int m = G.mode.load();
    while ((m & 0xff) == SRCNN_MODE_RELAXED && !G.mode.compare_exchange_weak(m, SRCNN_MODE_RELAXED | (int)(mask << 8))) {}
    return (int)prev;
}

size_t srcnn_set_workspace_limit(size_t bytes)
{
    return G.ws_budget.exchange(std::max<size_t>(bytes, 1u << 20));
}

int srcnn_device_name(char* buf, size_t cap)
{
    Ctx* cx = cur_ctx();
    if (!cx) return SRCNN_E_NODEVICE;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cx->device));
    snprintf(buf, cap, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return SRCNN_OK;
}

// ---- plumbing (all on the calling thread's current context) ------------------------------------
void* srcnn_dev_alloc(size_t bytes)
{
    if (!cur_ctx()) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { fail(SRCNN_E_DEVMEM, "hipMalloc(%zu) failed", bytes); return nullptr; }
    return p;
}
void srcnn_dev_free(void* p) { if (p) (void)hipFree(p); }
void* srcnn_host_alloc_pinned(size_t bytes)
{
    Ctx* cx = cur_ctx();
    if (!cx) return nullptr;
    void* p = pinned_alloc(*cx, bytes);
    if (p) { std::lock_guard<std::mutex> lk(g_pinned_mu); pinned_blocks()[reinterpret_cast<uintptr_t>(p)] = bytes ? bytes : 1; }
    return p;
}
void srcnn_host_free_pinned(void* p)
{
    if (!p) return;
    { std::lock_guard<std::mutex> lk(g_pinned_mu); pinned_blocks().erase(reinterpret_cast<uintptr_t>(p)); }
    (void)hipHostFree(p);
}

int srcnn_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream)
{
    Ctx* cx = ctx_for_stream(stream);
    if (!cx) return SRCNN_E_NODEVICE;
    if (int rc = bind(*cx)) return rc;
    return copy_h2d_any(*cx, dst, src, bytes, (hipStream_t)stream);
}
int srcnn_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream)
{
    Ctx* cx = ctx_for_stream(stream);
    if (!cx) return SRCNN_E_NODEVICE;
    if (int rc = bind(*cx)) return rc;
    return copy_d2h_any(*cx, dst, src, bytes, (hipStream_t)stream);
}
int srcnn_memset_dev(void* dst, int byte, size_t bytes, void* stream)
{
    if (!ctx_for_stream(stream)) return SRCNN_E_NODEVICE;
    HIP_TRY(hipMemsetAsync(dst, byte, bytes, (hipStream_t)stream));
    return SRCNN_OK;
}
int srcnn_stream_create(void** stream)
{
    Ctx* cx = cur_ctx();
    if (!cx) return SRCNN_E_NODEVICE;
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    { std::lock_guard<std::mutex> lk(G.mu); G.stream_ctx[s] = cx->index; }
    *stream = s;
    return SRCNN_OK;
}
int srcnn_stream_destroy(void* stream)
{
    if (!stream) return SRCNN_OK;
    Ctx* cx = ctx_for_stream(stream);
    if (!cx) return SRCNN_E_NODEVICE;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    std::unique_ptr<Workspace> ws;
    {
        std::lock_guard<std::mutex> lk(cx->mu);
        auto it = cx->ws.find((hipStream_t)stream);
        if (it != cx->ws.end()) { ws = std::move(it->second); cx->ws.erase(it); }
    }
    if (ws) { std::lock_guard<std::mutex> wl(ws->mu); }      // (a call that still enqueues on it finishes first)
    ws.reset();
    { std::lock_guard<std::mutex> lk(G.mu); G.stream_ctx.erase((hipStream_t)stream); }
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return SRCNN_OK;
}
int srcnn_stream_sync(void* stream)
{
    if (!ctx_for_stream(stream)) return SRCNN_E_NODEVICE;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return SRCNN_OK;
}
int srcnn_device_sync(void) { if (!cur_ctx()) return SRCNN_E_NODEVICE; HIP_TRY(hipDeviceSynchronize()); return SRCNN_OK; }
int srcnn_event_create(void** ev)
{
    if (!cur_ctx()) return SRCNN_E_NODEVICE;
    hipEvent_t e; HIP_TRY(hipEventCreate(&e)); *ev = e; return SRCNN_OK;
}
int srcnn_event_destroy(void* ev) { if (ev) HIP_TRY(hipEventDestroy((hipEvent_t)ev)); return SRCNN_OK; }
int srcnn_event_record(void* ev, void* stream)
{
    if (!ctx_for_stream(stream)) return SRCNN_E_NODEVICE;
    HIP_TRY(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return SRCNN_OK;
}
int srcnn_stream_wait_event(void* stream, void* ev)
{
    if (!ctx_for_stream(stream)) return SRCNN_E_NODEVICE;
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
    return SRCNN_OK;
}
int srcnn_event_elapsed_ms(void* start, void* stop, float* ms)
{
    HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return SRCNN_OK;
}

// ---- the hot path ------------------------------------------------------------------------------
int srcnn_y_path_f32_dev(const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                         float* d_out, void* stream)
{
    int rc;
    if ((rc = check_y_path_args(d_in, w, h, dw, dh, filter, d_out))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    return y_path_frame(sc.c, d_in, w, h, dw, dh, filter, d_out);
}

int srcnn_y_upscale2x_f32_dev(const float* d_in, unsigned w, unsigned h, float* d_out, void* stream)
{
    return srcnn_y_path_f32_dev(d_in, w, h, 2 * w, 2 * h, SRCNN_FILTER_BICUBIC, d_out, stream);
}

int srcnn_y_upscale2x_f32_batch_dev(const float* d_in, unsigned w, unsigned h, unsigned nframes, float* d_out,
                                    void* stream)
{
    if (nframes == 0) return fail(SRCNN_E_ARG, "nframes == 0");
    int rc;
    if ((rc = check_y_path_args(d_in, w, h, 2 * w, 2 * h, SRCNN_FILTER_BICUBIC, d_out))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    return batch_frames(sc.c, d_in, w, h, nframes, d_out);
}

int srcnn_batch_graph_create(const float* d_in, unsigned w, unsigned h, unsigned nframes, float* d_out, void* stream,
                             void** graph)
{
    if (!graph) return fail(SRCNN_E_ARG, "graph == NULL");
    if (!stream) return fail(SRCNN_E_ARG, "graph capture needs a non-default stream");
    if (nframes == 0) return fail(SRCNN_E_ARG, "nframes == 0");
    int rc;
    if ((rc = check_y_path_args(d_in, w, h, 2 * w, 2 * h, SRCNN_FILTER_BICUBIC, d_out))) return rc;
    Ctx* cx = ctx_for_stream(stream);
    if (!cx) return SRCNN_E_NODEVICE;
    auto bg = std::make_unique<BatchGraph>();
    bg->cx = cx;
    bg->device = cx->device;
    bg->stream = (hipStream_t)stream;
    Call c;
    c.cx = cx; c.s = bg->stream; c.ws = &bg->ws; c.mode = G.mode.load(); c.hold = &bg->tables;
    auto drop = [&](int code) { (void)hipStreamSynchronize(bg->stream); return code; };      // (bg frees what it holds after it)
    // eager run first: builds tables and grows the private workspace, so nothing allocates inside the capture
    if ((rc = batch_frames(c, d_in, w, h, nframes, d_out))) return drop(rc);
    if (hipStreamSynchronize(bg->stream) != hipSuccess) return drop(fail(SRCNN_E_HIP, "stream sync before capture failed"));
    bg->ws.frozen = true;
    c.timing = false;                                      // event pairs cannot be timed inside a capture
    Graph gr;
    hipError_t e = hipStreamBeginCapture(bg->stream, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) rc = batch_frames(c, d_in, w, h, nframes, d_out);
    hipError_t e2 = hipStreamEndCapture(bg->stream, gr.put());
    if (e != hipSuccess || e2 != hipSuccess)
        return drop(fail(SRCNN_E_HIP, "stream capture failed: %s", hipGetErrorString(e != hipSuccess ? e : e2)));
    if (rc) return drop(rc);
    e = hipGraphInstantiate(bg->exec.put(), gr.get(), nullptr, nullptr, 0);
    gr.reset();
    if (e != hipSuccess) return drop(fail(SRCNN_E_HIP, "hipGraphInstantiate -> %s", hipGetErrorString(e)));
    *graph = bg.release();
    return SRCNN_OK;
}

int srcnn_batch_graph_launch(void* graph)
{
    if (!graph) return fail(SRCNN_E_ARG, "graph == NULL");
    BatchGraph* b = static_cast<BatchGraph*>(graph);
    if (int rc = bind(*b->cx)) return rc;
    HIP_TRY(hipGraphLaunch(b->exec.get(), b->stream));
    return SRCNN_OK;
}

int srcnn_batch_graph_destroy(void* graph)
{
    if (!graph) return SRCNN_OK;
    BatchGraph* b = static_cast<BatchGraph*>(graph);
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->stream);
    delete b;
    return SRCNN_OK;
}

int srcnn_y_upscale2x_f32_band_dev(const float* d_in, unsigned w, unsigned h, unsigned row0, unsigned rows,
                                   float* d_out_band, void* stream)
{
    int rc;
    if ((rc = check_plane(d_in, w, h, d_out_band))) return rc;
    if (rows == 0) return fail(SRCNN_E_ARG, "rows == 0");
    if ((unsigned long long)row0 + rows > 2ull * h) return fail(SRCNN_E_ARG, "band [%u,+%u) outside the %u output rows", row0, rows, 2 * h);
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    return y_path_range(sc.c, d_in, w, h, 2 * w, 2 * h, SRCNN_FILTER_BICUBIC, row0, row0 + rows, d_out_band);
}

// ---- one rectangle of the output (include/srcnn_amd_rect.h) --------------------------------------
extern "C++" {
namespace srcnn {

// what both rect entry points refuse about the geometry, in the order the header gives
int check_rect_geometry(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned x0, unsigned y0, unsigned rw, unsigned rh)
{
    if (w == 0 || h == 0 || rw == 0 || rh == 0) return fail(SRCNN_E_ARG, "zero dimension (%ux%u, rect %ux%u)", w, h, rw, rh);
    if (dw == 0 || dh == 0) return fail(SRCNN_E_SCALE, "scaled size %ux%u", dw, dh);
    if (filter < 0 || filter > 4) return fail(SRCNN_E_ARG, "bad filter %d", filter);
    if ((unsigned long long)x0 + rw > dw || (unsigned long long)y0 + rh > dh)
        return fail(SRCNN_E_ARG, "rect %ux%u at (%u,%u) is not inside the %ux%u output", rw, rh, x0, y0, dw, dh);
    return SRCNN_OK;
}

int check_rect_limits(unsigned w, unsigned h, unsigned dw, unsigned dh, unsigned rh)
{
    if (!y_path_fits((unsigned long long)w * h, h, dw, dh, rh)) return fail(SRCNN_E_UNSUPPORTED, "%ux%u -> %ux%u is beyond the Y path's limits", w, h, dw, dh);
    return SRCNN_OK;
}

}  // namespace srcnn
}  // extern "C++"

int srcnn_rect_abi_version(void) { return SRCNN_AMD_RECT_VERSION; }

int srcnn_y_path_rect_source(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned x0, unsigned y0, unsigned rw,
                             unsigned rh, unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh)
{
    int rc;
    if ((rc = check_rect_geometry(w, h, dw, dh, filter, x0, y0, rw, rh))) return rc;
    if ((rc = check_rect_limits(w, h, dw, dh, rh))) return rc;
    unsigned lx, hx, ly, hy;
    y_path_rect_source_span(w, h, dw, dh, filter, x0, y0, x0 + rw, y0 + rh, lx, hx, ly, hy);
    if (sx0) *sx0 = lx;
    if (sy0) *sy0 = ly;
    if (sw) *sw = hx - lx;
    if (sh) *sh = hy - ly;
    return SRCNN_OK;
}

int srcnn_y_path_rect_f32_dev(const float* d_in, size_t in_pitch, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                              unsigned x0, unsigned y0, unsigned rw, unsigned rh, float* d_out, size_t out_pitch, void* stream)
{
    int rc;
    if (!d_in || !d_out) return fail(SRCNN_E_ARG, "NULL pointer");
    if ((rc = check_rect_geometry(w, h, dw, dh, filter, x0, y0, rw, rh))) return rc;
    YuvPlane in, out;
    if ((rc = describe_plane(in, d_in, in_pitch, sizeof(float) * (size_t)w, h, 4, "input", 0))) return rc;
    if ((rc = describe_plane(out, d_out, out_pitch, sizeof(float) * (size_t)rw, rh, 4, "output", 0))) return rc;
    if ((rc = check_rect_limits(w, h, dw, dh, rh))) return rc;
    if ((rc = check_in_out_overlap(&in, 1, &out, 1))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    return y_path_rect(sc.c, d_in, in.pitch / sizeof(float), 0, 0, w, h, dw, dh, filter, x0, y0, x0 + rw, y0 + rh, d_out, out.pitch / sizeof(float));
}

// ---- per-kernel timing -------------------------------------------------------------------------
int srcnn_profile_enable(int on) { return G.profiling.exchange(on != 0) ? 1 : 0; }

int srcnn_profile_reset(void)
{
    for (int k = 0; k < context_count(); ++k) {
        Ctx* cx = context_at(k);
        if (!cx) continue;
        (void)hipSetDevice(cx->device);
        std::lock_guard<std::mutex> lk(cx->mu);
        drain_spans_locked(*cx);
        for (int i = 0; i < SRCNN_STAGE_COUNT; ++i) { cx->stage_ms[i] = 0; cx->stage_n[i] = 0; }
    }
    if (Ctx* cx = context_at(srcnn_get_context())) (void)hipSetDevice(cx->device);
    return SRCNN_OK;
}

int srcnn_profile_read(int stage, double* total_ms, unsigned long long* launches)
{
    if (stage < 0 || stage >= SRCNN_STAGE_COUNT) return fail(SRCNN_E_ARG, "bad stage %d", stage);
    double ms = 0; unsigned long long n = 0;
    for (int k = 0; k < context_count(); ++k) {            // summed over the contexts of the process
        Ctx* cx = context_at(k);
        if (!cx) continue;
        (void)hipSetDevice(cx->device);
        std::lock_guard<std::mutex> lk(cx->mu);
        drain_spans_locked(*cx);
        ms += cx->stage_ms[stage]; n += cx->stage_n[stage];
    }
    if (Ctx* cx = context_at(srcnn_get_context())) (void)hipSetDevice(cx->device);
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    return SRCNN_OK;
}

// ---- clock probe: at which shader clock did each layer-1+2 launch run? ----
// When on, every k_conv12_mfma launch stamps s_memtime (shader cycles) and s_memrealtime (constant 100 MHz) at the start and
// the end of its workgroup 0, which is resident for the whole launch: cycles / ticks x 100 = MHz, ticks / 100 = microseconds.
// This is how "the same kernels run slower inside a ProcessSRCNN call" is told apart into clock and everything else
// (tools/process_clock_probe.py, profiles/r04_process_clock.txt).
int srcnn_debug_clock_probe(int on)
{
    if (int rc = ensure_init()) return rc;
    for (int k = 0; k < context_count(); ++k) {
        Ctx* cx = context_at(k);
        if (!cx) continue;
        (void)hipSetDevice(cx->device);
        if (on && !cx->clock_buf) {
            void* p = nullptr;
            if (hipMalloc(&p, sizeof(unsigned long long) * 2 * kClockSlots) != hipSuccess) return fail(SRCNN_E_DEVMEM, "clock probe buffer");
            cx->clock_buf = static_cast<unsigned long long*>(p);
        }
        if (cx->clock_buf) { (void)hipMemset(cx->clock_buf, 0, sizeof(unsigned long long) * 2 * kClockSlots); (void)hipDeviceSynchronize(); }
        cx->clock_n = 0;
    }
    if (Ctx* cur = context_at(srcnn_get_context())) (void)hipSetDevice(cur->device);
    return G.clock_probe.exchange(on != 0) ? 1 : 0;
}

// launches recorded on `context` since the probe was switched on (in launch order); writes at most `cap` (cycles, ticks) pairs
int srcnn_debug_clock_read(int context, unsigned long long* cycles, unsigned long long* ticks, int cap)
{
    Ctx* cx = context_at(context);
    if (!cx || !cx->clock_buf) return fail(SRCNN_E_ARG, "no clock probe on context %d", context);
    (void)hipSetDevice(cx->device);
    HIP_TRY(hipDeviceSynchronize());
    const unsigned n = std::min(cx->clock_n.load(), kClockSlots);
    std::vector<unsigned long long> host(2 * (size_t)n);
    if (n) HIP_TRY(hipMemcpy(host.data(), cx->clock_buf, sizeof(unsigned long long) * 2 * n, hipMemcpyDeviceToHost));
    for (unsigned i = 0; i < n && (int)i < cap; ++i) {
        if (cycles) cycles[i] = host[2 * i];
        if (ticks) ticks[i] = host[2 * i + 1];
    }
    if (Ctx* cur = context_at(srcnn_get_context())) (void)hipSetDevice(cur->device);
    return (int)n;
}

// the same for ONE context (which device is the straggler of a node-level call?)
int srcnn_profile_read_context(int context, int stage, double* total_ms, unsigned long long* launches)
{
    if (stage < 0 || stage >= SRCNN_STAGE_COUNT) return fail(SRCNN_E_ARG, "bad stage %d", stage);
    Ctx* cx = context_at(context);
    if (!cx) return fail(SRCNN_E_ARG, "no context %d", context);
    (void)hipSetDevice(cx->device);
    {
        std::lock_guard<std::mutex> lk(cx->mu);
        drain_spans_locked(*cx);
        if (total_ms) *total_ms = cx->stage_ms[stage];
        if (launches) *launches = cx->stage_n[stage];
    }
    if (Ctx* cur = context_at(srcnn_get_context())) (void)hipSetDevice(cur->device);
    return SRCNN_OK;
}

// ---- stage-level -------------------------------------------------------------------------------
int srcnn_resample_f32_dev(const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                           float* d_out, void* stream)
{
    int rc;
    if ((rc = check_y_path_args(d_in, w, h, dw, dh, filter, d_out))) return rc;
    if (dh > (1u << 20) || h > (1u << 20)) return fail(SRCNN_E_UNSUPPORTED, "too many rows");
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    rc = resample_rows_range(sc.c, d_in, w, h, dw, dh, filter, 0, dh, d_out);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return SRCNN_OK;
}

int srcnn_conv1_f32_dev(const float* d_y, unsigned w, unsigned h, float* d_c1, void* stream)
{
    int rc;
    if ((rc = check_plane(d_y, w, h, d_c1))) return rc;
    if (h > 65535u * 4u) return fail(SRCNN_E_UNSUPPORTED, "too many rows");
    if (!ctx_for_stream(stream)) return SRCNN_E_NODEVICE;
    launch_conv1_planes(d_y, (int)w, (int)h, d_c1, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SRCNN_OK;
}

int srcnn_conv2_f32_dev(const float* d_c1, unsigned w, unsigned h, float* d_c2, void* stream)
{
    int rc;
    if ((rc = check_plane(d_c1, w, h, d_c2))) return rc;
    if (!ctx_for_stream(stream)) return SRCNN_E_NODEVICE;
    launch_conv2_planes(d_c1, (size_t)w * h, d_c2, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SRCNN_OK;
}

int srcnn_conv3_f32_dev(const float* d_c2, unsigned w, unsigned h, float* d_out, void* stream)
{
    int rc;
    if ((rc = check_plane(d_c2, w, h, d_out))) return rc;
    if (h > kMaxGridRows) return fail(SRCNN_E_UNSUPPORTED, "too many rows");
    if (!ctx_for_stream(stream)) return SRCNN_E_NODEVICE;
    Call c;
    c.mode = G.mode.load();
    launch_conv3(d_c2, (size_t)w * h, (int)w, (int)h, 0, (int)h, d_out, 0, (int)h, c.relax(), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return SRCNN_OK;
}

int srcnn_conv12_f32_dev(const float* d_y, unsigned w, unsigned h, float* d_c2, void* stream)
{
    int rc;
    if ((rc = check_plane(d_y, w, h, d_c2))) return rc;
    if (h > 65535u * 4u) return fail(SRCNN_E_UNSUPPORTED, "too many rows");
    // On the stream's own workspace, like every path: run_conv12 draws tiles from the workspace's queue, and a call without a
    // workspace would deal them with the static stride -- not the form the hot path runs (tests/test_gpu_conv12_tile_loop.py).
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    run_conv12(sc.c, d_y, (int)w, (int)h, 0, (int)h, d_c2, (size_t)w * h, 0, (int)h);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
        sc.c.ws->queue_dirty = true;                   // re-zeroed on the launch stream before the next launch trusts it
        return fail(SRCNN_E_HIP, "srcnn_conv12_f32_dev: %s", hipGetErrorString(e));
    }
    return SRCNN_OK;
}

int srcnn_axis_table(int filter, unsigned dst_len, unsigned src_len, int* left, int* right, double* weights)
{
    if (dst_len == 0 || src_len == 0) return fail(SRCNN_E_ARG, "zero length");
    const srcnn::AxisTable t = srcnn::build_axis_table(filter, dst_len, src_len);
    if (left) memcpy(left, t.first.data(), sizeof(int) * dst_len);
    if (right) memcpy(right, t.last.data(), sizeof(int) * dst_len);
    if (weights) memcpy(weights, t.weight.data(), sizeof(double) * t.weight.size());
    return t.window;
}

// Diagnostic (tools/fused_timeline.py): the fused fp16 kernel on a device-resident UPSCALED plane with s_memtime stamps
// of workgroup 0 written to d_dbg (8 waves x 64 rows x 4 stamps: row start, layer 1 done, layers 2+3 done, row done).
int srcnn_fused_diag(const float* d_up, unsigned w, unsigned h, float* d_out, unsigned long long* d_dbg, void* stream)
{
    int rc;
    if ((rc = check_plane(d_up, w, h, d_out))) return rc;
#ifdef SRCNN_STRICT_ONLY
    (void)d_dbg; (void)stream;
    return fail(SRCNN_E_UNSUPPORTED, "strict-only build: the fused fp16 kernel is not compiled in");
#else
    Ctx* cx = ctx_for_stream(stream);
    if (!cx) return SRCNN_E_NODEVICE;
    launch_fused_f16(d_up, (int)w, (int)h, 0, (int)h, d_out, 0, (int)h, cx->fused_w.data(), cx->num_cus, (hipStream_t)stream, d_dbg);
    HIP_TRY(hipGetLastError());
    return SRCNN_OK;
#endif
}

// Test hook (tests/test_gpu_fused_f16_exact.py): the fused fp16 kernel, through the product's launcher, on output rows
// [out_row0, +out_rows) of an already upscaled w x h plane of which d_up holds rows [up_row0, +up_rows) -- with the product's
// weight image, or with one built here from a caller's blob by the product's own two packers.  Synchronous: the temporary
// weight image is freed before the call returns.
int srcnn_debug_fused_f16(const float* weights, const float* d_up, unsigned w, unsigned h, unsigned up_row0, unsigned up_rows,
                          float* d_out, unsigned out_row0, unsigned out_rows, void* stream)
{
    int rc;
    if ((rc = check_plane(d_up, w, h, d_out))) return rc;
    if (up_rows == 0 || out_rows == 0 || up_row0 >= h || up_rows > h - up_row0 || out_row0 >= h || out_rows > h - out_row0)
        return fail(SRCNN_E_ARG, "srcnn_debug_fused_f16: empty row range or rows outside the plane");
    const HaloSpan v = y_path_halo(h, out_row0, out_row0 + out_rows);
    if (up_row0 > v.ua || up_row0 + up_rows < v.ub)
        return fail(SRCNN_E_ARG, "srcnn_debug_fused_f16: staged rows [%u,%u) do not cover the halo [%u,%u) of output rows [%u,%u)", up_row0,
                    up_row0 + up_rows, v.ua, v.ub, out_row0, out_row0 + out_rows);
#ifdef SRCNN_STRICT_ONLY
    (void)weights; (void)stream;
    return fail(SRCNN_E_UNSUPPORTED, "strict-only build: the fused fp16 kernel is not compiled in");
#else
    Ctx* cx = ctx_for_stream(stream);
    if (!cx) return SRCNN_E_NODEVICE;
    DevBuf<FusedF16Weights> image;
    const FusedF16Weights* d_blob = cx->fused_w.data();
    if (weights) {
        auto dw = std::make_unique<DevWeights>();
        build_dev_weights(*dw, weights);
        auto fw = std::make_unique<FusedF16Weights>();
        build_fused_f16_weights(*dw, *fw);
        if ((rc = image.grow(1))) return rc;
        if ((rc = copy_h2d_any(*cx, image.data(), fw.get(), sizeof(FusedF16Weights), (hipStream_t)stream))) return rc;
        d_blob = image.data();
    }
    launch_fused_f16(d_up, (int)w, (int)h, (int)up_row0, (int)up_rows, d_out, (int)out_row0, (int)out_rows, d_blob, cx->num_cus,
                     (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(wait_stream((hipStream_t)stream));        // the image is freed on return
    return SRCNN_OK;
#endif
}

// The switches this process runs with (srcnn_settings.hpp): text into buf (NUL-terminated, truncated to cap), returns the
// length the full text needs.  markdown != 0: the rows of DESIGN.md section 6 (defaults, not current values).  No device needed.
int srcnn_debug_settings(char* buf, size_t cap, int markdown)
{
    const std::string t = settings().describe(markdown != 0);
    if (buf && cap) snprintf(buf, cap, "%s", t.c_str());
    return (int)t.size();
}

// test hook: number of cached contribution tables / of ProcessSRCNN lanes created so far, summed over the contexts
int srcnn_debug_counts(int* tables, int* lanes)
{
    int nt = 0, nl = 0;
    for (int k = 0; k < context_count(); ++k) {
        Ctx* cx = context_at(k);
        if (!cx) continue;
        { std::lock_guard<std::mutex> lk(cx->mu); nt += (int)cx->tables.size(); }
        { std::lock_guard<std::mutex> lk(cx->lane_mu); nl += (int)cx->lanes.size(); }
    }
    if (tables) *tables = nt;
    if (lanes) *lanes = nl;
    return SRCNN_OK;
}

}  // extern "C"
