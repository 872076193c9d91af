// tt_api.hip — the C ABI of include/truetrace_hip.h, part one: the stream registry and exit teardown, context
// create / destroy, the timing ring, diagnostics and tt_sync. Scenes: tt_scene_api.hip; launches: tt_dispatch.hip.
#include <sys/syscall.h>
#include <unistd.h>

#include <atomic>
#include <cstdlib>
#include <thread>

#include "tt_ctx.h"
#include "tt_launch.h"

extern "C" {

int32_t tt_abi_version(void) { return TT_ABI_VERSION; }

int32_t tt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char* tt_last_error(const tt_ctx* c) { return c ? c->err.c_str() : "null context"; }

}  // extern "C"

// Streams made by tt_stream_create that the caller has not destroyed yet. A queue created with a CU mask
// that is still alive when the HIP runtime's own static destructors run takes the process down in
// __cxa_finalize (SIGSEGV, gpurun_out/qmap.out under rocprofv3), so the library destroys what is left
// from an exit handler. It is registered after the first stream is made -- after the HIP runtime has
// initialised and registered its own destructors -- and exit handlers run in reverse order of
// registration, so it runs before the runtime tears down. A host that destroys its streams (or a
// Unity domain reload that misses StreamDestroy) is covered either way.
namespace {
std::mutex g_streams_mu;
std::vector<std::pair<int, hipStream_t>> g_streams;
// streams the teardown (tt_shutdown, the exit handlers) destroyed under a context still holding them: such a
// context refuses launches and skips the stream sync in tt_ctx_destroy (a host's static destructors may
// destroy contexts after the teardown ran)
std::vector<hipStream_t> g_dead;
std::atomic<uint32_t> g_dead_n{0};
bool g_streams_handler = false;

void release_live_streams() {
    std::vector<std::pair<int, hipStream_t>> live;
    {
        std::lock_guard<std::mutex> lk(g_streams_mu);
        live.swap(g_streams);
        for (auto& ds : live) g_dead.push_back(ds.second);
        g_dead_n.store((uint32_t)g_dead.size());
    }
    for (auto& ds : live) {
        if (hipSetDevice(ds.first) != hipSuccess) continue;
        (void)hipStreamSynchronize(ds.second);
        (void)hipStreamDestroy(ds.second);
    }
    (void)hipGetLastError();
}

// The atexit form. exit() has already destroyed the exiting thread's thread_locals when atexit handlers
// run, and a profiler that wraps the HIP API (rocprofv3) keeps per-thread state its stream calls need
// ("'get_stream_stack()' Must be non nullptr", profiles/r05/lifecycle/atexit_only_abort_under_rocprofv3.txt):
// so the teardown runs on a fresh thread, whose thread state is created on its first HIP call.
void release_live_streams_at_exit() {
    {
        std::lock_guard<std::mutex> lk(g_streams_mu);
        if (g_streams.empty()) return;
    }
    std::thread t(release_live_streams);
    t.join();
}

bool is_lib_stream(hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    return std::any_of(g_streams.begin(), g_streams.end(), [s](const std::pair<int, hipStream_t>& ds) { return ds.second == s; });
}
}  // namespace

bool stream_dead(hipStream_t s) {
    if (g_dead_n.load(std::memory_order_relaxed) == 0) return false;
    std::lock_guard<std::mutex> lk(g_streams_mu);
    return std::find(g_dead.begin(), g_dead.end(), s) != g_dead.end();
}

namespace {
// A profiler that wraps the HIP API (rocprofv3's tool) keeps per-thread state that its stream calls need
// ("'get_stream_stack()' Must be non nullptr"), and exit() destroys a thread's thread_local objects BEFORE it
// runs any atexit handler: from the atexit handler alone, the hipStreamDestroy calls abort under the tool.
// So the teardown is armed a second way: a thread_local guard, constructed on the first launch on one of the
// library's streams (after the tool's own per-thread state exists, so destroyed before it: glibc runs a
// thread's TLS destructors in reverse order of construction), whose destructor tears the streams down when
// the MAIN thread's thread_locals are destroyed -- i.e. from exit() -- and does nothing when another thread
// ends (the process goes on). The atexit handler stays for a process whose launches all came from other
// threads; a second run finds the list empty.
bool stream_exit_handler_on() {
    static const bool on = [] {  // TT_STREAM_EXIT_HANDLER=0: diagnosis only (the exit-time teardown off)
        const char* e = std::getenv("TT_STREAM_EXIT_HANDLER");
        return !(e && e[0] == '0');
    }();
    return on;
}
struct MainThreadExitGuard {
    ~MainThreadExitGuard() {
        if ((pid_t)syscall(SYS_gettid) == getpid()) release_live_streams();
    }
};
}  // namespace
void note_stream_launch(hipStream_t s) {
    thread_local bool armed = false;
    if (armed || !stream_exit_handler_on()) return;
    {
        std::lock_guard<std::mutex> lk(g_streams_mu);
        if (std::none_of(g_streams.begin(), g_streams.end(), [s](const std::pair<int, hipStream_t>& ds) { return ds.second == s; }))
            return;
    }
    armed = true;
    thread_local MainThreadExitGuard guard;
    (void)&guard;
}

extern "C" {

tt_status tt_shutdown(void) {
    release_live_streams();
    return TT_OK;
}

uint32_t tt_stream_live_count(void) {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    return (uint32_t)g_streams.size();
}

tt_status tt_stream_create(int32_t device, void** stream) {
    if (!stream) return TT_ERR_INVALID_ARG;
    *stream = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return TT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) return TT_ERR_INVALID_ARG;
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return TT_ERR_HIP;
    hipDeviceProp_t prop;
    hipStream_t s = nullptr;
    tt_status st = TT_OK;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        st = TT_ERR_HIP;
    } else {
        // every CU enabled: the mask only exists to get a HW queue that no other stream shares
        std::vector<uint32_t> mask(((uint32_t)prop.multiProcessorCount + 31u) / 32u, 0xffffffffu);
        if (hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            st = TT_ERR_HIP;
        }
    }
    (void)hipSetDevice(prev);  // the caller's current device is left as it was
    if (st == TT_OK) {
        *stream = s;
        std::lock_guard<std::mutex> lk(g_streams_mu);
        g_streams.emplace_back(device, s);
        // (a new stream may reuse a destroyed one's handle)
        g_dead.erase(std::remove(g_dead.begin(), g_dead.end(), s), g_dead.end());
        g_dead_n.store((uint32_t)g_dead.size());
        if (!g_streams_handler && stream_exit_handler_on())
            g_streams_handler = std::atexit(release_live_streams_at_exit) == 0;
    }
    return st;
}

tt_status tt_stream_destroy(void* stream) {
    if (!stream) return TT_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        std::lock_guard<std::mutex> lk(g_streams_mu);
        auto it = std::find_if(g_streams.begin(), g_streams.end(),
                               [s](const std::pair<int, hipStream_t>& ds) { return ds.second == s; });
        if (it == g_streams.end()) return TT_ERR_INVALID_ARG;  // not ours, or destroyed already
        g_streams.erase(it);
    }
    const hipError_t a = hipStreamSynchronize(s);
    const hipError_t b = hipStreamDestroy(s);
    return (a == hipSuccess && b == hipSuccess) ? TT_OK : TT_ERR_HIP;
}

tt_status tt_ctx_create(const tt_config* cfg, tt_ctx** out) {
    if (!cfg || !out) return TT_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return TT_ERR_NO_DEVICE;
    }
    if (cfg->device < 0 || cfg->device >= ndev) return TT_ERR_INVALID_ARG;
    tt_ctx* c = new tt_ctx();
    c->device = cfg->device;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) {
        delete c;
        return TT_ERR_HIP;
    }
    if (cfg->stream) {
        c->stream = static_cast<hipStream_t>(cfg->stream);
        c->lib_stream = is_lib_stream(c->stream);
    } else {
        // blocking (default-flag) stream: ordered with the legacy NULL stream, so callers that
        // fill device buffers on it (torch's default stream) cannot race the engine
        if (hipStreamCreate(&c->stream) != hipSuccess) {
            delete c;
            return TT_ERR_HIP;
        }
        c->own_stream = true;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) {
        tt_ctx_destroy(c);
        return TT_ERR_HIP;
    }
    c->num_cus = prop.multiProcessorCount;
    int occ[24];
    (void)tt_trace_occupancy_table(occ);
    // Residency check beyond the occupancy API: measured on MI355X, five 32-KiB-LDS blocks were
    // not co-resident (the fifth started only when another exited), consistent with the LDS being
    // allocated per half-CU (2 x 80 KiB). Size every persistent grid so all its blocks are resident.
    // (per form: the leaf-TLAS kernels, grid_of[18..23], split their LDS between a shallower stack and a ray pool)
    auto lds_cap_of = [](bool leaf) {
        const uint32_t lds_block = tt_trace_lds_bytes(leaf);
        return lds_block ? 2 * (int)((80u * 1024u) / lds_block) : 8;
    };
    const int lds_cap = lds_cap_of(false), lds_cap_leaf = lds_cap_of(true);
    int knob = 0;
    if (const char* e = std::getenv("TT_BLOCKS_PER_CU")) knob = std::atoi(e);  // tuning/diagnostic knob
    // at most 32 waves per CU (8 blocks of 4 waves at the default 256-thread block)
    const int wpb = (int)std::max(1u, tt_trace_block_size() / 64u);
    const int block_cap = std::max(1, 32 / wpb);
    for (int k = 0; k < 24; k++) {
        int b = std::max(1, std::min(std::min(occ[k], k >= 18 ? lds_cap_leaf : lds_cap), block_cap));
        if (knob > 0 && knob < b) b = knob;
        c->grid_of[k] = (uint32_t)(c->num_cus * b);
    }
    int socc[4];
    tt_shadow_occupancy_table(socc);
    for (int k = 0; k < 4; k++) {
        int b = std::max(1, std::min(std::min(socc[k], lds_cap), block_cap));
        if (knob > 0 && knob < b) b = knob;
        c->shadow_grid_of[k] = (uint32_t)(c->num_cus * b);
    }
    c->blocks_per_cu = (int)(c->grid_of[1] / c->num_cus);
    c->grid = c->grid_of[1];
    uint32_t max_grid = 0;
    for (int k = 0; k < 24; k++) max_grid = std::max(max_grid, c->grid_of[k]);  // (the spill area: the largest grid)
    for (int k = 0; k < 4; k++) max_grid = std::max(max_grid, c->shadow_grid_of[k]);
    c->spill_threads = max_grid * tt_trace_block_size();
    // two control blocks + the sticky overflow counter behind them
    if (hipMalloc(reinterpret_cast<void**>(&c->ctl), 2 * sizeof(TraceControl) + 256) != hipSuccess) {
        tt_ctx_destroy(c);
        return TT_ERR_OOM;
    }
    c->sticky = reinterpret_cast<uint32_t*>(c->ctl + 2);
    if (hipMemset(c->ctl, 0, 2 * sizeof(TraceControl) + 256) != hipSuccess) {
        tt_ctx_destroy(c);
        return TT_ERR_HIP;
    }
    for (uint32_t i = 0; i < TT_RING; i++) {
        if (hipEventCreate(&c->ring0[i]) != hipSuccess || hipEventCreate(&c->ring1[i]) != hipSuccess) {
            tt_ctx_destroy(c);
            return TT_ERR_HIP;
        }
    }
    if (const uint32_t se = tt_trace_spill_entries()) {
        if (c->spill.alloc((size_t)se * c->spill_threads) != hipSuccess) {
            tt_ctx_destroy(c);
            return TT_ERR_OOM;
        }
    }
    c->max_rays = cfg->max_rays;
    if (c->max_rays) {
        if (c->st_rays.alloc(c->max_rays) != hipSuccess) {
            tt_ctx_destroy(c);
            return TT_ERR_OOM;
        }
    }
    *out = c;
    return TT_OK;
}

tt_status tt_ctx_destroy(tt_ctx* c) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (c->borrowers > 0) return fail(c, TT_ERR_INVALID_ARG, "other contexts share this scene: destroy them first");
    (void)hipSetDevice(c->device);
    if (c->stream && !(c->lib_stream && stream_dead(c->stream))) (void)hipStreamSynchronize(c->stream);
    unlink_borrower(c);
    if (c->ev_scene) (void)hipEventDestroy(c->ev_scene);
    if (c->ev_blas) (void)hipEventDestroy(c->ev_blas);
    if (c->ev_read) (void)hipEventDestroy(c->ev_read);
    tt_refit_free(c->refit);
    for (auto& kv : c->blas_refit) tt_refit_free(kv.second.dev);
    tt_refit_free(c->refit_many.dev);
    if (c->ctl) (void)hipFree(c->ctl);
    for (uint32_t i = 0; i < TT_RING; i++) {
        if (c->ring0[i]) (void)hipEventDestroy(c->ring0[i]);
        if (c->ring1[i]) (void)hipEventDestroy(c->ring1[i]);
    }
    for (auto& pn : c->pin) {
        if (pn.p) (void)hipHostFree(pn.p);
        if (pn.ev) (void)hipEventDestroy(pn.ev);
    }
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;  // (frees every DevBuf the context owns)
    return TT_OK;
}

tt_status tt_ctx_set_timing(tt_ctx* c, int32_t enabled) {
    if (!c) return TT_ERR_INVALID_ARG;
    c->timing = enabled != 0;
    return TT_OK;
}

tt_status tt_ctx_set_frame_pixels(tt_ctx* c, uint32_t frame_pixels) {
    if (!c) return TT_ERR_INVALID_ARG;
    if (frame_pixels > 0x7fffffffu) return fail(c, TT_ERR_INVALID_ARG, "frame_pixels above 2^31 - 1");
    c->frame_pixels = frame_pixels;
    return TT_OK;
}

tt_status tt_timing_reset(tt_ctx* c) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_HIP(c, hipStreamSynchronize(c->stream));
    c->ring_base = c->ring_n;
    return TT_OK;
}

tt_status tt_timing_read(tt_ctx* c, float* ms, uint32_t max, uint32_t* n) {
    if (!c || !n || (max && !ms)) return TT_ERR_INVALID_ARG;
    TT_HIP(c, hipStreamSynchronize(c->stream));
    const uint32_t total = c->ring_n - c->ring_base;
    const uint32_t avail = std::min(total, TT_RING);
    const uint32_t k = std::min(avail, max);
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t slot = (c->ring_n - avail + i) % TT_RING;
        TT_HIP(c, hipEventElapsedTime(&ms[i], c->ring0[slot], c->ring1[slot]));
    }
    *n = k;
    return TT_OK;
}

tt_status tt_trace_diagnostics(const tt_ctx* c, uint64_t* out8) {
    if (!c || !out8) return TT_ERR_INVALID_ARG;
    for (int k = 0; k < 8; k++) out8[k] = c->last_diag[k];
    return TT_OK;
}

tt_status tt_trace_last_form(const tt_ctx* c, uint32_t* form) {
    if (!c || !form) return TT_ERR_INVALID_ARG;
    *form = c->last_form;
    return TT_OK;
}

tt_status tt_tlas_root_form(const tt_cwbvh_node* node0, uint32_t* form) {
    if (!node0 || !form) return TT_ERR_INVALID_ARG;
    const RootLeaf r = root_leaf_of(reinterpret_cast<const uint32_t*>(node0));
    *form = root_one_instance(r) ? TT_ROOT_ONE_INSTANCE : r.ok ? TT_ROOT_ONE_LEAF : TT_ROOT_GENERIC;
    return TT_OK;
}

tt_status tt_selftest_rcp(tt_ctx* c, uint64_t* mismatches) {
    if (!c || !mismatches) return TT_ERR_INVALID_ARG;
    TT_HIP(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> bad;
    TT_HIP(c, bad.alloc(1));
    TT_HIP(c, hipMemsetAsync(bad.p, 0, sizeof(unsigned long long), c->stream));
    TT_HIP(c, tt_launch_rcp_selftest(bad.p, c->stream));
    unsigned long long h = 0;
    TT_HIP(c, hipMemcpyAsync(&h, bad.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    TT_HIP(c, hipStreamSynchronize(c->stream));
    *mismatches = (uint64_t)h;
    return TT_OK;
}

void* tt_ctx_stream(tt_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

tt_status tt_async_overflows(tt_ctx* c, uint64_t* count) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t n = 0;
    TT_HIP(c, hipMemcpy(&n, c->sticky, sizeof(n), hipMemcpyDeviceToHost));
    TT_HIP(c, hipMemset(c->sticky, 0, sizeof(n)));
    if (count) *count = n;
    if (n) return fail(c, TT_ERR_STACK_OVERFLOW, "%u rays needed more than %d traversal stack entries", n, TT_STACK_SIZE);
    return TT_OK;
}

tt_status tt_sync(tt_ctx* c) {
    if (!c) return TT_ERR_INVALID_ARG;
    TT_REFUSE_DEAD_STREAM(c);
    TT_HIP(c, hipStreamSynchronize(c->stream));
    return TT_OK;
}

}  // extern "C"
