// tt_call_host.h — the pure part of a launch's call contract (no HIP: a host compiler builds it, and
// tests/native/call_kat_main.cpp runs it under the host sanitizers). The four ray-launch paths of
// tt_dispatch.hip check their arguments in three steps, with each path's own checks (NaN far_plane, missing
// atlases, hits_out, ...) between the first and the second and the device-memory checks after the third:
//   check_shape      null arguments, zero screen, negative bounce
//   plan_call        screen and ray-window ranges, the flag decode, the device-count refusals
//   (the caller zeroes `stats` and returns TT_OK for n_rays == 0)
//   check_alignment  16-byte alignment of the arrays the kernels load with 128-bit accesses
// The first violated condition decides status and text. Where the paths word a refusal differently the
// wording comes from the path's descriptor. The bounce enqueue has a contract of its own: check_enqueue.
#ifndef TT_CALL_HOST_H
#define TT_CALL_HOST_H
#include <cstdint>

#include "../../include/truetrace_hip.h"

namespace tt_call {

struct Path {
    const char* null_args;    // params or the ray array missing
    const char* misaligned;
    bool ray_window;          // rays live at (bounce odd ? W*H : 0) of a 2 W*H array: offset + n_rays must fit 32 bits
    bool takes_stats;         // the path has a TT_TRACE_STATS form (refused with a device count)
};
constexpr Path kTrace{"null params or rays", "GlobalRays / _PrimaryTriangleInfo must be 16-byte aligned", true, true};
constexpr Path kHeightmap = kTrace;
constexpr Path kShadow{"null params or shadow rays", "shadow rays / visibility / NEEPosA must be 16-byte aligned", false, true};
constexpr Path kShadowHeightmap{kShadow.null_args, kShadow.misaligned, false, false};

struct Refusal {
    tt_status status = TT_OK;
    const char* text = "";
    explicit operator bool() const { return status != TT_OK; }
};
inline Refusal refuse(const char* text) {
    Refusal r;
    r.status = TT_ERR_INVALID_ARG;
    r.text = text;
    return r;
}

// the five fields tt_trace_params and tt_shadow_params have in common
struct Common {
    uint32_t n_rays = 0, screen_width = 0, screen_height = 0;
    int32_t bounce = 0;
    uint32_t flags = 0;
};
template <class Params>
Common common_of(const Params& p) {
    Common q;
    q.n_rays = p.n_rays;
    q.screen_width = p.screen_width;
    q.screen_height = p.screen_height;
    q.bounce = p.bounce;
    q.flags = p.flags;
    return q;
}

// have_args: params and the ray array are both there (q is only read when they are)
inline Refusal check_shape(const Path& path, bool have_args, const Common& q) {
    if (!have_args) return refuse(path.null_args);
    if (q.screen_width == 0 || q.screen_height == 0) return refuse("zero screen size");
    if (q.bounce < 0) return refuse("negative bounce");
    return Refusal{};
}

struct Plan {
    Refusal refusal;
    uint64_t wh = 0;    // pixels
    uint32_t off = 0;   // first ray of the launch's window (0 on the paths without one)
    bool dev = false, async = false, want_stats = false;
};

// count_given: the call carries a device-resident ray count; count_on_device: that pointer is device memory
inline Plan plan_call(const Path& path, const Common& q, bool count_given, bool count_on_device) {
    Plan pl;
    pl.wh = (uint64_t)q.screen_width * q.screen_height;
    if (pl.wh > 0x7fffffffull) {
        pl.refusal = refuse("screen too large");
        return pl;
    }
    if (path.ray_window) {
        pl.off = (q.bounce % 2 == 1) ? (uint32_t)pl.wh : 0u;
        if ((uint64_t)pl.off + q.n_rays > 0xffffffffull) {
            pl.refusal = refuse("ray range overflows");
            return pl;
        }
    }
    pl.dev = (q.flags & TT_TRACE_DEVICE_PTRS) != 0;
    pl.async = pl.dev && ((q.flags & TT_TRACE_ASYNC) || count_given);
    pl.want_stats = (q.flags & TT_TRACE_STATS) != 0;
    if (count_given) {
        if (!pl.dev)
            pl.refusal = refuse("a device-resident ray count needs TT_TRACE_DEVICE_PTRS");
        else if (path.takes_stats && pl.want_stats)
            pl.refusal = refuse("TT_TRACE_STATS needs a host ray count");
        else if (!count_on_device)
            pl.refusal = refuse("the ray count pointer is not device memory");
    }
    return pl;
}

// a, b, c: the arrays that must be 16-byte aligned (null: not passed)
inline Refusal check_alignment(const Path& path, const void* a, const void* b = nullptr, const void* c = nullptr) {
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16) return refuse(path.misaligned);
    return Refusal{};
}

// tt_enqueue_diffuse_bounce(_indirect): survivors of the rays at `src` are written from `dst` on
struct EnqueuePlan {
    Refusal refusal;
    uint64_t wh = 0;
    uint32_t src = 0, dst = 0;
    bool dev = false;
};
// have_args: params, rays and one of the two survivor-count outputs; counts_given: a device-resident count in or out
inline EnqueuePlan check_enqueue(bool have_args, const Common& q, bool counts_given) {
    EnqueuePlan pl;
    if (!have_args) {
        pl.refusal = refuse("null argument");
        return pl;
    }
    pl.wh = (uint64_t)q.screen_width * q.screen_height;
    if (!pl.wh || pl.wh > 0x7fffffffull || q.n_rays > pl.wh) {
        pl.refusal = refuse("bad ray count / screen");
        return pl;
    }
    const bool odd = q.bounce % 2 == 1;
    pl.src = odd ? (uint32_t)pl.wh : 0u;
    pl.dst = odd ? 0u : (uint32_t)pl.wh;
    pl.dev = (q.flags & TT_TRACE_DEVICE_PTRS) != 0;
    if (counts_given && !pl.dev) pl.refusal = refuse("device-resident ray counts need TT_TRACE_DEVICE_PTRS");
    return pl;
}

}  // namespace tt_call
#endif
