// order_probe.hip — drives tt_order_kernel (csrc/tt_order.hip) directly with host-supplied costs
// (tests/test_gpu_order_pin.py). Linked with the package's own build/tt_order.o, unchanged: through a trace the
// kernel only ever sees what a scene produces (at most 1000, a few dozen distinct values).
//
// tt_order_probe: `cost` (n_chunks words) is uploaded; the device `order` starts as TT_PROBE_SENTINEL in every
// word, the device `cost_clear` as the caller's cost_clear_inout. Both sit between two guard regions of
// TT_PROBE_GUARD words each. After tt_launch_order and a synchronise, order, cost_clear and (cost_after) the cost
// buffer are copied back, and guards_out receives the four guard regions in the order: before order, after order,
// before cost_clear, after cost_clear (4 * TT_PROBE_GUARD words, each TT_PROBE_GUARD_WORD when untouched).
// Returns the first hipError_t that was not hipSuccess, else hipSuccess.
#include <vector>

#include "tt_device.h"

#define TT_PROBE_GUARD 64u
#define TT_PROBE_GUARD_WORD 0xC0DEFACEu
#define TT_PROBE_SENTINEL 0xFFFFFFFFu

namespace {
struct DeviceWords {
    uint32_t* p = nullptr;
    ~DeviceWords() {
        if (p) (void)hipFree(p);
    }
};
}  // namespace

extern "C" int tt_order_probe(const uint32_t* cost, uint32_t n_rays, uint32_t n_chunks, uint32_t hot, uint32_t* order_out,
                              uint32_t* cost_clear_inout, uint32_t* cost_after, uint32_t* guards_out) {
    if (!cost || !order_out || !cost_clear_inout || !cost_after || !guards_out || n_chunks == 0u ||
        (n_rays + 63u) / 64u != n_chunks)
        return (int)hipErrorInvalidValue;
    const size_t G = TT_PROBE_GUARD, n = n_chunks, padded = n + 2 * G;
    DeviceWords d_cost, d_order, d_clear;
    hipError_t e;
#define PROBE_TRY(call)                   \
    do {                                  \
        e = (call);                       \
        if (e != hipSuccess) return (int)e; \
    } while (0)
    PROBE_TRY(hipMalloc(reinterpret_cast<void**>(&d_cost.p), n * sizeof(uint32_t)));
    PROBE_TRY(hipMalloc(reinterpret_cast<void**>(&d_order.p), padded * sizeof(uint32_t)));
    PROBE_TRY(hipMalloc(reinterpret_cast<void**>(&d_clear.p), padded * sizeof(uint32_t)));
    std::vector<uint32_t> h_order(padded, TT_PROBE_GUARD_WORD), h_clear(padded, TT_PROBE_GUARD_WORD);
    for (size_t i = 0; i < n; i++) {
        h_order[G + i] = TT_PROBE_SENTINEL;
        h_clear[G + i] = cost_clear_inout[i];
    }
    PROBE_TRY(hipMemcpy(d_cost.p, cost, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    PROBE_TRY(hipMemcpy(d_order.p, h_order.data(), padded * sizeof(uint32_t), hipMemcpyHostToDevice));
    PROBE_TRY(hipMemcpy(d_clear.p, h_clear.data(), padded * sizeof(uint32_t), hipMemcpyHostToDevice));
    OrderArgs a;
    a.cost = d_cost.p;
    a.cost_clear = d_clear.p + G;
    a.n_rays = n_rays;
    a.n_chunks = n_chunks;
    a.hot = hot;
    a.order = d_order.p + G;
    PROBE_TRY(tt_launch_order(a, nullptr));
    PROBE_TRY(hipDeviceSynchronize());
    PROBE_TRY(hipMemcpy(h_order.data(), d_order.p, padded * sizeof(uint32_t), hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(h_clear.data(), d_clear.p, padded * sizeof(uint32_t), hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(cost_after, d_cost.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
#undef PROBE_TRY
    for (size_t i = 0; i < n; i++) {
        order_out[i] = h_order[G + i];
        cost_clear_inout[i] = h_clear[G + i];
    }
    for (size_t i = 0; i < G; i++) {
        guards_out[i] = h_order[i];
        guards_out[G + i] = h_order[G + n + i];
        guards_out[2 * G + i] = h_clear[i];
        guards_out[3 * G + i] = h_clear[G + n + i];
    }
    return (int)hipSuccess;
}
