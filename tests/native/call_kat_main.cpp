// Known-answer test of csrc/tt_call_host.h, the pure part of the launch paths' call contract: a stand-alone
// program (built by tests/test_call_host.py with the host sanitizers) that runs a table of rows through the
// steps in the order tt_dispatch.hip runs them and compares status, text and plan with the row's expectation.
//
// One row per line, tab-separated:
//   name path have_args n_rays width height bounce flags count_given count_on_device ptr_a ptr_b ptr_c
//   status text plan            (plan: "wh off dst dev async stats", or "-" when the row is refused)
// path: trace | heightmap | shadow | shadow_heightmap | enqueue
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tt_call_host.h"

namespace {

struct Result {
    tt_status status = TT_OK;
    std::string text;
    std::string plan = "-";
};

std::string plan_text(uint64_t wh, uint32_t off, uint32_t dst, bool dev, bool async, bool stats) {
    char buf[128];
    std::snprintf(buf, sizeof(buf), "%" PRIu64 " %u %u %d %d %d", wh, off, dst, dev ? 1 : 0, async ? 1 : 0, stats ? 1 : 0);
    return buf;
}

Result refused(const tt_call::Refusal& r) {
    Result out;
    out.status = r.status;
    out.text = r.text;
    return out;
}

Result run(const std::string& path, bool have_args, const tt_call::Common& q, bool count_given, bool count_on_device,
           const void* a, const void* b, const void* c) {
    Result out;
    if (path == "enqueue") {
        const tt_call::EnqueuePlan pl = tt_call::check_enqueue(have_args, q, count_given);
        if (pl.refusal) return refused(pl.refusal);
        out.plan = plan_text(pl.wh, pl.src, pl.dst, pl.dev, false, false);
        return out;
    }
    const tt_call::Path* p = path == "trace"              ? &tt_call::kTrace
                             : path == "heightmap"        ? &tt_call::kHeightmap
                             : path == "shadow"           ? &tt_call::kShadow
                             : path == "shadow_heightmap" ? &tt_call::kShadowHeightmap
                                                          : nullptr;
    if (!p) {
        std::fprintf(stderr, "unknown path %s\n", path.c_str());
        std::exit(2);
    }
    if (const tt_call::Refusal r = tt_call::check_shape(*p, have_args, q)) return refused(r);
    const tt_call::Plan pl = tt_call::plan_call(*p, q, count_given, count_on_device);
    if (pl.refusal) return refused(pl.refusal);
    out.plan = plan_text(pl.wh, pl.off, 0, pl.dev, pl.async, pl.want_stats);
    if (q.n_rays == 0) return out;  // TT_OK before the alignment check
    if (const tt_call::Refusal r = tt_call::check_alignment(*p, a, b, c)) return refused(r);
    return out;
}

std::vector<std::string> split_tabs(const std::string& line) {
    std::vector<std::string> f;
    std::stringstream ss(line);
    std::string cell;
    while (std::getline(ss, cell, '\t')) f.push_back(cell);
    if (!line.empty() && line.back() == '\t') f.push_back("");
    return f;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s table.tsv\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    unsigned rows = 0, bad = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        const std::vector<std::string> f = split_tabs(line);
        if (f.size() != 16) {
            std::fprintf(stderr, "row %u: %zu fields\n", rows, f.size());
            return 2;
        }
        tt_call::Common q;
        q.n_rays = (uint32_t)std::strtoull(f[3].c_str(), nullptr, 0);
        q.screen_width = (uint32_t)std::strtoull(f[4].c_str(), nullptr, 0);
        q.screen_height = (uint32_t)std::strtoull(f[5].c_str(), nullptr, 0);
        q.bounce = (int32_t)std::strtoll(f[6].c_str(), nullptr, 0);
        q.flags = (uint32_t)std::strtoull(f[7].c_str(), nullptr, 0);
        const void* ptr[3];  // (values only: never dereferenced)
        for (int k = 0; k < 3; k++) ptr[k] = reinterpret_cast<const void*>((uintptr_t)std::strtoull(f[10 + k].c_str(), nullptr, 0));
        const Result r = run(f[1], f[2] == "1", q, f[8] == "1", f[9] == "1", ptr[0], ptr[1], ptr[2]);
        const tt_status want = (tt_status)std::atoi(f[13].c_str());
        rows++;
        if (r.status != want || r.text != f[14] || r.plan != f[15]) {
            bad++;
            std::printf("MISMATCH %s: got (%d, \"%s\", %s), want (%d, \"%s\", %s)\n", f[0].c_str(), (int)r.status,
                        r.text.c_str(), r.plan.c_str(), (int)want, f[14].c_str(), f[15].c_str());
        }
    }
    std::printf("%u rows, %u mismatches\n", rows, bad);
    return bad ? 1 : 0;
}
