// pt_jit_state.cpp -- the scene kernels at run time: a code object loaded as
// a HIP module, which of its kernels serves which stage, the process-wide
// code cache, and a context's builds on its PtJitState (topology build,
// values-baked tier-up, unload).
#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>

#include "pt_host.h"

bool pt_jit_load(const std::vector<char> &code, PtJitModule &m, std::string &err) {
    hipError_t e = hipModuleLoadData(&m.module, code.data());
    if (e != hipSuccess) {
        err = std::string("hipModuleLoadData: ") + hipGetErrorString(e);
        m.module = nullptr;
        return false;
    }
    for (const PtJitKernel &k : kJitKernels)
        if ((e = hipModuleGetFunction(&m.fn[k.fn], m.module, k.name)) != hipSuccess) {
            err = std::string("hipModuleGetFunction: ") + hipGetErrorString(e);
            pt_jit_unload(m);
            return false;
        }
    return true;
}

void pt_jit_unload(PtJitModule &m) {
    if (m.module) (void)hipModuleUnload(m.module);
    m.module = nullptr;
    std::fill(m.fn, m.fn + kJitFnCount, nullptr);
    m.key.clear();
}

hipFunction_t pt_jit_select(const PtJitModule &m, PtJitStage stage, bool stats, bool posed, bool taps_shade,
                            bool gen_norec) {
    switch (stage) {
        case PtJitStage::Render: return m.fn[stats ? kJitRenderStats : kJitRender];
        // (the instrumented gen kernel serves both cameras)
        case PtJitStage::Gen: return m.fn[stats ? kJitGenStats : (posed ? kJitGenC : kJitGen)];
        case PtJitStage::Trace:
            return taps_shade ? m.fn[stats ? kJitTraceMStats : kJitTraceM] : m.fn[stats ? kJitTraceStats : kJitTrace];
        case PtJitStage::TraceFirst: return m.fn[posed ? kJitTraceGC : kJitTraceG];
        case PtJitStage::Shade:  // (the table kernel's shade pass is the ahead-of-time one)
            if (!taps_shade) return nullptr;
            // shade pass 0 without ray records makes the camera rays again
            return m.fn[stats ? kJitShadeTStats : (posed && gen_norec ? kJitShadeTC : kJitShadeT)];
    }
    return nullptr;
}

// ---- a context's scene kernels: build, tier-up, unload ---------------------------
namespace {

// code objects by generated source, shared by every context of the process
std::map<std::string, PtJitBuild> &jit_cache() {
    static std::map<std::string, PtJitBuild> cache;
    return cache;
}
std::mutex &jit_mutex() {
    static std::mutex m;
    return m;
}

// Code object for a generated source: from the process-wide cache, else
// from the on-disk cache or compiled (without holding the cache lock).
PtJitBuild jit_code(const std::string &src, std::string &log) {
    PtJitBuild b;
    {
        std::lock_guard<std::mutex> g(jit_mutex());
        auto it = jit_cache().find(src);
        if (it != jit_cache().end()) {
            b = it->second;
            b.seconds = 0.0;
            return b;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    bool disk = false;
    if (!pt_jit_compile_source(src, b.code, log, &disk)) b.code.clear();
    b.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    b.from = disk ? kJitDisk : kJitCompiled;
    if (!b.code.empty()) {
        std::lock_guard<std::mutex> g(jit_mutex());
        jit_cache()[src] = b;
    }
    return b;
}

}  // namespace

void pt_jit_poll(PtJitState &j, bool wait) {
    if (j.tier_job.valid() &&
        (wait || j.tier_job.wait_for(std::chrono::seconds(0)) == std::future_status::ready)) {
        PtJitBuild done = j.tier_job.get();
        j.tier_seconds = done.seconds;
        if (done.code.empty()) j.tier_failed = j.tier_job_src;
        if (!done.code.empty() && j.tier_job_src == j.tier_want && !j.tier.module) {
            std::string err;
            if (pt_jit_load(done.code, j.tier, err)) {
                j.tier.key = j.tier_job_src;
                j.tier_from = done.from;
            } else {
                j.log = err;
                j.tier_failed = j.tier_job_src;
            }
        }
        j.tier_job_src.clear();
    }
    if (!j.tier_job.valid() && !j.tier_want.empty() && j.tier.key != j.tier_want && j.tier_want != j.tier_failed) {
        std::string src = j.tier_want;
        j.tier_job_src = src;
        j.tier_job = std::async(std::launch::async, [src]() {
            std::string log;
            return jit_code(src, log);
        });
        if (wait) pt_jit_poll(j, true);
    }
}

const PtJitModule *pt_jit_active(const PtJitState &j) {
    if (j.tier.module) return &j.tier;
    return j.mod.module ? &j.mod : nullptr;
}

void pt_jit_disable(PtJitState &j) {
    pt_jit_unload(j.mod);
    pt_jit_unload(j.tier);
    j.tier_want.clear();
}

void pt_jit_destroy(PtJitState &j) {
    if (j.tier_job.valid()) j.tier_job.wait();
    pt_jit_unload(j.mod);
    pt_jit_unload(j.tier);
}

void pt_jit_refresh(PtJitState &j, const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes,
                    bool fast_bounds) {
    if (!j.enabled) return pt_jit_disable(j);
    const int bake = j.bake;
    std::string src = pt_jit_source(nodes, boxes, fast_bounds, bake == 1);
    // the tier-up build for these values (bake 2); a stale one is dropped
    j.tier_want = bake == 2 ? pt_jit_source(nodes, boxes, fast_bounds, true) : std::string();
    if (j.tier.module && j.tier.key != j.tier_want) pt_jit_unload(j.tier);
    if (!(j.mod.module && j.mod.key == src)) {
        pt_jit_unload(j.mod);
        std::string log;
        PtJitBuild b = jit_code(src, log);
        j.seconds = b.seconds;
        if (b.code.empty()) {
            j.log = "hipRTC compile failed: " + log;
            return;
        }
        std::string err;
        if (!pt_jit_load(b.code, j.mod, err)) {
            j.log = err;
            return;
        }
        j.mod.key = std::move(src);
        j.from = b.from;
        j.log.clear();
    }
    if (bake == 2) pt_jit_poll(j, false);
}
