// pt_map_probe.hip -- the probe entry points of include/pt_abi.h: pt_probe_map,
// pt_probe_taps, pt_probe_bounds.  Test infrastructure: a
// scene's map() variants and bounds() on caller-supplied inputs, results per
// input.  PT_PROBE_INTERP runs the ahead-of-time kernels below (InterpMap,
// bounds_mask); PT_PROBE_TABLE / PT_PROBE_BAKED run the scene's generated code
// in a probe module (pt_jit.cpp pt_probe_source: the scene's source and the
// one kernel the call needs), compiled with hipRTC on first use, once per
// distinct source per context, outside the on-disk cache.
// Every launch on the context's stream; nothing here touches an image, the
// scene kernels or an option.
#include <chrono>
#include <cstring>

#include "pt_ctx.h"
#include "pt_map_probe.h"

namespace pt {

// the interpreter's six taps: six plain evaluations
struct InterpTaps {
    static __device__ __forceinline__ uint64_t alive(uint64_t) { return ~0ull; }
    template <bool ST>
    static __device__ __forceinline__ Hit first(const PtLaunch &L, float qx, float qy, float qz, const Check &ck,
                                                float bnd, float bndw, uint64_t &live, Stats<ST> &st) {
        return InterpMap::eval<ST>(L, qx, qy, qz, ck, bnd, bndw, live, st);
    }
    template <bool ST>
    static __device__ __forceinline__ Hit rest(const PtLaunch &L, float qx, float qy, float qz, const Check &ck,
                                               float bnd, float bndw, uint64_t &live, Stats<ST> &st) {
        return InterpMap::eval<ST>(L, qx, qy, qz, ck, bnd, bndw, live, st);
    }
};

template <bool ST>
__global__ __launch_bounds__(64) void probe_map_interp(PtProbe P) {
    probe_map_body<InterpMap, ST>(P);
}
template <bool ST>
__global__ __launch_bounds__(64) void probe_taps_interp(PtProbe P) {
    probe_taps_body<InterpTaps, ST>(P);
}
template <bool ST>
__global__ __launch_bounds__(64) void probe_bounds_interp(PtProbe P) {
    probe_bounds_body<InterpMap, ST>(P);
}

}  // namespace pt

namespace {

void unload(PtProbeModule &m) {
    if (m.module) (void)hipModuleUnload(m.module);
    m = PtProbeModule{};
}

// The probe module of kernel (fn, stats) for the context's scene as uploaded
// (kind: table or baked values): loaded already, or compiled and loaded now.
// A failed build leaves its log on the context (pt_jit_log).
int probe_module(pt_ctx *c, int kind, PtProbeFn fn, bool stats, const PtProbeModule *&out) {
    pt_ctx::Probe &pb = c->probe;
    std::string src = pt_probe_source(c->prog.host_nodes, c->prog.host_boxes, c->prog.fast_bounds, kind == PT_PROBE_BAKED,
                                      fn, stats);
    auto it = pb.mods.find(src);
    if (it != pb.mods.end()) {
        out = &it->second;
        return PT_OK;
    }
    // (a context edited through many baked sources keeps the last modules only)
    if (pb.mods.size() >= 64) {
        for (auto &kv : pb.mods) unload(kv.second);
        pb.mods.clear();
    }
    std::vector<char> code;
    std::string log;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = pt_probe_compile(src, code, log);
    pb.seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    pb.compiles += 1;
    if (!ok) {
        c->jit.log = "probe module: hipRTC compile failed: " + log;
        return fail(c, PT_ERR_HIP, "the probe module did not compile (pt_jit_log has the log)");
    }
    PtProbeModule m;
    hipError_t e = hipModuleLoadData(&m.module, code.data());
    for (const PtProbeKernel &k : kProbeKernels)
        if (k.fn == fn && e == hipSuccess)
            e = hipModuleGetFunction(&m.fn, m.module, (std::string(k.name) + (stats ? "_stats" : "")).c_str());
    if (e != hipSuccess) {
        unload(m);
        c->jit.log = std::string("probe module: ") + hipGetErrorString(e);
        return fail(c, PT_ERR_HIP, c->jit.log);
    }
    out = &pb.mods.emplace(std::move(src), m).first->second;
    return PT_OK;
}

// one probe call: what to stage in, what to bring back
struct Io {
    const void *in[pt_ctx::Probe::kBufs] = {};
    void *out[pt_ctx::Probe::kBufs] = {};
    size_t bytes[pt_ctx::Probe::kBufs] = {};
};

int run(pt_ctx *c, int kind, PtProbeFn fn, uint32_t n, int union_mode, int skip_mode, const Io &io, uint64_t *counters) {
    using B = pt_ctx::Probe;
    HIPCHK(c, hipSetDevice(c->device));
    const PtProbeModule *mod = nullptr;
    int rc;
    const bool st = counters != nullptr;
    if (kind != PT_PROBE_INTERP && (rc = probe_module(c, kind, fn, st, mod)) != PT_OK) return rc;
    B &pb = c->probe;
    void *dev[B::kBufs] = {};
    for (int k = 0; k < B::kBufs; ++k) {
        if (!io.in[k] && !io.out[k]) continue;
        if ((rc = ensure(c, pb.buf[k], io.bytes[k])) != PT_OK) return rc;
        dev[k] = pb.buf[k].p;
        if (io.in[k]) HIPCHK(c, hipMemcpyAsync(dev[k], io.in[k], io.bytes[k], hipMemcpyHostToDevice, c->stream));
    }
    PtProbe P;
    std::memset(&P, 0, sizeof P);
    P.L.nodes = c->prog.nodes.as<PtNode>();
    P.L.aabbs = c->prog.boxes.as<PtAabb>();
    P.L.mats = c->prog.mats.as<PtMat>();
    P.L.n_nodes = int32_t(c->prog.ops.size());
    P.L.n_aabb = int32_t(c->prog.aabbs.size());
    P.L.fast_bounds = c->prog.fast_bounds ? 1 : 0;
    P.L.bound_k = c->prog.bound_k;
    if (counters) {
        HIPCHK(c, hipMemsetAsync(c->prog.stats.p, 0, sizeof(unsigned long long) * PT_ST_COUNT, c->stream));
        P.L.stats = c->prog.stats.as<unsigned long long>();
    }
    P.xyz = static_cast<const float *>(dev[B::kXyz]);
    P.rd = static_cast<const float *>(dev[B::kRd]);
    P.check = static_cast<const uint64_t *>(dev[B::kCheck]);
    P.bnd = static_cast<const float *>(dev[B::kBnd]);
    P.live_in = static_cast<const uint64_t *>(dev[B::kLiveIn]);
    P.d = static_cast<float *>(dev[B::kD]);
    P.shape = static_cast<int32_t *>(dev[B::kShape]);
    P.live_out = static_cast<uint64_t *>(dev[B::kLiveOut]);
    P.mask = static_cast<uint4 *>(dev[B::kMask]);
    P.skip = static_cast<uint64_t *>(dev[B::kSkip]);
    P.n = n;
    P.union_mode = union_mode;
    P.skip_mode = skip_mode;
    const unsigned grid = unsigned((uint64_t(n) + 63u) / 64u);
    if (mod) {
        void *args[] = {&P};
        HIPCHK(c, hipModuleLaunchKernel(mod->fn, grid, 1, 1, 64, 1, 1, 0, c->stream, args, nullptr));
    } else {
        const dim3 g(grid), b(64);
        if (fn == kProbeTaps) {
            if (st) hipLaunchKernelGGL(pt::probe_taps_interp<true>, g, b, 0, c->stream, P);
            else hipLaunchKernelGGL(pt::probe_taps_interp<false>, g, b, 0, c->stream, P);
        } else if (fn == kProbeBounds) {
            if (st) hipLaunchKernelGGL(pt::probe_bounds_interp<true>, g, b, 0, c->stream, P);
            else hipLaunchKernelGGL(pt::probe_bounds_interp<false>, g, b, 0, c->stream, P);
        } else {  // (the interpreter has one map(): every variant is InterpMap)
            if (st) hipLaunchKernelGGL(pt::probe_map_interp<true>, g, b, 0, c->stream, P);
            else hipLaunchKernelGGL(pt::probe_map_interp<false>, g, b, 0, c->stream, P);
        }
        HIPCHK(c, hipGetLastError());
    }
    for (int k = 0; k < B::kBufs; ++k)
        if (io.out[k]) HIPCHK(c, hipMemcpyAsync(io.out[k], dev[k], io.bytes[k], hipMemcpyDeviceToHost, c->stream));
    unsigned long long host[PT_ST_COUNT] = {};
    if (counters) HIPCHK(c, hipMemcpyAsync(host, c->prog.stats.p, sizeof host, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (counters)
        for (int k = 0; k < PT_STAT_COUNT; ++k) counters[k] = k < PT_ST_COUNT ? host[k] : 0;
    return PT_OK;
}

bool bad_kind(int kind) { return kind != PT_PROBE_INTERP && kind != PT_PROBE_TABLE && kind != PT_PROBE_BAKED; }

}  // namespace

void pt_probe_unload(pt_ctx *c) {
    for (auto &kv : c->probe.mods) unload(kv.second);
    c->probe.mods.clear();
}

extern "C" {

int pt_probe_map(pt_ctx *c, int kind, int variant, uint32_t n, const float *xyz, const uint64_t *check, const float *bnd,
                 const uint64_t *live_in, int union_mode, float *d, int32_t *shape, uint64_t *live_out,
                 uint64_t *counters) {
    using B = pt_ctx::Probe;
    if (!c) return PT_ERR_INVALID;
    if (n && !xyz) return fail(c, PT_ERR_INVALID, "null points");
    if (bad_kind(kind) || variant < PT_PROBE_MAP || variant > PT_PROBE_MAP_B1 || (union_mode != 0 && union_mode != 1))
        return fail(c, PT_ERR_INVALID, "bad probe kind, map variant or union mode");
    if (!c->prog.have_program || !c->prog.have_data) return fail(c, PT_ERR_STATE, "no program/data uploaded");
    if (!n) return PT_OK;
    Io io;
    const size_t N = n;
    io.in[B::kXyz] = xyz, io.bytes[B::kXyz] = N * 12;
    io.in[B::kCheck] = check, io.bytes[B::kCheck] = N * 16;
    io.in[B::kBnd] = bnd, io.bytes[B::kBnd] = N * 4;
    io.in[B::kLiveIn] = live_in, io.bytes[B::kLiveIn] = N * 8;
    io.out[B::kD] = d, io.bytes[B::kD] = N * 4;
    io.out[B::kShape] = shape, io.bytes[B::kShape] = N * 4;
    io.out[B::kLiveOut] = live_out, io.bytes[B::kLiveOut] = N * 8;
    const PtProbeFn fn = variant == PT_PROBE_MAP ? kProbeMap : (variant == PT_PROBE_MAP_B0 ? kProbeMapB0 : kProbeMapB1);
    return run(c, kind, fn, n, union_mode, 0, io, counters);
}

int pt_probe_taps(pt_ctx *c, int kind, uint32_t n, const float *hit, const uint64_t *check, const float *bnd, float *d6,
                  int32_t *shape6, uint64_t *live, uint64_t *counters) {
    using B = pt_ctx::Probe;
    if (!c) return PT_ERR_INVALID;
    if (n && !hit) return fail(c, PT_ERR_INVALID, "null hit points");
    if (bad_kind(kind)) return fail(c, PT_ERR_INVALID, "bad probe kind");
    if (!c->prog.have_program || !c->prog.have_data) return fail(c, PT_ERR_STATE, "no program/data uploaded");
    if (!n) return PT_OK;
    Io io;
    const size_t N = n;
    io.in[B::kXyz] = hit, io.bytes[B::kXyz] = N * 12;
    io.in[B::kCheck] = check, io.bytes[B::kCheck] = N * 16;
    io.in[B::kBnd] = bnd, io.bytes[B::kBnd] = N * 4;
    io.out[B::kD] = d6, io.bytes[B::kD] = N * 24;
    io.out[B::kShape] = shape6, io.bytes[B::kShape] = N * 24;
    io.out[B::kLiveOut] = live, io.bytes[B::kLiveOut] = N * 8;
    return run(c, kind, kProbeTaps, n, 0, 0, io, counters);
}

int pt_probe_bounds(pt_ctx *c, int kind, uint32_t n, const float *ro, const float *rd, int skip_mode, uint32_t *mask,
                    uint64_t *skip, uint64_t *counters) {
    using B = pt_ctx::Probe;
    if (!c) return PT_ERR_INVALID;
    if (n && (!ro || !rd || !mask)) return fail(c, PT_ERR_INVALID, "null rays or mask");
    if (bad_kind(kind) || (skip_mode != 0 && skip_mode != 1)) return fail(c, PT_ERR_INVALID, "bad probe kind or skip mode");
    if (!c->prog.have_program || !c->prog.have_data) return fail(c, PT_ERR_STATE, "no program/data uploaded");
    if (!n) return PT_OK;
    Io io;
    const size_t N = n;
    io.in[B::kXyz] = ro, io.bytes[B::kXyz] = N * 12;
    io.in[B::kRd] = rd, io.bytes[B::kRd] = N * 12;
    io.out[B::kMask] = mask, io.bytes[B::kMask] = N * 16;
    if (skip_mode) io.out[B::kSkip] = skip, io.bytes[B::kSkip] = ((N + 63) / 64) * 8;
    return run(c, kind, kProbeBounds, n, 0, skip_mode, io, counters);
}

}  // extern "C"
