// pt_host.h -- host-side internals shared by the runtime's host files (pt_runtime.hip, pt_post_host.cpp,
// pt_bin_host.cpp, pt_options.cpp, pt_derive.cpp), the scene-kernel generator (pt_jit.cpp), the scene kernels' hipRTC build and
// on-disk cache (pt_jit_build.cpp) and their loading and lifecycle (pt_jit_state.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <future>
#include <string>
#include <vector>

#include "pt_binned.h"
#include "pt_device.h"

// ahead-of-time scene kernels (pt_kernel.hip; the image-space kernels' launches are in pt_post.h).  moments: the
// simple kernel also mixes each frame's squared colour into the moment image (pt_set_option "moments", DESIGN.md
// 3.28; debug 0, write 1 only), nullptr: the simple or the wave kernel as L asks
bool pt_use_simple_kernel(const PtLaunch &L);
void pt_launch_render(const PtLaunch &L, bool stats, float *moments, hipStream_t stream);
// the binned pipeline's ahead-of-time kernels (pt_bin_kernels.hip)
enum class PtBinStage { Gen, Shade, Scan, Scatter, Trace };
void pt_launch_bin(PtBinStage stage, const PtPass &P, bool stats, unsigned grid, hipStream_t stream);
int pt_bin_trace_blocks_per_cu(bool stats);  // occupancy of the interpreter trace kernel
// the sky pass after a binned trace pass (pt_set_sky): P as that trace pass's shade pass takes it; quads: the
// trace pass wrote hit quads (taps in the shade pass), not hit records
void pt_launch_bin_sky(const PtPass &P, bool quads, unsigned grid, hipStream_t stream);
// the fold of a chunk; moments: it also keeps the moment image (as pt_launch_render; pt_bin_fold_m_kernel instead
// of pt_bin_fold_kernel), nullptr: the plain fold
void pt_launch_bin_fold(const PtPass &P, float *moments, unsigned grid, hipStream_t stream);
// the denoiser's guide images (pt_render_guides): L as a dispatch takes it, over every tile, a lens as its pinhole
void pt_launch_guides(const PtLaunch &L, float *g0, float *g1, hipStream_t stream);
// ray queries (pt_trace_rays / pt_pick_pixels): L as pt_launch_guides takes it; device pointers, any
// output nullptr.  rays: n caller rays, ro and rd [n][3].  pick: xy [n][2] pixels inside the image, answers in list
// order; or xy nullptr and n = L.n_tiles * 64 threads, one per tile pixel, answers in image order
#ifndef PT_RAYS_BLOCK              // (an A/B build may set it: build.build_variant)
#define PT_RAYS_BLOCK 64           // threads per block of both kernels (64 against 256: EXPERIMENTS.md)
#endif
void pt_launch_rays(const PtLaunch &L, const float *ro, const float *rd, uint32_t n, float *t, int32_t *shape, float *normal,
                    hipStream_t stream);
void pt_launch_pick(const PtLaunch &L, const int32_t *xy, uint32_t n, float *t, int32_t *shape, float *normal,
                    hipStream_t stream);
// radiance queries (pt_trace_radiance): one chunk of a call, whole rays.  L as a dispatch takes it
// (the sky kept), bounces the call's.  Three launches on `stream`: first (PT_RADIANCE_RAY only) marches each ray's
// first segment once into `first`; samples runs one path per (ray, sample) into `colour`; fold mixes each ray's
// colours in sample order into mean / moment.  Device pointers throughout.
#ifndef PT_RADIANCE_RAY_FASTEST    // (an A/B build may set it: build.build_variant)
#define PT_RADIANCE_RAY_FASTEST 0  // 0: a wave's lanes are successive samples of a ray; 1: successive rays of a sample (EXPERIMENTS.md)
#endif
struct PtRadiance {
    const float *ro, *rd;  // [n][3], every ray of the call
    float4 *first;         // [rays][2] of the chunk: {hit point, t}, {tap differences, material index or -1: not traced}
    float4 *colour;        // [rays][spp] of the chunk
    float *mean, *moment;  // [n][3], in / out; either nullptr
    uint32_t ray0, rays;   // the chunk's first ray in the call, and its ray count (rays * spp < 2^31)
    uint32_t spp, sample0, seed;
    int32_t mode;          // PT_RADIANCE_*
};
enum class PtRadianceStage { First, Samples, Fold };
void pt_launch_radiance(PtRadianceStage stage, const PtLaunch &L, const PtRadiance &R, hipStream_t stream);
// preview shading (pt_render_preview): L as pt_launch_guides takes it but with the sky kept; the
// caller's parameters as the host checked them, and the device image the texels go to, [height][width]
struct PtPreview {
    pt_preview_params p;
    float4 *out;
};
void pt_launch_preview(const PtLaunch &L, const PtPreview &V, hipStream_t stream);

// Expand (program, data[]) into the device tables (see pt_device.h).
int pt_derive(const std::vector<pt_op> &ops, const std::vector<pt_aabb> &aabbs, const float *data, uint32_t n,
              std::vector<PtNode> &nodes, std::vector<PtAabb> &boxes, std::vector<PtMat> &mats, std::string &err);

// Margin constant of the map() bound; NaN: no bound.
float pt_bound_k(const std::vector<PtNode> &nodes);

// Every box coordinate lies inside the reciprocal guard (pt_div_coord_ok): bounds() may take its slab values from
// reciprocal products (PtLaunch.fast_bounds).
bool pt_fast_bounds(const std::vector<PtAabb> &boxes);

// Scene-specialised kernels (hipRTC): a loaded code object and its kernels.
enum PtJitFn {
    kJitRender,       // pt_wave_jit: the tile-resident wave kernel
    kJitRenderStats,
    kJitTrace,        // binned pipeline trace pass (pt_binned.h)
    kJitTraceStats,
    kJitTraceM,       // march-only trace pass (normal taps in the shade pass)
    kJitTraceMStats,
    kJitShadeT,       // shade pass with the normal taps (JitMapB)
    kJitShadeTStats,
    kJitGen,          // camera rays + the scene's straight-line bounds()
    kJitGenStats,
    kJitTraceG,       // first pass with its own camera rays (PtPass gen_trace)
    // the kernels that make camera rays, built for a posed camera (pt_set_camera; pt_path.h PT_CAMK_POSED):
    // gen pass, first pass, shade pass 0 -- the ones above serve the fixed camera only
    kJitGenC,
    kJitTraceGC,
    kJitShadeTC,
    kJitFnCount
};
// The binned trace and shade kernels are built for 8 waves per SIMD (<= 64
// VGPRs); a kernel whose build spills is rebuilt at 7 (compile_with_fallback).
// With 28 trace waves per CU beside the other pipeline's passes, 8 + 8
// measured +1.5 % over 7 + 7 at 24 (DESIGN.md 5 history).
constexpr int kJitWaves = 8;
// the shade kernel's accepted spill, bytes per lane, before its 7-wave rebuild
constexpr long kShadeSpillOk = 16;
// The scene kernels, in the order the generated source defines them: what the generator emits for each
// (`extern "C" __global__ __launch_bounds__(bounds) [waves] void name(param) { body; }`), the name pt_jit_load
// looks up for `fn`, and, for the four kernels built to a register budget, the spill (scratch bytes per lane)
// beyond which compile_with_fallback rebuilds with `fallback`.
struct PtJitKernel {
    PtJitFn fn;
    const char *name, *bounds;
    const char *waves;  // the waves-per-SIMD attribute macro (pt_jit.cpp emit_waves_macros), or nullptr
    const char *param, *body;
    long spill_ok;
    const char *fallback;  // hipRTC option that lowers `waves` to 7, or nullptr: never rebuilt
};
inline constexpr PtJitKernel kJitKernels[] = {
    {kJitRender, "pt_wave_jit", "64", "PT_WAVES", "PtLaunch L", "pt::wave_body<pt::JitMap, false>(L)", 0, nullptr},
    {kJitRenderStats, "pt_wave_jit_stats", "64", nullptr, "PtLaunch L", "pt::wave_body<pt::JitMap, true>(L)", 0,
     nullptr},
    // PT_TT_N: the pass with the taps in it
    {kJitTrace, "pt_bin_trace_jit", "64", "PT_TRACET_WAVES", "PtPass P", "pt::bin_trace_body<pt::JitMap, false>(P)",
     0, "-DPT_TT_N=7"},
    {kJitTraceStats, "pt_bin_trace_jit_stats", "64", nullptr, "PtPass P", "pt::bin_trace_body<pt::JitMap, true>(P)",
     0, nullptr},
    // normal taps in the shade pass (PtPass.taps_in_shade): march-only trace (PT_TW_N), shade with JitMapB taps
    {kJitTraceM, "pt_bin_trace_m_jit", "64", "PT_TRACE_WAVES", "PtPass P",
     "pt::bin_trace_body<pt::JitMap, false, false>(P)", 0, "-DPT_TW_N=7"},
    {kJitTraceMStats, "pt_bin_trace_m_jit_stats", "64", nullptr, "PtPass P",
     "pt::bin_trace_body<pt::JitMap, true, false>(P)", 0, nullptr},
    // the first pass without a gen pass (PtPass gen_trace; PT_TG_N)
    {kJitTraceG, "pt_bin_trace_g_jit", "64", "PT_TRACEG_WAVES", "PtPass P",
     "pt::bin_trace_body<pt::JitMap, false, false, true, PT_CAMK_FIXED>(P)", 0, "-DPT_TG_N=7"},
    // (C3's shade kernel spills 8 bytes per lane at 8 waves and keeps them; PT_SW_N)
    {kJitShadeT, "pt_bin_shade_t_jit", "PT_BIN_BLOCK", "PT_SHADE_WAVES", "PtPass P",
     "pt::bin_shade_body<pt::JitTaps, false, false, PT_CAMK_FIXED>(P)", kShadeSpillOk, "-DPT_SW_N=7"},
    // the same two for a posed camera (pt_set_camera; pt_path.h PT_CAMK_*): the host launches
    // pt_bin_shade_tc_jit for shade pass 0 only, the one pass that makes camera rays again
    {kJitTraceGC, "pt_bin_trace_gc_jit", "64", "PT_POSED_WAVES", "PtPass P",
     "pt::bin_trace_body<pt::JitMap, false, false, true, PT_CAMK_POSED>(P)", 0, nullptr},
    {kJitShadeTC, "pt_bin_shade_tc_jit", "PT_BIN_BLOCK", "PT_POSED_WAVES", "PtPass P",
     "pt::bin_shade_body<pt::JitTaps, false, false, PT_CAMK_POSED>(P)", 0, nullptr},
    {kJitShadeTStats, "pt_bin_shade_t_jit_stats", "PT_BIN_BLOCK", nullptr, "PtPass P",
     "pt::bin_shade_body<pt::JitTaps, true, false>(P)", 0, nullptr},
    // camera rays with the scene's bounds() (straight-line slab tests)
    {kJitGen, "pt_bin_gen_jit", "PT_BIN_BLOCK", nullptr, "PtPass P",
     "pt::bin_gen_body<pt::JitTaps, false, PT_CAMK_FIXED>(P)", 0, nullptr},
    {kJitGenC, "pt_bin_gen_c_jit", "PT_BIN_BLOCK", nullptr, "PtPass P",
     "pt::bin_gen_body<pt::JitTaps, false, PT_CAMK_POSED>(P)", 0, nullptr},
    {kJitGenStats, "pt_bin_gen_jit_stats", "PT_BIN_BLOCK", nullptr, "PtPass P",
     "pt::bin_gen_body<pt::JitTaps, true>(P)", 0, nullptr},
};
static_assert(sizeof kJitKernels / sizeof kJitKernels[0] == kJitFnCount, "one kernel per PtJitFn");
constexpr bool pt_jit_kernels_cover_every_fn() {
    for (int f = 0; f < kJitFnCount; ++f) {
        int n = 0;
        for (const PtJitKernel &k : kJitKernels) n += k.fn == f;
        if (n != 1) return false;
    }
    return true;
}
static_assert(pt_jit_kernels_cover_every_fn(), "each PtJitFn names exactly one kernel");
struct PtJitModule {
    hipModule_t module = nullptr;
    hipFunction_t fn[kJitFnCount] = {};
    std::string key;  // generated source
};
// The scene kernel of one stage of a dispatch.  stats: the instrumented run;
// posed: a pt_set_camera view; taps_shade: normal taps in the shade pass;
// gen_norec: the first pass stored no ray records.  nullptr: the stage has no
// scene kernel in this configuration (the ahead-of-time one runs).
enum class PtJitStage { Render, Gen, Trace, TraceFirst, Shade };
hipFunction_t pt_jit_select(const PtJitModule &m, PtJitStage stage, bool stats, bool posed, bool taps_shade,
                            bool gen_norec);

// Source of the specialised kernel for these derived nodes.  bake=false:
// only the topology, per-node flags and material indices enter (values stay
// in the node table, value-only edits do not recompile); bake=true: node
// values become exact f32 literals too (no scalar loads; recompiles, cached,
// when a value changes).
std::string pt_jit_source(const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes, bool fast_bounds,
                          bool bake);
// (program, data) -> the derived tables and the source generated for them (pt_jit_compile, pt_scene_kernel_source);
// pt_derive's return code, `src` set on PT_OK
struct PtDerived {
    std::vector<PtNode> nodes;
    std::vector<PtAabb> boxes;
    std::vector<PtMat> mats;
};
int pt_derive_source(const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb, const float *data,
                     uint32_t n_data, bool bake, PtDerived &t, std::string &src, std::string &err);
// Compile with hipRTC for gfx950; returns the code object or an error log.
// on-disk cache first (*from_disk: the code object came from lib/jitcache)
bool pt_jit_compile_source(const std::string &src, std::vector<char> &code, std::string &log, bool *from_disk = nullptr);
// Load a code object on the current device.
bool pt_jit_load(const std::vector<char> &code, PtJitModule &m, std::string &err);
void pt_jit_unload(PtJitModule &m);

// The probe module (pt_probe_map / pt_probe_taps / pt_probe_bounds, pt_map_probe.hip): the
// scene's generated map() variants and bounds() under the probe kernels of pt_map_probe.h.  Each kernel has two
// builds, `name` and the instrumented `name`_stats: `extern "C" __global__ __launch_bounds__(64) void name(PtProbe P) { pt::body, ST>(P); }`
enum PtProbeFn { kProbeMap, kProbeMapB0, kProbeMapB1, kProbeTaps, kProbeBounds, kProbeFnCount };
struct PtProbeKernel {
    PtProbeFn fn;
    const char *name, *body;
};
inline constexpr PtProbeKernel kProbeKernels[] = {
    {kProbeMap, "pt_probe_map_jit", "probe_map_body<pt::JitMap"},
    {kProbeMapB0, "pt_probe_map_b0_jit", "probe_map_body<pt::JitMapB0"},
    {kProbeMapB1, "pt_probe_map_b1_jit", "probe_map_body<pt::JitMapB1"},
    {kProbeTaps, "pt_probe_taps_jit", "probe_taps_body<pt::JitTaps"},
    {kProbeBounds, "pt_probe_bounds_jit", "probe_bounds_body<pt::JitTaps"},
};
static_assert(sizeof kProbeKernels / sizeof kProbeKernels[0] == kProbeFnCount, "one kernel per PtProbeFn");
struct PtProbeModule {  // one kernel of one source
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
};
// pt_jit_source's text up to and including the wave macros, then probe kernel `fn` (instrumented with `stats`),
// or every probe kernel in both builds (fn < 0)
std::string pt_probe_source(const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes, bool fast_bounds,
                            bool bake, int fn = -1, bool stats = false);
// One hipRTC compile with the scene kernels' options; no rebuild rule, no on-disk cache.
bool pt_probe_compile(const std::string &src, std::vector<char> &code, std::string &log);

// A context's scene kernels and their lifecycle (pt_jit_state.cpp).  A code object
// and where it came from: compiled by this process's hipRTC, or read from the
// shipped on-disk cache (lib/jitcache)
enum PtJitFrom { kJitCompiled = 0, kJitDisk = 1 };
struct PtJitBuild {
    std::vector<char> code;  // empty: the compile failed (log set)
    double seconds = 0.0;
    int from = kJitCompiled;
};
struct PtJitState {
    int enabled = 1;  // pt_set_option "jit": 1 use per-scene hipRTC kernels, 0 interpreter
    int bake = 2;     // "jit_bake": 0 values from the node table, 1 baked as literals, 2 tier-up
    PtJitModule mod;  // scene kernel for the topology (key = its source)
    // tier-up (bake 2): the same kernel with the current values baked in as
    // literals, compiled on a worker thread and used once ready while the
    // values stay unchanged -- value edits never wait for a compile
    PtJitModule tier;
    std::string tier_want;  // baked source for the current values
    std::string tier_job_src;
    std::string tier_failed;  // a baked source that did not build (not retried)
    // code object (empty: compile failed) and its compile seconds; the worker
    // returns both through the future, so no field is shared with it
    std::future<PtJitBuild> tier_job;
    double seconds = 0.0, tier_seconds = 0.0;
    int from = -1, tier_from = -1;  // where the loaded builds came from (PtJitFrom)
    std::string log;
};
// (Re)build the scene kernel when the generated source changed.  A failure
// leaves the interpreter kernel in use and records the log.
void pt_jit_refresh(PtJitState &j, const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes,
                    bool fast_bounds);
// Install a finished tier-up compile if it is still the one the current
// values want; start the wanted one if nothing is pending.  wait: block on a
// pending compile first.
void pt_jit_poll(PtJitState &j, bool wait);
// The scene kernel in use: the tier-up build when loaded, else the topology one.
const PtJitModule *pt_jit_active(const PtJitState &j);
void pt_jit_disable(PtJitState &j);  // unload both builds and want no tier-up (until the next pt_jit_refresh)
void pt_jit_destroy(PtJitState &j);  // wait for a pending compile, then unload
