// pt_host.h -- host-side internals shared by pt_runtime.hip and pt_jit.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "pt_binned.h"
#include "pt_device.h"

// ahead-of-time kernels (pt_kernel.hip)
bool pt_use_simple_kernel(const PtLaunch &L);
void pt_launch_render(const PtLaunch &L, bool stats, hipStream_t stream);
enum class PtBinStage { Gen, Shade, Scan, Scatter, Trace, Fold };
void pt_launch_bin(PtBinStage stage, const PtPass &P, bool stats, unsigned grid, hipStream_t stream);
int pt_bin_trace_blocks_per_cu(bool stats);  // occupancy of the interpreter trace kernel
// the sky pass after a binned trace pass (pt_set_sky): P as that trace pass's shade pass takes it; quads: the
// trace pass wrote hit quads (taps in the shade pass), not hit records
void pt_launch_bin_sky(const PtPass &P, bool quads, unsigned grid, hipStream_t stream);
void pt_launch_display(const float *img, uint32_t w, uint32_t h, int fmt, void *out, hipStream_t stream);
// the denoiser's guide images (pt_render_guides): L as a dispatch takes it, over every tile, a lens as its pinhole
void pt_launch_guides(const PtLaunch &L, float *g0, float *g1, hipStream_t stream);
// one iteration of the a-trous filter (pt_denoise): every iteration's constants travel in the launch arguments
#define PT_ATROUS_BX 64            // direct form: block 64 x 4, a wave = one row segment
#define PT_ATROUS_BY 4
#define PT_ATROUS_T 16             // LDS form: 16 x 16 tile + halo
#define PT_ATROUS_LDS_MAX_STEP 2   // ... for steps 1 and 2
struct PtAtrous {
    const float4 *in, *g0, *g1;
    float4 *out;
    int32_t w, h;
    int32_t iter;   // taps at step 1 << iter
    int32_t npow;   // normal_power_log2
    float ka;
    float kc[PT_DENOISE_MAX_ITERATIONS], kz[PT_DENOISE_MAX_ITERATIONS];
};
void pt_launch_atrous(const PtAtrous &A, bool lds, hipStream_t stream);

// Expand (program, data[]) into the device tables (see pt_device.h).
int pt_derive(const std::vector<pt_op> &ops, const std::vector<pt_aabb> &aabbs, const float *data, uint32_t n,
              std::vector<PtNode> &nodes, std::vector<PtAabb> &boxes, std::vector<PtMat> &mats, std::string &err);

// Margin constant of the map() bound; NaN: no bound.
float pt_bound_k(const std::vector<PtNode> &nodes);

// Scene-specialised kernels (hipRTC).
struct PtJitModule {
    hipModule_t module = nullptr;
    hipFunction_t render = nullptr;
    hipFunction_t render_stats = nullptr;
    hipFunction_t trace = nullptr;        // binned pipeline trace pass (pt_binned.h)
    hipFunction_t trace_stats = nullptr;
    hipFunction_t trace_m = nullptr;        // march-only trace pass (normal taps in the shade pass)
    hipFunction_t trace_m_stats = nullptr;
    hipFunction_t shade_t = nullptr;        // shade pass with the normal taps (JitMapB)
    hipFunction_t shade_t_stats = nullptr;
    hipFunction_t gen = nullptr;  // camera rays + the scene's straight-line bounds()
    hipFunction_t gen_stats = nullptr;
    hipFunction_t trace_g = nullptr;  // first pass with its own camera rays (PtPass gen_trace)
    // the kernels that make camera rays, built for a posed camera (pt_set_camera; pt_path.h PT_CAMK_POSED):
    // gen pass, first pass, shade pass 0 -- the ones above serve the fixed camera only
    hipFunction_t gen_c = nullptr, trace_gc = nullptr, shade_tc = nullptr;
    std::string key;  // generated source
};

// Source of the specialised kernel for these derived nodes.  bake=false:
// only the topology, per-node flags and material indices enter (values stay
// in the node table, value-only edits do not recompile); bake=true: node
// values become exact f32 literals too (no scalar loads; recompiles, cached,
// when a value changes).
std::string pt_jit_source(const std::vector<PtNode> &nodes, const std::vector<PtAabb> &boxes, bool fast_bounds,
                          bool bake);
// Compile with hipRTC for gfx950; returns the code object or an error log.
// on-disk cache first (*from_disk: the code object came from lib/jitcache)
bool pt_jit_compile_source(const std::string &src, std::vector<char> &code, std::string &log, bool *from_disk = nullptr);
// Load a code object on the current device.
bool pt_jit_load(const std::vector<char> &code, PtJitModule &m, std::string &err);
void pt_jit_unload(PtJitModule &m);
