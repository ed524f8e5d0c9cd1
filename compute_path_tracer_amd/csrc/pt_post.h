// pt_post.h -- launch parameters of the image-space kernels (pt_post.hip):
// the display pass, the variance planes, the edge-stopping filters
//  and temporal accumulation (3.30).  One thread per
// pixel, no map(): none of them reads the scene.  Shared with the host entry
// points in pt_post_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.h"

void pt_launch_display(const float *img, uint32_t w, uint32_t h, int fmt, void *out, hipStream_t stream);

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
// one iteration of the variance-guided filter (pt_denoise_guided, pt_denoise_history): PtAtrous's taps with a
// per-pixel colour constant from the 3x3-smoothed variance plane, which is filtered beside the colour (vin -> vout)
struct PtGuided {
    const float4 *in, *g0, *g1;
    const float *vin;
    float4 *out;
    float *vout;
    int32_t w, h;
    int32_t iter;   // taps at step 1 << iter
    int32_t npow;   // normal_power_log2
    float ka;
    float sv2;      // sigma_variance squared
    float kz[PT_DENOISE_MAX_ITERATIONS];
};
// (two blocks, not one: each kernel's argument block, and with it its scalar loads, stays as it was)
void pt_launch_filter(const PtAtrous &A, bool lds, hipStream_t stream);  // lds: staged taps at steps 1 and 2
void pt_launch_filter(const PtGuided &A, bool lds, hipStream_t stream);

// v[i] = ((vr + vg) + vb), v.k = max(m.k - a.k * a.k, 0) / nm1, over n texels of the images a and m.  counts
// nullptr: nm1 for every texel (pt_read_variance, pt_denoise_guided); else counts[i] - 1 (pt_denoise_history)
void pt_launch_variance(const float *a, const float *m, const float *counts, float nm1, float *v, uint32_t n,
                        hipStream_t stream);

// temporal accumulation (pt_temporal_accumulate): the current view -- image, moments, guides, of
// n_cur frames, under (cam_mode, cam, aspect, fov) -- merged with the history of the previous view (p*: its colour,
// moments, count and guide planes, its camera, and that camera's origin and reciprocal basis) into the new history
// (o*).  have 0: nothing is taken and no p* pointer is read (no history yet, or a degenerate previous basis)
struct PtTemporal {
    const float4 *a, *m, *g0, *g1;
    const float4 *ph, *phm, *pg0, *pg1;
    const float *phn;
    float4 *oh, *ohm;
    float *ohn;
    int32_t w, h;
    int32_t have;
    int32_t cam_mode, pcam_mode;  // PT_CAM_DEFAULT or PT_CAM_PINHOLE (a lens as its pinhole)
    float n_cur;
    float aspect, fov, paspect, pfov;
    float max_history, depth_tolerance, normal_cos, at2;  // at2 = albedo_tolerance squared
    float po[3], ir[3], iu[3], ifw[3];
    pt_camera cam, pcam;
};
void pt_launch_temporal(const PtTemporal &T, hipStream_t stream);
