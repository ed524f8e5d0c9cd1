// pt_pixel.h -- what the scene-side per-pixel kernels (pt_kernel.hip: guides,
// picks) and the image-space kernels (pt_post.hip: temporal accumulation, the
// filters) both state: a pixel's jitter-free primary ray and the finite tests;
// and what the simple kernel (pt_kernel.hip) and the binned fold
// (pt_bin_kernels.hip) both state: a frame's second moments.
// Ahead-of-time only: no hipRTC scene source includes it, so it is not among
// the embedded headers (build.py EMBED) and no scene kernel's cache key sees it.
#pragma once

#include "pt_path.h"

__device__ __forceinline__ bool pt_finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// pt_finite_f of r, g and b, spelled out: as three calls the compiler turns each test into a class compare, which
// is other (and faster) code in every kernel that filters or reprojects -- a change of its own (EXPERIMENTS.md)
__device__ __forceinline__ bool pt_finite_rgb(const float4 &c) {
    return (__float_as_uint(c.x) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(c.y) & 0x7f800000u) != 0x7f800000u &&
           (__float_as_uint(c.z) & 0x7f800000u) != 0x7f800000u;
}

// Second moments (pt_set_option "moments"): a frame's squared
// colour into the moment texel, with mix_frame's own w and 1 - w; the moment
// texel is the accumulation texel's place in the moment image.
__device__ __forceinline__ void mix_moment(float &mr, float &mg, float &mb, const pt_f3 &c, int32_t last_clear) {
    pt::mix_frame(mr, mg, mb, pt_f3{c.x * c.x, c.y * c.y, c.z * c.z}, last_clear);
}
__device__ __forceinline__ float4 *moment_texel(const PtLaunch &L, float *moments, const float4 *texel) {
    return reinterpret_cast<float4 *>(moments) + (texel - reinterpret_cast<const float4 *>(L.accum));
}

// The jitter-free primary ray of pixel (x, y) under a camera: calc_uv without
// the jitter term, then the camera with a lens taken as its pinhole (no lens
// draw, so no rng).  Stated once for the guide images, the history's
// reprojection and the pixel picks: the same operations, so the same bits.
__device__ __forceinline__ void pixel_ray(int x, int y, int w, int h, float aspect, float fov, int cam_mode,
                                          const pt_camera &cam, pt_f3 &ro, pt_f3 &rd) {
    float ux = float(x) / float(w), uy = float(y) / float(h);
    ux = ux * 2.0f - 1.0f;
    uy = uy * 2.0f - 1.0f;
    ux *= aspect;
    uint32_t rng = 0u;  // (no lens, so no draw)
    pt::camera_from_uv(ux, uy, fov, cam_mode == PT_CAM_DEFAULT ? PT_CAM_DEFAULT : PT_CAM_PINHOLE, cam, rng, ro, rd);
}
