// pt_post_host.cpp -- the image-space entry points of the C ABI
// (include/pt_abi.h): pt_display, pt_read_variance, the three filters
// pt_denoise / pt_denoise_guided / pt_denoise_history (DESIGN.md 3.26, 3.28,
// 3.30) and temporal accumulation (pt_temporal_*, pt_read_history, 3.30).
// Host only; the kernels are in pt_post.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "pt_ctx.h"
#include "pt_post.h"

static_assert(sizeof(pt_denoise_params) == 5 * 4, "pt_denoise_params layout");
static_assert(sizeof(pt_guided_params) == 5 * 4, "pt_guided_params layout");
static_assert(sizeof(pt_temporal_params) == 4 * 4, "pt_temporal_params layout");

// ---- variance --------------------------------------------
// Where a variance plane comes from: an image and its moment image, of `frames` frames throughout or, with
// `counts`, of counts[i] frames at texel i; and the section that times its kernel.
struct VarianceOf {
    const DevBuf &image, &moments;
    const DevBuf *counts;
    uint32_t frames;
    TimedSection &time;
};
static VarianceOf accum_variance(pt_ctx *c) { return {c->img.accum, c->mom.img, nullptr, c->mom.frames, c->mom.variance_time}; }

// the variance plane into mom.var[0] (asynchronous, timed)
static int launch_variance(pt_ctx *c, const VarianceOf &v) {
    const size_t texels = size_t(c->img.width) * c->img.height;
    int rc;
    for (DevBuf &b : c->mom.var)
        if ((rc = ensure(c, b, std::max<size_t>(texels * sizeof(float), 16))) != PT_OK) return rc;
    HIPCHK(c, v.time.begin(c->stream));
    pt_launch_variance(v.image.as<float>(), v.moments.as<float>(), v.counts ? v.counts->as<float>() : nullptr,
                       float(v.frames - 1u), c->mom.var[0].as<float>(), uint32_t(texels), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, v.time.end(c->stream));
    return PT_OK;
}

static const char *const kNoGuides = "guides stale: call pt_render_guides";
static const char *const kNoVariance = "no variance: valid moments of at least 2 frames are needed";
static const char *const kNoHistory = "no history: call pt_temporal_accumulate";

// ---- the filters -------------------------------------
// One setup and one driver under pt_denoise (A = PtAtrous, P = pt_denoise_params) and pt_denoise_guided /
// pt_denoise_history (A = PtGuided, P = pt_guided_params).
template <class A>
constexpr bool kGuided = std::is_same<A, PtGuided>::value;

// 1 / (sigma * scale)^2 in f32: the scaled sigma, its square, one division of 1 (a term that is off: 0)
static float inv_sq(float sigma, float scale) {
    if (sigma == 0.0f) return 0.0f;
    const float v = sigma * scale;
    const float sq = v * v;
    return 1.0f / sq;
}

// The refusals every filter shares, in their order -- null parameters, format, iterations, normal power, sigmas,
// sigma_variance (guided), a constant that is not finite -- and the iterations' constants into K, zeroed first.
template <class A, class P>
static int filter_setup(pt_ctx *c, const P *p, int format, A &K) {
    if (!p) return fail(c, PT_ERR_INVALID, "null denoise parameters");
    if (format != PT_DISPLAY_RGBA32F && format != PT_DISPLAY_SRGB8 && format != PT_DENOISE_LINEAR)
        return fail(c, PT_ERR_INVALID, "bad denoise format");
    if (p->iterations < 1 || p->iterations > PT_DENOISE_MAX_ITERATIONS)
        return fail(c, PT_ERR_INVALID, "denoise iterations must be in [1, 8]");
    if (p->normal_power_log2 > 8) return fail(c, PT_ERR_INVALID, "denoise normal_power_log2 must be in [0, 8]");
    float sigma_color = 0.0f;
    if constexpr (!kGuided<A>) sigma_color = p->sigma_color;
    for (float v : {sigma_color, p->sigma_depth, p->sigma_albedo})
        if (!std::isfinite(v) || v < 0.0f) return fail(c, PT_ERR_INVALID, "denoise sigma must be finite and >= 0");
    std::memset(&K, 0, sizeof K);
    if constexpr (kGuided<A>) {
        if (!std::isfinite(p->sigma_variance) || !(p->sigma_variance > 0.0f))
            return fail(c, PT_ERR_INVALID, "denoise sigma_variance must be finite and > 0");
        K.sv2 = p->sigma_variance * p->sigma_variance;
    }
    K.npow = int32_t(p->normal_power_log2);
    K.ka = inv_sq(p->sigma_albedo, 1.0f);
    bool finite = std::isfinite(K.ka);
    for (uint32_t i = 0; i < p->iterations; ++i) {
        if constexpr (!kGuided<A>) {
            K.kc[i] = inv_sq(sigma_color, std::ldexp(1.0f, -int(i)));
            finite = finite && std::isfinite(K.kc[i]);
        }
        K.kz[i] = inv_sq(p->sigma_depth, std::ldexp(1.0f, int(i)));
        finite = finite && std::isfinite(K.kz[i]);
    }
    if (!finite) return fail(c, PT_ERR_INVALID, "denoise sigma too small: 1 / sigma^2 is not finite");
    return PT_OK;
}

// The filter itself, after the caller's state refusals: the output-size refusal, the buffers, the variance plane
// (guided: `var`, into var[0]), then colour -> filter[0] -> filter[1] -> filter[0] ... under the guide planes
// g0 / g1 (guided: with the variance var[0] -> var[1] -> var[0] ... beside it), timed by `time`; the result
// through the display pass unless `format` is linear, and back to the host.  The colour image is only read.
template <class A>
static int run_filter(pt_ctx *c, A &K, uint32_t iterations, const DevBuf &colour, const DevBuf &g0, const DevBuf &g1,
                      const VarianceOf *var, TimedSection &time, int format, void *out, size_t bytes) {
    const size_t texels = size_t(c->img.width) * c->img.height;
    const size_t need = texels * (format == PT_DISPLAY_SRGB8 ? 4 : 16);
    if (!out || bytes < need) return fail(c, PT_ERR_SIZE, "denoise output buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    for (DevBuf &f : c->dn.filter)
        if ((rc = ensure(c, f, std::max<size_t>(texels * 16, 16))) != PT_OK) return rc;
    if (format != PT_DENOISE_LINEAR && (rc = ensure(c, c->img.display, std::max<size_t>(need, 16))) != PT_OK) return rc;
    if (var && (rc = launch_variance(c, *var)) != PT_OK) return rc;
    K.g0 = g0.as<const float4>();
    K.g1 = g1.as<const float4>();
    K.w = int32_t(c->img.width);
    K.h = int32_t(c->img.height);
    const float *src = colour.as<float>();
    HIPCHK(c, time.begin(c->stream));
    for (uint32_t i = 0; i < iterations; ++i) {
        K.in = reinterpret_cast<const float4 *>(src);
        K.out = c->dn.filter[i & 1].as<float4>();
        if constexpr (kGuided<A>) {
            K.vin = c->mom.var[i & 1].as<const float>();
            K.vout = c->mom.var[(i + 1) & 1].as<float>();
        }
        K.iter = int32_t(i);
        pt_launch_filter(K, c->dn.lds != 0, c->stream);
        HIPCHK(c, hipGetLastError());
        src = c->dn.filter[i & 1].as<float>();
    }
    HIPCHK(c, time.end(c->stream));
    const void *result = src;
    if (format != PT_DENOISE_LINEAR) {
        pt_launch_display(src, c->img.width, c->img.height, format, c->img.display.p, c->stream);
        HIPCHK(c, hipGetLastError());
        result = c->img.display.p;
    }
    return read_back(c, out, bytes, result, need, nullptr);
}

// ---- temporal accumulation ---------------------------------------
// The reciprocal basis of (right, up, forward): cross products over the determinant, in double, each component
// rounded once to f32.  false: the determinant is zero or not finite (nothing can be projected).
static bool reciprocal_basis(const pt_camera &cam, float ir[3], float iu[3], float ifw[3]) {
    const double r[3] = {cam.right[0], cam.right[1], cam.right[2]}, u[3] = {cam.up[0], cam.up[1], cam.up[2]},
                 f[3] = {cam.forward[0], cam.forward[1], cam.forward[2]};
    auto cross = [](const double a[3], const double b[3], double o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1];
        o[1] = a[2] * b[0] - a[0] * b[2];
        o[2] = a[0] * b[1] - a[1] * b[0];
    };
    double uf[3], fr[3], ru[3];
    cross(u, f, uf);
    cross(f, r, fr);
    cross(r, u, ru);
    const double det = (r[0] * uf[0] + r[1] * uf[1]) + r[2] * uf[2];
    if (!std::isfinite(det) || det == 0.0) return false;
    for (int k = 0; k < 3; ++k) {
        ir[k] = float(uf[k] / det);
        iu[k] = float(fr[k] / det);
        ifw[k] = float(ru[k] / det);
    }
    return true;
}

extern "C" {

int pt_display(pt_ctx *c, int format, void *out, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    if (format != PT_DISPLAY_RGBA32F && format != PT_DISPLAY_SRGB8) return fail(c, PT_ERR_INVALID, "bad display format");
    const size_t need = c->img.bytes(format == PT_DISPLAY_RGBA32F ? 16 : 4);
    if (!out || bytes < need) return fail(c, PT_ERR_SIZE, "display buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure(c, c->img.display, std::max<size_t>(need, 16));
    if (rc != PT_OK) return rc;
    HIPCHK(c, c->img.display_time.begin(c->stream));
    pt_launch_display(c->img.accum.as<float>(), c->img.width, c->img.height, format, c->img.display.p, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->img.display_time.end(c->stream));
    return read_back(c, out, bytes, c->img.display.p, need, nullptr);
}

int pt_read_variance(pt_ctx *c, float *v, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    if (!c->mom.valid || c->mom.frames < 2) return fail(c, PT_ERR_STATE, kNoVariance);
    const size_t need = c->img.bytes(sizeof(float));
    if (!v || bytes < need) return fail(c, PT_ERR_SIZE, "variance buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = launch_variance(c, accum_variance(c));
    if (rc != PT_OK) return rc;
    return read_back(c, v, bytes, c->mom.var[0].p, need, nullptr);
}

int pt_denoise(pt_ctx *c, const pt_denoise_params *p, int format, void *out, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    PtAtrous K;
    const int rc = filter_setup(c, p, format, K);
    if (rc != PT_OK) return rc;
    if (!c->dn.guides_valid) return fail(c, PT_ERR_STATE, kNoGuides);
    return run_filter(c, K, p->iterations, c->img.accum, c->dn.guides[0], c->dn.guides[1], nullptr, c->dn.denoise_time,
                      format, out, bytes);
}

// The variance-guided form of pt_denoise: the colour constant per pixel from the variance plane
// of the accumulation image and its moments, which the iterations filter beside the colour.
int pt_denoise_guided(pt_ctx *c, const pt_guided_params *p, int format, void *out, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    PtGuided K;
    const int rc = filter_setup(c, p, format, K);
    if (rc != PT_OK) return rc;
    if (!c->dn.guides_valid) return fail(c, PT_ERR_STATE, kNoGuides);
    if (!c->mom.valid || c->mom.frames < 2) return fail(c, PT_ERR_STATE, kNoVariance);
    const VarianceOf var = accum_variance(c);
    return run_filter(c, K, p->iterations, c->img.accum, c->dn.guides[0], c->dn.guides[1], &var, c->mom.guided_time,
                      format, out, bytes);
}

// pt_denoise_guided over the history: the history's colour, its own copy of the guides, and the
// variance of its moments under its per-pixel count, for the accumulation image, the live guides and n.
int pt_denoise_history(pt_ctx *c, const pt_guided_params *p, int format, void *out, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    PtGuided K;
    const int rc = filter_setup(c, p, format, K);
    if (rc != PT_OK) return rc;
    pt_ctx::History &hs = c->hist;
    if (!hs.valid) return fail(c, PT_ERR_STATE, kNoHistory);
    const pt_ctx::History::Set &s = hs.set[hs.cur];
    const VarianceOf var = {s.h, s.hm, &s.hn, 0, hs.variance_time};
    return run_filter(c, K, p->iterations, s.h, s.g0, s.g1, &var, hs.denoise_time, format, out, bytes);
}

int pt_temporal_accumulate(pt_ctx *c, const pt_temporal_params *p) {
    if (!c) return PT_ERR_INVALID;
    if (!p) return fail(c, PT_ERR_INVALID, "null temporal parameters");
    for (float v : {p->max_history, p->depth_tolerance, p->albedo_tolerance})
        if (!std::isfinite(v) || v < 0.0f) return fail(c, PT_ERR_INVALID, "temporal max_history and tolerances must be finite and >= 0");
    if (!(p->normal_cos >= -1.0f && p->normal_cos <= 1.0f)) return fail(c, PT_ERR_INVALID, "temporal normal_cos must lie in [-1, 1]");
    if (c->view.nranks != 1)
        return fail(c, PT_ERR_UNSUPPORTED, "the history is of the whole image: pt_set_tiles(0, 1), then write the reduced image and moments");
    if (!c->dn.guides_valid) return fail(c, PT_ERR_STATE, kNoGuides);
    if (!c->mom.valid || c->mom.frames < 2) return fail(c, PT_ERR_STATE, kNoVariance);
    HIPCHK(c, hipSetDevice(c->device));
    pt_ctx::History &hs = c->hist;
    const size_t texels = size_t(c->img.width) * c->img.height;
    const size_t rgba = std::max<size_t>(texels * 16, 16), plane = std::max<size_t>(texels * sizeof(float), 16);
    int rc;
    for (pt_ctx::History::Set &s : hs.set) {
        for (DevBuf *b : {&s.h, &s.hm, &s.g0, &s.g1})
            if ((rc = ensure(c, *b, rgba)) != PT_OK) return rc;
        if ((rc = ensure(c, s.hn, plane)) != PT_OK) return rc;
    }
    const pt_ctx::History::Set &prev = hs.set[hs.cur], &next = hs.set[hs.cur ^ 1];
    PtTemporal T;
    std::memset(&T, 0, sizeof T);
    T.a = c->img.accum.as<const float4>();
    T.m = c->mom.img.as<const float4>();
    T.g0 = c->dn.guides[0].as<const float4>();
    T.g1 = c->dn.guides[1].as<const float4>();
    T.ph = prev.h.as<const float4>();
    T.phm = prev.hm.as<const float4>();
    T.phn = prev.hn.as<const float>();
    T.pg0 = prev.g0.as<const float4>();
    T.pg1 = prev.g1.as<const float4>();
    T.oh = next.h.as<float4>();
    T.ohm = next.hm.as<float4>();
    T.ohn = next.hn.as<float>();
    T.w = int32_t(c->img.width);
    T.h = int32_t(c->img.height);
    T.n_cur = float(c->mom.frames);
    T.cam_mode = c->dn.guide_cam_mode;
    T.cam = c->dn.guide_cam;
    T.aspect = c->dn.guide_aspect;
    T.fov = c->dn.guide_fov;
    T.pcam_mode = hs.cam_mode;
    T.pcam = hs.cam;
    T.paspect = hs.aspect;
    T.pfov = hs.fov;
    T.max_history = p->max_history;
    T.depth_tolerance = p->depth_tolerance;
    T.normal_cos = p->normal_cos;
    T.at2 = p->albedo_tolerance * p->albedo_tolerance;
    for (int k = 0; k < 3; ++k) T.po[k] = hs.cam.origin[k];
    // (a degenerate previous basis: nothing is taken, the history starts again from the current view)
    T.have = hs.valid && reciprocal_basis(hs.cam, T.ir, T.iu, T.ifw) ? 1 : 0;
    HIPCHK(c, hs.accumulate_time.begin(c->stream));
    pt_launch_temporal(T, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hs.accumulate_time.end(c->stream));
    // the new history's guides are the current view's
    if (texels) {
        HIPCHK(c, hipMemcpyAsync(next.g0.p, c->dn.guides[0].p, texels * 16, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(next.g1.p, c->dn.guides[1].p, texels * 16, hipMemcpyDeviceToDevice, c->stream));
    }
    hs.cur ^= 1;
    hs.cam_mode = T.cam_mode;
    hs.cam = T.cam;
    hs.aspect = T.aspect;
    hs.fov = T.fov;
    hs.valid = true;
    hs.views += 1;
    return PT_OK;
}

int pt_temporal_reset(pt_ctx *c) {
    if (!c) return PT_ERR_INVALID;
    c->hist.drop();
    return PT_OK;
}

int pt_read_history(pt_ctx *c, float *colour, float *moments, float *count, size_t bytes_rgba) {
    if (!c) return PT_ERR_INVALID;
    if (!c->hist.valid) return fail(c, PT_ERR_STATE, kNoHistory);
    const size_t need = c->img.bytes();
    if (bytes_rgba < need) return fail(c, PT_ERR_SIZE, "history buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    const pt_ctx::History::Set &s = c->hist.set[c->hist.cur];
    // (any of the three may be left out; one wait for all)
    if (colour && need) HIPCHK(c, hipMemcpyAsync(colour, s.h.p, need, hipMemcpyDeviceToHost, c->stream));
    if (moments && need) HIPCHK(c, hipMemcpyAsync(moments, s.hm.p, need, hipMemcpyDeviceToHost, c->stream));
    return read_back(c, count, need / 4, s.hn.p, count ? need / 4 : 0, nullptr);
}

}  // extern "C"
