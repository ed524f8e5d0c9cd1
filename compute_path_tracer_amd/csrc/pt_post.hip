// pt_post.hip -- the image-space kernels for CDNA4 (gfx950): what runs on the
// accumulation image and its companions after the render, one thread per
// pixel, none of it through map().  Beside the scene kernels of pt_kernel.hip;
// host entry points in pt_post_host.cpp.
//
//   pt_display_kernel                     the display pass (pt_display)
//   pt_variance_kernel, pt_history_variance_kernel
//                                         the variance plane of an image and its
//                                         moments
//   pt_atrous_*, pt_guided_*              one iteration of the edge-stopping
//                                         filter, fixed or variance-guided, in a
//                                         direct and an LDS-staged form (3.26, 3.28)
//   pt_temporal_kernel                    temporal accumulation (3.30)
#include <type_traits>

#include "pt_pixel.h"
#include "pt_post.h"

using namespace pt;

// ---- display pass (render_texture_shader.wgsl) ------------------------------
// PT_DISPLAY_RGBA32F: fs_main's output per texel (row 0 = bottom, as stored).
// PT_DISPLAY_SRGB8: what the sRGB swapchain holds, in screen order (row 0 =
// top; screen row j shows texel row H-1-j at window size = image size).
// HBM-bound: 16 B read + 16 or 4 B written per pixel, one thread per pixel.
__global__ __launch_bounds__(256) void pt_display_kernel(const float4 *__restrict__ img, uint32_t w, uint32_t h,
                                                         int fmt, void *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    if (fmt == PT_DISPLAY_RGBA32F) {
        const float4 v = img[i];
        reinterpret_cast<float4 *>(out)[i] =
            make_float4(pt_display_channel(v.x), pt_display_channel(v.y), pt_display_channel(v.z), 1.0f);
    } else {
        const uint32_t row = i / w, x = i - row * w;
        const float4 v = img[size_t(h - 1 - row) * w + x];
        const uint32_t r = pt_srgb8(pt_display_channel(v.x)), g = pt_srgb8(pt_display_channel(v.y)),
                       b = pt_srgb8(pt_display_channel(v.z));
        reinterpret_cast<uint32_t *>(out)[i] = r | (g << 8) | (b << 16) | (255u << 24);
    }
}

void pt_launch_display(const float *img, uint32_t w, uint32_t h, int fmt, void *out, hipStream_t stream) {
    const uint32_t n = w * h;
    if (n == 0) return;
    hipLaunchKernelGGL(pt_display_kernel, dim3((n + 255) / 256), dim3(256), 0, stream,
                       reinterpret_cast<const float4 *>(img), w, h, fmt, out);
}

// ---- variance -----------------------------------------
// Variance of the mean from an image a and its moment image m, one thread per
// pixel: v.k = max(m.k - a.k^2, 0) / nm1 (the max drops a NaN: 0), summed
// (r + g) + b.  nm1 is the frame count - 1 of the accumulation image, or the
// history's count of the pixel - 1.  HBM-bound: 32 or 36 B read, 4 B written.
__device__ __forceinline__ float variance_of_mean(const float4 &a, const float4 &m, float nm1) {
    const float vr = pt_gmax(m.x - a.x * a.x, 0.0f) / nm1;
    const float vg = pt_gmax(m.y - a.y * a.y, 0.0f) / nm1;
    const float vb = pt_gmax(m.z - a.z * a.z, 0.0f) / nm1;
    return (vr + vg) + vb;
}

__global__ __launch_bounds__(256) void pt_variance_kernel(const float4 *__restrict__ A, const float4 *__restrict__ M,
                                                          float *__restrict__ v, uint32_t n, float nm1) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    v[i] = variance_of_mean(A[i], M[i], nm1);
}

__global__ __launch_bounds__(256) void pt_history_variance_kernel(const float4 *__restrict__ H, const float4 *__restrict__ HM,
                                                                  const float *__restrict__ HN, float *__restrict__ v,
                                                                  uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    v[i] = variance_of_mean(H[i], HM[i], HN[i] - 1.0f);
}

void pt_launch_variance(const float *a, const float *m, const float *counts, float nm1, float *v, uint32_t n,
                        hipStream_t stream) {
    if (n == 0) return;
    const float4 *a4 = reinterpret_cast<const float4 *>(a), *m4 = reinterpret_cast<const float4 *>(m);
    if (counts) hipLaunchKernelGGL(pt_history_variance_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a4, m4, counts, v, n);
    else hipLaunchKernelGGL(pt_variance_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a4, m4, v, n, nm1);
}

// ---- the edge-stopping filter --------------------------
// One iteration of the a-trous wavelet (Dammertz et al. 2010): 5x5 B3 taps at
// step 1 << iter.  Stated once for the fixed filter (PtAtrous: the colour
// constant kc[iter]) and the variance-guided one (PtGuided: a colour constant
// per pixel, and the variance plane filtered beside the colour), and once for
// the direct and the LDS-staged form: `tap` loads one texel's colour, guides
// and, for PtGuided, variance, so every form runs the same arithmetic.
// HBM/L2-bound: 25 taps of 48 (52) B per pixel against 64 (72) B of unique traffic.
template <class P>
constexpr bool kWithVariance = std::is_same<P, PtGuided>::value;

// The weight of tap (dx, dy), texel q against the centre p: the B3 factor
// divided by the rational colour, albedo and depth terms and multiplied by the
// clamped normal dot product squared npow times.  false: the tap is left out
// (a hit against a miss, or a weight that is not > 0).  Every operation is one
// f32 rounding in the order of DESIGN.md 3.26.
__device__ __forceinline__ bool tap_weight(int dx, int dy, const float4 &cp, const float4 &np, const float4 &ap,
                                           const float4 &cq, const float4 &nq, const float4 &aq, bool hit_p, float kc,
                                           float ka, float kz, int npow, float &w) {
    const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
    const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f);
    w = hy * hx;
    if (dx != 0 || dy != 0) {
        if (aq.w != ap.w) return false;  // hit and miss texels never mix
        const float ex = cq.x - cp.x, ey = cq.y - cp.y, ez = cq.z - cp.z;
        float den = 1.0f + ((ex * ex + ey * ey) + ez * ez) * kc;
        if (hit_p) {
            const float ax = aq.x - ap.x, ay = aq.y - ap.y, az = aq.z - ap.z;
            den = den * (1.0f + ((ax * ax + ay * ay) + az * az) * ka);
            const float dz = nq.w - np.w;
            den = den * (1.0f + (dz * dz) * kz);
            float nd = pt_gmax(pt_dot(pt_f3{np.x, np.y, np.z}, pt_f3{nq.x, nq.y, nq.z}), 0.0f);
            for (int k = 0; k < npow; ++k) nd = nd * nd;
            w = w * nd;
        }
        w = w / den;
        if (!(w > 0.0f)) return false;  // (false for NaN)
    }
    return true;
}

// The guided filter's colour constant of pixel (x, y): kc = 1 / (sv2 g + EPS),
// g the variance plane smoothed over the 3x3 neighbourhood (step 1, weights
// {1/2, 1/4} per axis, non-finite and outside taps left out; none left: g =
// +inf and the colour term is off).  `near` loads one neighbour's variance.
// One f32 rounding per operation, in the order of DESIGN.md 3.28.
template <class Near>
__device__ __forceinline__ float variance_kc(const PtGuided &A, int x, int y, const Near &near) {
    float sg3 = 0.0f, sw3 = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= A.w || qy >= A.h) continue;
            const float vq = near(dx, dy);
            if (!pt_finite_f(vq)) continue;
            const float w3 = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            sw3 = sw3 + w3;
            sg3 = sg3 + w3 * vq;
        }
    }
    const float g = sw3 > 0.0f ? sg3 / sw3 : __uint_as_float(0x7f800000u);
    return 1.0f / (A.sv2 * g + 1e-10f);
}

// One pixel of one iteration: its colour, and for PtGuided its variance in
// vout.  `tap(dx, dy, c, n, a, v)` loads the texel of 5x5 tap (dx, dy) in the
// form's own storage (v: PtGuided only), `near(dx, dy)` the variance of a 3x3
// neighbour (PtGuided only).  A tap's coordinates are tested against the image
// before it is loaded.  A centre that is not finite passes through.
template <class P, class Tap, class Near>
__device__ __forceinline__ float4 filter_pixel(const P &A, int x, int y, const Tap &tap, const Near &near, float &vout) {
    constexpr bool kVar = kWithVariance<P>;
    const int s = 1 << A.iter;
    const float kz = A.kz[A.iter], ka = A.ka;
    float kc;
    if constexpr (!kVar) kc = A.kc[A.iter];
    float4 cp, np, ap;
    tap(0, 0, cp, np, ap, vout);
    if (!pt_finite_rgb(cp)) return cp;
    if constexpr (kVar) kc = variance_kc(A, x, y, near);
    const bool hit_p = ap.w != 0.0f;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + s * dx, qy = y + s * dy;
            if (qx < 0 || qy < 0 || qx >= A.w || qy >= A.h) continue;
            float4 cq, nq, aq;
            float vq, w;
            tap(dx, dy, cq, nq, aq, vq);
            if (!pt_finite_rgb(cq)) continue;
            if (!tap_weight(dx, dy, cp, np, ap, cq, nq, aq, hit_p, kc, ka, kz, A.npow, w)) continue;
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            if constexpr (kVar) sv = sv + (w * w) * vq;
        }
    }
    if constexpr (kVar) vout = sv / (sw * sw);
    return make_float4(sr / sw, sg / sw, sb / sw, cp.w);
}

// pixel p of the iteration's output
template <class P>
__device__ __forceinline__ void filter_store(const P &A, size_t p, const float4 &c, float v) {
    A.out[p] = c;
    if constexpr (kWithVariance<P>) A.vout[p] = v;
}

// Direct form: one thread per pixel, blocks 64 wide in x, so a wave's tap row
// is one contiguous run of 16 B texels at every step; the centre's colour and
// guides stay in registers.
template <class P>
__device__ __forceinline__ void filter_direct(const P &A) {
    const int x = int(blockIdx.x) * PT_ATROUS_BX + int(threadIdx.x), y = int(blockIdx.y) * PT_ATROUS_BY + int(threadIdx.y);
    if (x >= A.w || y >= A.h) return;
    const size_t p = size_t(y) * size_t(A.w) + size_t(x);
    const int s = 1 << A.iter;
    auto at = [&](int ox, int oy) { return size_t(ptrdiff_t(p) + ptrdiff_t(oy) * ptrdiff_t(A.w) + ptrdiff_t(ox)); };
    auto tap = [&](int dx, int dy, float4 &c, float4 &n, float4 &a, float &v) {
        // (in range: filter_pixel tests the tap's coordinates first)
        const size_t q = at(s * dx, s * dy);
        c = A.in[q];
        n = A.g0[q];
        a = A.g1[q];
        if constexpr (kWithVariance<P>) v = A.vin[q];
    };
    auto near = [&](int dx, int dy) {
        if constexpr (kWithVariance<P>) return A.vin[at(dx, dy)];
    };
    float v;
    const float4 c = filter_pixel(A, x, y, tap, near, v);
    filter_store(A, p, c, v);
}

// LDS form for the steps whose halo is small (1 and 2): a 16x16 block stages
// its tile plus a halo of 2 * step texels -- colour, both guides and, for
// PtGuided, the variance: 48 (52) B per texel, (16 + 4 * step)^2 texels, 19
// (21) KB at step 1 and 27 (30) KB at step 2 -- and takes the 5x5 taps and the
// 3x3 variance neighbours (1 <= 2 * step) from there.  Texels outside the
// image are not staged and never read.
constexpr int kFilterTile = (PT_ATROUS_T + 4 * PT_ATROUS_LDS_MAX_STEP) * (PT_ATROUS_T + 4 * PT_ATROUS_LDS_MAX_STEP);
template <class P>
__device__ __forceinline__ void filter_lds(const P &A) {
    __shared__ float4 sc[kFilterTile], sn[kFilterTile], sa[kFilterTile];
    __shared__ float sv[kWithVariance<P> ? kFilterTile : 1];  // (PtAtrous: never referenced, so never allocated)
    const int s = 1 << A.iter;  // (host: s <= PT_ATROUS_LDS_MAX_STEP)
    const int w = A.w, h = A.h;  // (read once, ahead of the loop: left in it they are carried across it in VGPRs)
    const int side = PT_ATROUS_T + 4 * s;
    const int x0 = int(blockIdx.x) * PT_ATROUS_T - 2 * s, y0 = int(blockIdx.y) * PT_ATROUS_T - 2 * s;
    const int tid = int(threadIdx.y) * PT_ATROUS_T + int(threadIdx.x);
    for (int i = tid; i < side * side; i += PT_ATROUS_T * PT_ATROUS_T) {
        const int ly = i / side, lx = i - ly * side;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx < 0 || gy < 0 || gx >= w || gy >= h) continue;
        const size_t q = size_t(gy) * size_t(w) + size_t(gx);
        sc[i] = A.in[q];
        sn[i] = A.g0[q];
        sa[i] = A.g1[q];
        if constexpr (kWithVariance<P>) sv[i] = A.vin[q];
    }
    __syncthreads();
    const int x = int(blockIdx.x) * PT_ATROUS_T + int(threadIdx.x), y = int(blockIdx.y) * PT_ATROUS_T + int(threadIdx.y);
    if (x >= A.w || y >= A.h) return;  // (the fields, as filter_pixel's bounds tests read them: those then fold)
    const int lp = (int(threadIdx.y) + 2 * s) * side + int(threadIdx.x) + 2 * s;
    auto tap = [&](int dx, int dy, float4 &c, float4 &n, float4 &a, float &v) {
        const int q = lp + s * dy * side + s * dx;
        c = sc[q];
        n = sn[q];
        a = sa[q];
        if constexpr (kWithVariance<P>) v = sv[q];
    };
    auto near = [&](int dx, int dy) {
        if constexpr (kWithVariance<P>) return sv[lp + dy * side + dx];
    };
    float v;
    const size_t p = size_t(y) * size_t(w) + size_t(x);
    const float4 c = filter_pixel(A, x, y, tap, near, v);
    filter_store(A, p, c, v);
}

__global__ __launch_bounds__(PT_ATROUS_BX *PT_ATROUS_BY) void pt_atrous_kernel(PtAtrous A) { filter_direct(A); }
__global__ __launch_bounds__(PT_ATROUS_T *PT_ATROUS_T) void pt_atrous_lds_kernel(PtAtrous A) { filter_lds(A); }
__global__ __launch_bounds__(PT_ATROUS_BX *PT_ATROUS_BY) void pt_guided_kernel(PtGuided A) { filter_direct(A); }
__global__ __launch_bounds__(PT_ATROUS_T *PT_ATROUS_T) void pt_guided_lds_kernel(PtGuided A) { filter_lds(A); }

// the LDS form at the steps it serves when asked for, else the direct form
template <class P>
static void launch_filter(const P &A, bool lds, void (*direct)(P), void (*staged)(P), hipStream_t stream) {
    if (A.w <= 0 || A.h <= 0) return;
    if (lds && (1 << A.iter) <= PT_ATROUS_LDS_MAX_STEP) {
        const dim3 grid(unsigned((A.w + PT_ATROUS_T - 1) / PT_ATROUS_T), unsigned((A.h + PT_ATROUS_T - 1) / PT_ATROUS_T));
        hipLaunchKernelGGL(staged, grid, dim3(PT_ATROUS_T, PT_ATROUS_T), 0, stream, A);
    } else {
        const dim3 grid(unsigned((A.w + PT_ATROUS_BX - 1) / PT_ATROUS_BX), unsigned((A.h + PT_ATROUS_BY - 1) / PT_ATROUS_BY));
        hipLaunchKernelGGL(direct, grid, dim3(PT_ATROUS_BX, PT_ATROUS_BY), 0, stream, A);
    }
}
void pt_launch_filter(const PtAtrous &A, bool lds, hipStream_t stream) {
    launch_filter(A, lds, pt_atrous_kernel, pt_atrous_lds_kernel, stream);
}
void pt_launch_filter(const PtGuided &A, bool lds, hipStream_t stream) {
    launch_filter(A, lds, pt_guided_kernel, pt_guided_lds_kernel, stream);
}

// ---- temporal accumulation (pt_temporal_accumulate) ----------
// (pixel_ray, pt_pixel.h, is the guide kernel's ray of a pixel under either view.)
// One thread per pixel, blocks 64 x 4 as pt_atrous_kernel: the current view's
// four 16 B loads per pixel are contiguous runs per wave, the history taps a
// near-coherent gather (neighbours reproject to neighbours).  A hit pixel's
// first-hit point goes through the previous camera's reciprocal basis to a
// position in the previous view; the four texels around it are taken
// bilinearly, each only if its own first-hit point lies near the pixel's
// tangent plane and its normal and albedo agree.  Every operation is one f32
// rounding in the order of DESIGN.md 3.30; no float is converted to int before
// the range test has passed, and every tap is tested against the image before
// it is loaded.  HBM-bound: 64 B of the current view and up to 4 x 68 B of
// history read, 36 B written per pixel.
__global__ __launch_bounds__(PT_ATROUS_BX *PT_ATROUS_BY) void pt_temporal_kernel(PtTemporal T) {
    const int x = int(blockIdx.x) * PT_ATROUS_BX + int(threadIdx.x), y = int(blockIdx.y) * PT_ATROUS_BY + int(threadIdx.y);
    if (x >= T.w || y >= T.h) return;
    const size_t p = size_t(y) * size_t(T.w) + size_t(x);
    const float4 a = T.a[p], m = T.m[p];
    float4 oh = a, om = m;  // (nothing taken: the current view; the alphas are the current view's either way)
    float on = T.n_cur;
    if (T.have) {
        const float4 g0 = T.g0[p], g1 = T.g1[p];
        if (g1.w != 0.0f && pt_finite_rgb(a) && pt_finite_rgb(m) && pt_finite_f(g0.w)) {
            pt_f3 ro, rd;
            pixel_ray(x, y, T.w, T.h, T.aspect, T.fov, T.cam_mode, T.cam, ro, rd);
            const pt_f3 X{ro.x + rd.x * g0.w, ro.y + rd.y * g0.w, ro.z + rd.z * g0.w};  // (the guide kernel's hit point)
            const pt_f3 d{X.x - T.po[0], X.y - T.po[1], X.z - T.po[2]};
            const float ca = pt_dot(d, pt_f3{T.ir[0], T.ir[1], T.ir[2]});
            const float cb = pt_dot(d, pt_f3{T.iu[0], T.iu[1], T.iu[2]});
            const float cc = pt_dot(d, pt_f3{T.ifw[0], T.ifw[1], T.ifw[2]});
            if (cc > 0.0f) {
                const float fw = float(T.w), fh = float(T.h);
                const float fx = ((((ca / cc) * T.pfov) / T.paspect) + 1.0f) * 0.5f * fw;
                const float fy = (((cb / cc) * T.pfov) + 1.0f) * 0.5f * fh;
                if (fx > -1.0f && fx < fw && fy > -1.0f && fy < fh) {  // (false for NaN; only now to int)
                    const float flx = floorf(fx), fly = floorf(fy);
                    const int x0 = int(flx), y0 = int(fly);
                    const float tx = fx - flx, ty = fy - fly;
                    const float tol = T.depth_tolerance * pt_sqrt(pt_dot(d, d));
                    const pt_f3 np{g0.x, g0.y, g0.z};
                    float sw = 0.0f, sn = 0.0f;
                    float shx = 0.0f, shy = 0.0f, shz = 0.0f, smx = 0.0f, smy = 0.0f, smz = 0.0f;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const int qx = x0 + i, qy = y0 + j;
                            if (qx < 0 || qy < 0 || qx >= T.w || qy >= T.h) continue;
                            const size_t q = size_t(qy) * size_t(T.w) + size_t(qx);
                            const float4 qa = T.pg1[q];
                            if (qa.w == 0.0f) continue;
                            const float qn = T.phn[q];
                            const float4 qh = T.ph[q], qm = T.phm[q];
                            if (!(qn > 0.0f) || !pt_finite_rgb(qh) || !pt_finite_rgb(qm)) continue;
                            const float4 qg = T.pg0[q];
                            pt_f3 qo, qd;
                            pixel_ray(qx, qy, T.w, T.h, T.paspect, T.pfov, T.pcam_mode, T.pcam, qo, qd);
                            const pt_f3 e{(qo.x + qd.x * qg.w) - X.x, (qo.y + qd.y * qg.w) - X.y, (qo.z + qd.z * qg.w) - X.z};
                            if (!(fabsf(pt_dot(e, np)) <= tol)) continue;  // distance to p's tangent plane
                            if (!(pt_dot(np, pt_f3{qg.x, qg.y, qg.z}) >= T.normal_cos)) continue;
                            const float ex = qa.x - g1.x, ey = qa.y - g1.y, ez = qa.z - g1.z;
                            if (!((ex * ex + ey * ey) + ez * ez <= T.at2)) continue;
                            const float w = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                            if (!(w > 0.0f)) continue;
                            sw = sw + w;
                            shx = shx + w * qh.x;
                            shy = shy + w * qh.y;
                            shz = shz + w * qh.z;
                            smx = smx + w * qm.x;
                            smy = smy + w * qm.y;
                            smz = smz + w * qm.z;
                            sn = sn + w * qn;
                        }
                    }
                    if (sw > 0.0f) {
                        const float hn = pt_gmin(sn / sw, T.max_history);
                        if (hn > 0.0f) {
                            const float n = hn + T.n_cur;
                            const float wgt = T.n_cur / n;
                            const float omw = 1.0f - wgt;
                            oh.x = (shx / sw) * omw + a.x * wgt;
                            oh.y = (shy / sw) * omw + a.y * wgt;
                            oh.z = (shz / sw) * omw + a.z * wgt;
                            om.x = (smx / sw) * omw + m.x * wgt;
                            om.y = (smy / sw) * omw + m.y * wgt;
                            om.z = (smz / sw) * omw + m.z * wgt;
                            on = n;
                        }
                    }
                }
            }
        }
    }
    T.oh[p] = oh;
    T.ohm[p] = om;
    T.ohn[p] = on;
}

void pt_launch_temporal(const PtTemporal &T, hipStream_t stream) {
    if (T.w <= 0 || T.h <= 0) return;
    const dim3 grid(unsigned((T.w + PT_ATROUS_BX - 1) / PT_ATROUS_BX), unsigned((T.h + PT_ATROUS_BY - 1) / PT_ATROUS_BY));
    hipLaunchKernelGGL(pt_temporal_kernel, grid, dim3(PT_ATROUS_BX, PT_ATROUS_BY), 0, stream, T);
}
