// pt_path.h -- the per-lane path arithmetic of the state-machine kernels
// (pt_wave.h: tile-resident wavefront, pt_binned.h: mask-binned passes).
// One definition of each step, so both schedules compute every sample with
// the same f32 operations as pt_kernel.hip's reference-structured loop and
// the oracle.
#pragma once

#include "pt_common.h"

namespace pt {

enum : int { ST_FREE = 0, ST_BOUNDS = 1, ST_MARCH = 2, ST_NORMAL = 3, ST_SHADE = 4 };

// Which cameras a kernel instance serves (camera_ray's CAM): the first binned
// pass, shade pass 0 and the gen pass of the scene kernels sit at their
// register budget with the fixed camera's origin folded into their code as
// constants, so they are built once for the fixed camera alone -- the code
// they always had -- and once for a posed one, and the host launches the one
// that matches (pt_runtime.hip).  Every other kernel branches on the launch
// block's cam_mode, which is wave-uniform.
#define PT_CAMK_ANY (-1)   // branch on cam_mode at run time
#define PT_CAMK_FIXED 0    // PT_CAM_DEFAULT only
#define PT_CAMK_POSED 1    // PT_CAM_PINHOLE / PT_CAM_LENS only

// Camera ray of pixel (x, y) in frame `frame`: gen_rng, sub-pixel jitter,
// calc_uv and the camera.  PT_CAM_DEFAULT: the reference's fixed pinhole
// (test_compute.glsl:224-235), in its own code: the general formula's
// ux * 1 + uy * 0 would turn a -0 into +0.  PT_CAM_PINHOLE / PT_CAM_LENS: the
// pose and lens of pt_set_camera, read from the launch block
// where they are used -- kernel arguments in scalar registers, never per-lane
// state.  The lens draws its two numbers directly after the jitter's, and
// the rng it leaves is the one the path goes on with.
// The camera of a sample whose scaled uv is (ux, uy) -- what camera_ray runs
// once the jitter and calc_uv have formed them: the fixed pinhole in its own
// code path, or the posed basis and, for PT_CAM_LENS, the lens.
template <int CAM = PT_CAMK_ANY>
__device__ __forceinline__ void camera_from_uv(float ux, float uy, float fov, int cam_mode, const pt_camera &cam,
                                               uint32_t &rng, pt_f3 &ro, pt_f3 &rd) {
    if (CAM == PT_CAMK_FIXED || (CAM == PT_CAMK_ANY && cam_mode == PT_CAM_DEFAULT)) {
        rd = pt_normalize(pt_f3{ux, uy, fov});
        ro = pt_f3{0.0f, 0.0f, -3.0f};
        return;
    }
    const float *org = cam.origin, *right = cam.right, *up = cam.up, *fwd = cam.forward;
    rd = pt_normalize(pt_f3{(right[0] * ux + up[0] * uy) + fwd[0] * fov, (right[1] * ux + up[1] * uy) + fwd[1] * fov,
                            (right[2] * ux + up[2] * uy) + fwd[2] * fov});
    ro = pt_f3{org[0], org[1], org[2]};
    if (cam_mode == PT_CAM_LENS) {
        // a point of the lens disc (radius aperture, spanned by right / up)
        // aimed at the pinhole ray's point at distance focus
        const float aperture = cam.aperture, focus = cam.focus;
        const float u1 = pt_random01(rng);
        const float u2 = pt_random01(rng);
        const float r = pt_sqrt(u1) * aperture;
        const float a = u2 * kPi2;
        float sa, ca;
        pt_sincos(a, sa, ca);
        const float lx = r * ca, ly = r * sa;
        const pt_f3 pf{ro.x + rd.x * focus, ro.y + rd.y * focus, ro.z + rd.z * focus};
        ro = pt_f3{(ro.x + right[0] * lx) + up[0] * ly, (ro.y + right[1] * lx) + up[1] * ly,
                   (ro.z + right[2] * lx) + up[2] * ly};
        rd = pt_normalize(pt_f3{pf.x - ro.x, pf.y - ro.y, pf.z - ro.z});
    }
}
template <int CAM = PT_CAMK_ANY>
__device__ __forceinline__ void camera_ray(int x, int y, int32_t frame, int width, int height, float aspect, float fov,
                                           int cam_mode, const pt_camera &cam, uint32_t &rng, pt_f3 &ro, pt_f3 &rd) {
    rng = pt_gen_rng(x, y, frame, width, height);
    float jx = pt_random01(rng);
    float jy = pt_random01(rng);
    jx = jx - 0.5f;
    jy = jy - 0.5f;
    float ux = (float(x) + jx) / float(width), uy = (float(y) + jy) / float(height);
    ux = ux * 2.0f - 1.0f;
    uy = uy * 2.0f - 1.0f;
    ux *= aspect;
    camera_from_uv<CAM>(ux, uy, fov, cam_mode, cam, rng, ro, rd);
}

// Radiance of the sky (pt_set_sky) along direction rd: the
// vertical gradient, plus the sun's colour inside its disc.  f32, no
// contraction, in this order.  The sky itself is read from the launch block
// where it is used -- kernel arguments in scalar registers, never per-lane
// state.
__device__ __forceinline__ pt_f3 sky_radiance(const pt_sky &sky, const pt_f3 &rd) {
    const float t = rd.y * 0.5f + 0.5f;
    pt_f3 g{sky.bottom[0] + (sky.top[0] - sky.bottom[0]) * t, sky.bottom[1] + (sky.top[1] - sky.bottom[1]) * t,
            sky.bottom[2] + (sky.top[2] - sky.bottom[2]) * t};
    const float s = pt_dot(rd, pt_f3{sky.sun_dir[0], sky.sun_dir[1], sky.sun_dir[2]});
    if (s >= sky.sun_cos) {
        g.x = g.x + sky.sun_color[0];
        g.y = g.y + sky.sun_color[1];
        g.z = g.z + sky.sun_color[2];
    }
    return g;
}

// A segment that missed (CastRay's t > FP, test_compute.glsl:106) with a sky
// set: ret += sky_radiance(rd) * thr before the path ends.  Behind the launch
// block's sky_mode, which is wave-uniform (a scalar branch: without a sky the
// lanes skip the whole term).  No rng draw.
__device__ __forceinline__ void sky_miss(const PtLaunch &L, const pt_f3 &rd, const pt_f3 &thr, pt_f3 &ret) {
    if (L.sky_mode == PT_SKY_OFF) return;
    // (the sky's offset in the launch block through an empty asm: read as
    // L.sky, the 13 loads are loop-invariant kernel arguments, the compiler
    // hoists them out of the wave kernel's main loop, and their scalar
    // registers, held across the whole body, cost the C3 scene kernel 9
    // VGPRs of spills and one wave of occupancy -- with or without a sky.
    // With an offset it cannot see, the loads stay inside this branch.)
    uint32_t off = uint32_t(__builtin_offsetof(PtLaunch, sky));
    __asm__ volatile("" : "+s"(off));
    const pt_sky &sky = *reinterpret_cast<const pt_sky *>(reinterpret_cast<const char *>(&L) + off);
    const pt_f3 g = sky_radiance(sky, rd);
    ret.x = ret.x + g.x * thr.x;
    ret.y = ret.y + g.y * thr.y;
    ret.z = ret.z + g.z * thr.z;
}

// The slab test's tail, intersectAABB + bool_hit (aabb.glsl:21-33), stated
// once for the five forms below: the ray's parameter range inside the three
// slabs from the six slab values, and the hit test on it.  DESIGN.md 3.14,
// 3.18 and 3.19 argue about these two functions.
__device__ __forceinline__ void slab_ends(float tminx, float tmaxx, float tminy, float tmaxy, float tminz, float tmaxz,
                                          float &tnear, float &tfar) {
    tnear = pt_gmax(pt_gmax(pt_gmin(tminx, tmaxx), pt_gmin(tminy, tmaxy)), pt_gmin(tminz, tmaxz));
    tfar = pt_gmin(pt_gmin(pt_gmax(tminx, tmaxx), pt_gmax(tminy, tmaxy)), pt_gmax(tminz, tmaxz));
}
__device__ __forceinline__ bool slab_hit(float tnear, float tfar) { return tnear < tfar && tfar > 0.0f; }

// The ray inside the reciprocal guard (pt_math.h pt_div_*_ok): with the
// scene's boxes inside it too (L.fast_bounds), bounds() may take its slab
// values from per-ray reciprocals.  The fast path of bounds_mask, the box skip
// (pt_binned.h; 3.20's proof needs the two to agree) and the self-test use
// this one; the generated bounds() keeps its own `&` form of the same six
// tests (pt_jit.cpp emit_map_bounds).
__device__ __forceinline__ bool ray_in_guard(const pt_f3 &ro, const pt_f3 &rd) {
    return pt_div_coord_ok(ro.x) && pt_div_coord_ok(ro.y) && pt_div_coord_ok(ro.z) && pt_div_dir_ok(rd.x) &&
           pt_div_dir_ok(rd.y) && pt_div_dir_ok(rd.z);
}

// bounds(): one box's slab test as the generated bounds() applies it per check[] entry.
__device__ __forceinline__ bool ray_box(const PtAabb &bx, float ox, float oy, float oz, float dx, float dy, float dz) {
    float tnear, tfar;
    slab_ends((bx.bmin[0] - ox) / dx, (bx.bmax[0] - ox) / dx, (bx.bmin[1] - oy) / dy, (bx.bmax[1] - oy) / dy,
              (bx.bmin[2] - oz) / dz, (bx.bmax[2] - oz) / dz, tnear, tfar);
    return slab_hit(tnear, tfar);
}

// The same test with the divisions as pt_div_rcp from per-ray reciprocals
// (y = RN(1/d)); bit-identical results when the pt_div_*_ok guards hold for
// the ray and the box (bounds_mask in pt_binned.h).
__device__ __forceinline__ bool ray_box_rcp(const PtAabb &bx, float ox, float oy, float oz, float dx, float dy,
                                            float dz, float yx, float yy, float yz) {
    float tnear, tfar;
    slab_ends(pt_div_rcp(bx.bmin[0] - ox, dx, yx), pt_div_rcp(bx.bmax[0] - ox, dx, yx),
              pt_div_rcp(bx.bmin[1] - oy, dy, yy), pt_div_rcp(bx.bmax[1] - oy, dy, yy),
              pt_div_rcp(bx.bmin[2] - oz, dz, yz), pt_div_rcp(bx.bmax[2] - oz, dz, yz), tnear, tfar);
    return slab_hit(tnear, tfar);
}

// The slab ends from the reciprocal products alone: t' = RN(a * y) with a =
// RN(bmin - o) as in ray_box_rcp and y = RN(1/d) (ray_box_approx, ray_box_ulp).
__device__ __forceinline__ void slab_ends_rcp(const PtAabb &bx, float ox, float oy, float oz, float yx, float yy,
                                              float yz, float &tnear, float &tfar) {
    slab_ends((bx.bmin[0] - ox) * yx, (bx.bmax[0] - ox) * yx, (bx.bmin[1] - oy) * yy, (bx.bmax[1] - oy) * yy,
              (bx.bmin[2] - oz) * yz, (bx.bmax[2] - oz) * yz, tnear, tfar);
}

// The slab test from those products.  Under the same guards,
// |t' - t| <= 3 * 2^-24 |t| for every slab value t = RN(a / d), and t' has
// t's sign and zeros, so:
//  * tfar' > 0 exactly when tfar > 0 (min / max keep the signs);
//  * tnear < tfar is decided by tnear' < tfar' whenever |tfar' - tnear'| >
//    2^-20 (|tnear'| + |tfar'|) (min / max move each end by <= 2^-22 of
//    itself); `gap` keeps the least |tfar' - tnear'| - that margin over the
//    boxes tested, and a lane whose gap is <= 0 takes ray_box_rcp.
__device__ __forceinline__ bool ray_box_approx(const PtAabb &bx, float ox, float oy, float oz, float yx, float yy,
                                               float yz, float &gap) {
    float tnear, tfar;
    slab_ends_rcp(bx, ox, oy, oz, yx, yy, yz, tnear, tfar);
    gap = fminf(gap, fabsf(tfar - tnear) - (fabsf(tnear) + fabsf(tfar)) * 0x1p-20f);
    return slab_hit(tnear, tfar);
}

// ray_box_approx with the margin in units of the last place (DESIGN.md
// 3.19): each slab value t' is within 4 representable steps of the IEEE slab
// value (3 roundings of <= 2^-24 relative each), with the same sign and
// zeros, so min / max keep tnear' and tfar' within 4 steps of the IEEE tnear
// and tfar, and tnear' < tfar' decides tnear < tfar whenever the two bit
// patterns differ by more than 8 (opposite signs differ by >= 2^31 and are
// decided by the signs).  `gapu` keeps the least |bits(tfar') -
// bits(tnear')| (v_sad_u32: one instruction, against four for the float
// margin); a lane whose gapu is <= PT_ULP_MARGIN takes ray_box_rcp.
#define PT_ULP_MARGIN 16u
// (SAD false: max - min, for loops the compiler is to unroll -- inline asm is
// convergent, which blocks a runtime-count unroll)
template <bool SAD = true>
__device__ __forceinline__ uint32_t pt_absdiff_u32(uint32_t a, uint32_t b) {
    if constexpr (!SAD) return max(a, b) - min(a, b);
    uint32_t d;
    __asm__("v_sad_u32 %0, %1, %2, 0" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
template <bool SAD = true>
__device__ __forceinline__ bool ray_box_ulp(const PtAabb &bx, float ox, float oy, float oz, float yx, float yy,
                                            float yz, uint32_t &gapu) {
    float tnear, tfar;
    slab_ends_rcp(bx, ox, oy, oz, yx, yy, yz, tnear, tfar);
    gapu = min(gapu, pt_absdiff_u32<SAD>(__float_as_uint(tfar), __float_as_uint(tnear)));
    return slab_hit(tnear, tfar);
}

// The slab test from one fma per slab: t' = RN(b * y + n) with n = -RN(o * y)
// per ray and axis, y = RN(1/d).  Under the guards of ray_box_rcp,
// |t' - t| <= 2^-21 |t| + 2^-23 M for every slab value t = RN(RN(b - o) / d),
// M = max over the axes of |n| (the product's rounding adds an absolute
// term: DESIGN.md 3.18).  `gap` as in ray_box_approx and `tfa` (the least
// |tfar'|) decide a lane when gap > 2^-21 M and tfa > 2^-22 M (fma_decided);
// an undecided lane takes ray_box_rcp.  One fma per slab instead of a
// subtraction and a product.
__device__ __forceinline__ bool ray_box_fma(const PtAabb &bx, float nx, float ny, float nz, float yx, float yy,
                                            float yz, float &gap, float &tfa) {
    float tnear, tfar;
    slab_ends(fmaf(bx.bmin[0], yx, nx), fmaf(bx.bmax[0], yx, nx), fmaf(bx.bmin[1], yy, ny), fmaf(bx.bmax[1], yy, ny),
              fmaf(bx.bmin[2], yz, nz), fmaf(bx.bmax[2], yz, nz), tnear, tfar);
    gap = fminf(gap, fabsf(tfar - tnear) - (fabsf(tnear) + fabsf(tfar)) * 0x1p-20f);
    tfa = fminf(tfa, fabsf(tfar));
    return slab_hit(tnear, tfar);
}
__device__ __forceinline__ bool fma_decided(float gap, float tfa, float nx, float ny, float nz) {
    const float m = pt_gmax(fabsf(nx), pt_gmax(fabsf(ny), fabsf(nz)));
    return gap > m * 0x1p-21f && tfa > m * 0x1p-22f;
}

// The map() argument of a lane: CastRay's p = ro + rd*t (MARCH), or normal
// tap `step` (0..5 = +x,-x,+y,-y,+z,-z) around the hit point held in ro
// (calc_normal, test_compute.glsl:57-66).
__device__ __forceinline__ void map_point(int state, int step, const pt_f3 &ro, const pt_f3 &rd, float t, float &qx,
                                          float &qy, float &qz) {
    if (state == ST_MARCH) {
        qx = ro.x + rd.x * t;
        qy = ro.y + rd.y * t;
        qz = ro.z + rd.z * t;
    } else {
        const float e = 0.0001f;
        const int axis = step >> 1;
        const bool neg = (step & 1) != 0;
        const float on = neg ? -e : e, off = neg ? -0.0f : 0.0f;
        qx = ro.x + (axis == 0 ? on : off);
        qy = ro.y + (axis == 1 ? on : off);
        qz = ro.z + (axis == 2 ? on : off);
    }
}

// calc_normal's bookkeeping for tap k with map() value d: an even tap keeps
// d(p + e) in dplus, an odd one stores d(p + e) - d(p - e) for its axis.
__device__ __forceinline__ void normal_tap(int k, float d, float &dplus, float &dv0, float &dv1, float &dv2) {
    if ((k & 1) == 0) {
        dplus = d;
    } else {
        const float dd = dplus - d;
        if (k == 1) dv0 = dd;
        else if (k == 3) dv1 = dd;
        else dv2 = dd;
    }
}

// calc_normal (funcs.glsl:21-35): central differences, e = 1e-4, over
// map_point's six taps (the zero components of -e are -0.0, so p.y + (-0.0)
// == p.y exactly); MapAt(x, y, z, args...) is the map() distance at a point (a
// function, not a closure: with a closure in an out-of-line caller the simple
// kernel copies its launch block to scratch).  The caller normalises.
template <auto MapAt, class... Args>
__device__ __forceinline__ pt_f3 calc_normal(const pt_f3 &p, Args &&...args) {
    float dv[3], dplus = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        float qx, qy, qz;
        map_point(ST_NORMAL, k, p, p, 0.0f, qx, qy, qz);
        const float d = MapAt(qx, qy, qz, args...);
        // (normal_tap written out on an array: through it mesh_vertex_kernel gains 28 instructions, 0.665 -> 0.667 ms)
        if ((k & 1) == 0) dplus = d;
        else dv[k >> 1] = dplus - d;
    }
    return pt_f3{dv[0], dv[1], dv[2]};
}

// Advance a MARCH / NORMAL lane by the map() result h.  MARCH: CastRay's loop
// body and exit tests (test_compute.glsl:42-54); on exit either a miss
// (-> SHADE with step = -1) or calc_point into ro (-> NORMAL).  NORMAL: the
// six taps give the central differences d(p+e) - d(p-e) per axis.
// MARCH_ONLY: the caller never maps a NORMAL lane (the binned trace pass
// whose shade pass takes the taps), so the taps' branch is left out.
template <bool ST, bool MARCH_ONLY = false>
__device__ __forceinline__ void after_map(const Hit &h, int &state, int &step, float &t, pt_f3 &ro, const pt_f3 &rd,
                                          int &mat, float &dv0, float &dv1, float &dv2, Stats<ST> &st) {
    if (MARCH_ONLY || state == ST_MARCH) {
        st.add(PT_ST_MARCH);
        mat = h.m;
        t += h.d;
        ++step;
        if (fabsf(h.d) < kMhd || t > kFp || step == kSteps) {
            if (t > kFp) {
                state = ST_SHADE;  // miss: path ends
                step = -1;
            } else {
                ro = pt_f3{ro.x + rd.x * t, ro.y + rd.y * t, ro.z + rd.z * t};  // calc_point
                state = ST_NORMAL;
                step = 0;
            }
        }
    } else if constexpr (!MARCH_ONLY) {
        normal_tap(step, h.d, t, dv0, dv1, dv2);  // (t keeps d(p + e))
        ++step;
        if (step == 6) {
            st.add(PT_ST_NORMAL_MAPS, 6);
            state = ST_SHADE;
        }
    }
}

// Upper bound on map() at every calc_normal tap of a hit:
// the march's last map() value was d at point q (t: the ray parameter after
// t += d), the hit point is |d| further along the ray and each tap e = 1e-4
// from it.  map() is 1-Lipschitz (a min/max/assign composition of exact SDFs
// under rotations, scales and translations) up to the rotation constants'
// rounding (x(1 + 2^-16)); mg covers the f32 rounding of the two evaluations
// and of the point arithmetic: a few tens of ulp of |q|_1 + |d| + t + bk,
// bk = the scene's transform-chain magnitude (pt_bound_k; NaN: no bound).
__device__ __forceinline__ float tap_bound(float d, float qx, float qy, float qz, float t, float bk) {
    const float ad = fabsf(d);
    const float mg = 0x1p-10f * (fabsf(qx) + fabsf(qy) + fabsf(qz) + ad + fabsf(t) + bk);
    return ((d + ad) * 0x1.0001p+0f + mg) + 0x1.a38p-14f;  // + e = 1e-4 (x(1 + 2^-16), rounded up)
}

// Shading of a hit and Russian roulette (test_compute.glsl:116-159).
// Returns true when the path ends here (miss: step < 0, roulette, or the
// bounce limit); otherwise ro/rd/thr hold the next segment's ray and seg was
// incremented.
template <bool ST>
__device__ __forceinline__ bool shade_lane(const PtMat *__restrict__ mats, int bounces, int mat, float dv0, float dv1,
                                           float dv2, int step, uint32_t &rng, pt_f3 &ro, pt_f3 &rd, pt_f3 &thr,
                                           pt_f3 &ret, int &seg, Stats<ST> &st) {
    if (step < 0) return true;  // miss
    const pt_f3 n = pt_normalize(pt_f3{dv0, dv1, dv2});
    const pt_f3 hp = ro;
    ro = pt_f3{hp.x + n.x * kOffset, hp.y + n.y * kOffset, hp.z + n.z * kOffset};
    st.add(PT_ST_SHADED);
    const PtMat &m = mats[mat];
    const float spec_chance = m.spec;
    const bool do_spec = pt_random01(rng) < spec_chance;
    float ray_prob = do_spec ? spec_chance : 1.0f - spec_chance;
    ray_prob = pt_gmax(ray_prob, 0.0001f);
    const float uz = pt_random01(rng) * 2.0f - 1.0f;
    const float ua = pt_random01(rng) * kPi2;
    const float ur = pt_sqrt(1.0f - uz * uz);
    float sa, ca;
    pt_sincos(ua, sa, ca);
    const pt_f3 diffuse = pt_normalize(pt_f3{n.x + ur * ca, n.y + ur * sa, n.z + uz});
    if (do_spec) {
        const float k = 2.0f * pt_dot(n, rd);
        const pt_f3 sr{rd.x - k * n.x, rd.y - k * n.y, rd.z - k * n.z};
        const float al = m.rough2, oma = 1.0f - al;
        rd = pt_normalize(pt_f3{sr.x * oma + diffuse.x * al, sr.y * oma + diffuse.y * al, sr.z * oma + diffuse.z * al});
    } else {
        rd = diffuse;
    }
    const float fs = do_spec ? 1.0f : 0.0f, omf = 1.0f - fs;
    ret.x += m.emis[0] * thr.x;
    ret.y += m.emis[1] * thr.y;
    ret.z += m.emis[2] * thr.z;
    thr.x *= m.col[0] * omf + m.spec_col[0] * fs;
    thr.y *= m.col[1] * omf + m.spec_col[1] * fs;
    thr.z *= m.col[2] * omf + m.spec_col[2] * fs;
    thr.x /= ray_prob;
    thr.y /= ray_prob;
    thr.z /= ray_prob;
    const float pmax = pt_gmax(thr.x, pt_gmax(thr.y, thr.z));
    if (pt_random01(rng) > pmax) {
        st.add(PT_ST_RR_BREAK);
        return true;
    }
    const float ip = 1.0f / pmax;
    thr.x *= ip;
    thr.y *= ip;
    thr.z *= ip;
    ++seg;
    return seg > bounces;
}

// The sample's colour once its path ended (debug 3: bounce count, :163).
__device__ __forceinline__ pt_f3 final_color(int debug, int seg, int bounces, const pt_f3 &ret) {
    if (debug == 3) {
        const float v = float(seg) / float(bounces);
        return pt_f3{v, v, v};
    }
    return ret;
}

// One frame into a texel's running colour: mix(last, colour, 1 / (last_clear
// + 1)) as x * (1 - w) + y * w (test_compute.glsl:242-245).
__device__ __forceinline__ void mix_frame(float &ar, float &ag, float &ab, const pt_f3 &colour, int32_t last_clear) {
    const float w = 1.0f / float(last_clear + 1), omw = 1.0f - w;
    ar = ar * omw + colour.x * w;
    ag = ag * omw + colour.y * w;
    ab = ab * omw + colour.z * w;
}

// Tile to pixel.  Ranks own the 8x8 tiles cyclically: a rank's local tile k is
// tile g = rank + k * nranks of the image, row-major; lane p of a tile is pixel
// (p & 7, p >> 3) from its origin.  pixel_of: local pixel slot pl = k * 64 + p.
// (One function per term: pixel_of over a two-step origin / offset pair
// reordered instructions of the scene kernels' gen pass.)
__device__ __forceinline__ int tile_index(int rank, int nranks, int k) { return rank + k * nranks; }
__device__ __forceinline__ int tile_x0(int g, int tiles_x) { return (g % tiles_x) * PT_TILE; }
__device__ __forceinline__ int tile_y0(int g, int tiles_x) { return (g / tiles_x) * PT_TILE; }
__device__ __forceinline__ int lane_dx(int p) { return p & 7; }
__device__ __forceinline__ int lane_dy(int p) { return p >> 3; }
__device__ __forceinline__ void pixel_of(int rank, int nranks, int tiles_x, uint32_t pl, int &x, int &y) {
    const int k = int(pl >> 6), p = int(pl & 63u);
    const int g = tile_index(rank, nranks, k);
    x = tile_x0(g, tiles_x) + lane_dx(p);
    y = tile_y0(g, tiles_x) + lane_dy(p);
}
__device__ __forceinline__ void pixel_of(const PtLaunch &L, uint32_t pl, int &x, int &y) {
    pixel_of(L.rank, L.nranks, L.tiles_x, pl, x, y);
}

// The accumulation texel of pixel (x, y) over a launch: its address, its
// running colour, and the (r, g, b, 1) store.  accum_mixes: the launch starts
// from the texel's colour only when it mixes frames into it -- a debug view
// stores its last frame, and write = 0 leaves the image alone.  first_frame: a
// debug view renders only the launch's last frame, the one its store keeps.
__device__ __forceinline__ float4 *accum_texel(const PtLaunch &L, int x, int y) {
    return reinterpret_cast<float4 *>(L.accum + (size_t(y) * size_t(L.width) + size_t(x)) * 4);
}
__device__ __forceinline__ bool accum_mixes(const PtLaunch &L) { return L.debug == 0 && L.write; }
__device__ __forceinline__ void accum_load(const float4 *texel, float &ar, float &ag, float &ab) {
    const float4 v = *texel;
    ar = v.x;
    ag = v.y;
    ab = v.z;
}
__device__ __forceinline__ void accum_store(float4 *texel, float ar, float ag, float ab) {
    *texel = make_float4(ar, ag, ab, 1.0f);
}
__device__ __forceinline__ int first_frame(const PtLaunch &L) { return L.debug != 0 ? L.spp - 1 : 0; }

}  // namespace pt
