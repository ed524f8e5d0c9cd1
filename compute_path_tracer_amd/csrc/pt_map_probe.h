// pt_map_probe.h -- the probe kernels' bodies: a map type's
// map(), the shade pass's six normal taps and bounds() on caller-supplied
// inputs, one thread per input in 64-thread blocks (one wave), results per
// input.  Ahead of time they run the interpreter (InterpMap, bounds_mask:
// pt_map_probe.hip); in a probe module (pt_jit.cpp pt_probe_source) the
// scene's own generated JitMap / JitMapB0 / JitMapB1 and MapBounds<JitTaps>,
// the text the scene kernels are built from.  Nothing here is part of a
// pipeline kernel: the image tests remain the check of those as compiled.
#pragma once

#include "pt_binned.h"

struct PtProbe {
    PtLaunch L;               // the scene tables, fast_bounds, bound_k; stats for an instrumented run
    const float *xyz;         // [n][3] map: points; taps: hit points; bounds: ray origins
    const float *rd;          // [n][3] bounds: ray directions
    const uint64_t *check;    // [n][2] check[] bits 0..63, 64..127 (null: every bit set)
    const float *bnd;         // [n] the map() bound (null: +inf)
    const uint64_t *live_in;  // [n] map: the live mask handed in (null: 0)
    float *d;                 // [n] map, [n][6] taps (null: not stored; so the next two)
    int32_t *shape;           // ... Hit.m - 1: the PT_OP_SHAPE ordinal, -1 = none
    uint64_t *live_out;       // [n] the live mask after the call (taps: after the first tap)
    uint4 *mask;              // [n] bounds: the four mask words
    uint64_t *skip;           // [ceil(n / 64)] bounds, skip_mode 1: the wave's skip word
    uint32_t n;
    int32_t union_mode;       // map: 1 = Check.alo/ahi are the wave's union of masks (0: all ones)
    int32_t skip_mode;        // bounds: 1 = primary_box_skip, then mask_skip
    int32_t pad;
};

namespace pt {

// One map() call per input.  Every lane of the wave makes the call, so the
// wave-level steps (the check[] union, the shortcuts' ballots) see a full
// wave; a lane beyond n carries an empty mask -- no shape behind a box is
// evaluated for it -- and stores nothing.  A point with a non-finite
// coordinate is mapped as (NaN, NaN, NaN), as pt_sample_field maps it.  bndw is
// the bound widened as the shade pass widens it, about the point itself.
template <class Map, bool ST>
__device__ __forceinline__ void probe_map_body(const PtProbe &P) {
    Stats<ST> st;
    st.init();
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool in = i < P.n;
    Check ck{0ull, 0ull};
    float x = 0.0f, y = 0.0f, z = 0.0f, bnd = __builtin_inff();
    uint64_t live = 0ull;
    if (in) {
        x = P.xyz[3 * size_t(i)], y = P.xyz[3 * size_t(i) + 1], z = P.xyz[3 * size_t(i) + 2];
        if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) x = y = z = __builtin_nanf("");
        ck.lo = P.check ? P.check[2 * size_t(i)] : ~0ull;
        ck.hi = P.check ? P.check[2 * size_t(i) + 1] : ~0ull;
        if (P.bnd) bnd = P.bnd[i];
        if (P.live_in) live = P.live_in[i];
    }
    if (P.union_mode) {  // (as the trace pass's park() forms them)
        ck.alo = wave_or_u64(ck.lo);
        ck.ahi = wave_or_u64(ck.hi);
    }
    const float bndw = bnd + (0x1.a3ap-13f + 0x1p-20f * (fabsf(x) + fabsf(y) + fabsf(z)));
    if constexpr (ST)
        if (first_active_lane()) st.add(PT_ST_WAVE_MAPS);
    const Hit h = Map::template eval<ST>(P.L, x, y, z, ck, bnd, bndw, live, st);
    if (in) {
        if (P.d) P.d[i] = h.d;
        if (P.shape) P.shape[i] = h.m - 1;
        if (P.live_out) P.live_out[i] = live;
    }
    flush_stats<ST>(P.L, st);
}

// calc_normal's six taps of the shade pass around each hit point:
// bin_shade_body's loop (TAPS = false) written out again, with every tap's
// map() value and shape stored instead of the differences.
template <class Taps, bool ST>
__device__ __forceinline__ void probe_taps_body(const PtProbe &P) {
    Stats<ST> stt;
    stt.init();
    const PtLaunch &L = P.L;
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool in = i < P.n;
    pt_f3 ro{0.0f, 0.0f, 0.0f};
    Check ck{0ull, 0ull};
    float bnd = __builtin_inff();
    if (in) {
        ro = pt_f3{P.xyz[3 * size_t(i)], P.xyz[3 * size_t(i) + 1], P.xyz[3 * size_t(i) + 2]};
        ck.lo = P.check ? P.check[2 * size_t(i)] : ~0ull;
        ck.hi = P.check ? P.check[2 * size_t(i) + 1] : ~0ull;
        if (P.bnd) bnd = P.bnd[i];
    }
    const pt_f3 rd = ro;  // (map_point reads no direction for a tap)
    const float bndw = bnd + (0x1.a3ap-13f + 0x1p-20f * (fabsf(ro.x) + fabsf(ro.y) + fabsf(ro.z)));
    uint64_t live = 0ull;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        float qx, qy, qz;
        map_point(ST_NORMAL, k, ro, rd, 0.0f, qx, qy, qz);
        if constexpr (ST)
            if (first_active_lane()) stt.add(PT_ST_WAVE_MAPS);
        const Hit h = k == 0 ? Taps::template first<ST>(L, qx, qy, qz, ck, bnd, bndw, live, stt)
                             : Taps::template rest<ST>(L, qx, qy, qz, ck, bnd, bndw, live, stt);
        if (k == 0) {
            ck.alo = Taps::alive(live);  // (the other taps' wave-level live test)
            if (in && P.live_out) P.live_out[i] = live;
        }
        if (in) {
            if (P.d) P.d[6 * size_t(i) + size_t(k)] = h.d;
            if (P.shape) P.shape[6 * size_t(i) + size_t(k)] = h.m - 1;
        }
    }
    stt.add(PT_ST_NORMAL_MAPS, 6);
    flush_stats<ST>(L, stt);
}

// bounds() of each ray.  The lanes beyond n sit out, as the lanes without a
// ray do in the passes.  skip_mode 1: what the first pass's stage() does -- a
// full wave asks primary_box_skip which boxes none of its rays can hit and
// hands the answer to mask_skip; a ragged wave skips nothing.
template <class Map, bool ST>
__device__ __forceinline__ void probe_bounds_body(const PtProbe &P) {
    Stats<ST> st;
    st.init();
    const PtLaunch &L = P.L;
    const uint32_t base = blockIdx.x * 64u, i = base + threadIdx.x;
    const uint32_t cnt = P.n - base < 64u ? P.n - base : 64u;
    if (i < P.n) {
        const pt_f3 ro{P.xyz[3 * size_t(i)], P.xyz[3 * size_t(i) + 1], P.xyz[3 * size_t(i) + 2]};
        const pt_f3 rd{P.rd[3 * size_t(i)], P.rd[3 * size_t(i) + 1], P.rd[3 * size_t(i) + 2]};
        uint4 m;
        if (P.skip_mode) {
            const uint64_t skip = cnt == 64u ? primary_box_skip(L, ro, rd) : 0ull;
            m = MapBounds<Map>::template mask_skip<ST>(L, ro, rd, skip, st);
            if (threadIdx.x == 0u && P.skip) P.skip[blockIdx.x] = skip;
        } else {
            m = MapBounds<Map>::template mask<ST>(L, ro, rd, st);
        }
        P.mask[i] = m;
    }
    flush_stats<ST>(L, st);
}

}  // namespace pt
