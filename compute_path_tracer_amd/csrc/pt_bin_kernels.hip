// pt_bin_kernels.hip -- the ahead-of-time kernels of the mask-binned pass
// pipeline (pt_binned.h, PT_KERNEL_BINNED):
//
//   pt_bin_gen_kernel, pt_bin_shade_kernel, pt_bin_trace_kernel
//                     pt_binned.h's gen, shade and trace bodies over the op-list
//                     interpreter; per-scene hipRTC builds of the same bodies
//                     replace them when available (pt_jit.cpp).
//   pt_bin_scan_kernel, pt_bin_scatter_kernel   bin order from the histogram.
//   pt_bin_sky_kernel the sky for a trace pass's misses (pt_set_sky).
//   pt_bin_fold_kernel, pt_bin_fold_m_kernel    each pixel mixes its frames; the
//                     second also keeps the moment image (option "moments").
// The four fixed passes -- scan, scatter, sky, fold -- evaluate no map(), so no
// scene has a build of them: they are written here and not in pt_binned.h,
// which every scene's runtime-compiled source includes and whose text is part
// of the scene kernels' cache key.  An edit to them leaves that key alone.
// Scan, scatter and fold are inlined bodies that take the pass block by
// reference under one-line kernels, as the three bodies of pt_binned.h are:
// written on the kernel's own by-value argument, scan and scatter compile to
// other instructions (EXPERIMENTS.md).
#include "pt_binned.h"
#include "pt_host.h"
#include "pt_pixel.h"

using namespace pt;

template <bool ST>
__global__ __launch_bounds__(PT_BIN_BLOCK) void pt_bin_gen_kernel(PtPass P) {
    bin_gen_body<InterpMap, ST>(P);
}
template <bool ST>
__global__ __launch_bounds__(PT_BIN_BLOCK) void pt_bin_shade_kernel(PtPass P) {
    bin_shade_body<InterpMap, ST, true>(P);
}
template <bool ST>
__global__ __launch_bounds__(64) void pt_bin_trace_kernel(PtPass P) {
    bin_trace_body<InterpMap, ST>(P);
}

// scan: exclusive prefix of the histogram; clears the histogram and this
// pass's cursors.  One wave (PT_SCAN_THREADS lanes, PT_BINS / 64 bins each,
// no LDS): it fits on a CU beside the other pipeline's persistent trace
// waves (28 of 32 slots), where a 1024-thread block waited for that trace
// pass to drain (1.26 ms per launch with two pipelines, 5 us alone).
#define PT_SCAN_THREADS 64
__device__ __forceinline__ void scan_body(const PtPass &P) {
    constexpr int PER = PT_BINS / PT_SCAN_THREADS;
    const int t = int(threadIdx.x);
    uint4 *h4 = reinterpret_cast<uint4 *>(P.hist + t * PER);
    uint4 *o4 = reinterpret_cast<uint4 *>(P.offs + t * PER);
    uint32_t sum = 0u;
#pragma unroll
    for (int j = 0; j < PER / 4; ++j) {
        const uint4 v = h4[j];
        sum += v.x + v.y + v.z + v.w;
    }
    uint32_t inc = sum;  // inclusive prefix over the wave's lanes
#pragma unroll
    for (int off = 1; off < PT_SCAN_THREADS; off <<= 1) {
        const uint32_t x = uint32_t(__shfl_up(int(inc), off, PT_SCAN_THREADS));
        if (t >= off) inc += x;
    }
    uint32_t run = inc - sum;
#pragma unroll
    for (int j = 0; j < PER / 4; ++j) {
        const uint4 v = h4[j];
        uint4 o;
        o.x = run;
        run += v.x;
        o.y = run;
        run += v.y;
        o.z = run;
        run += v.z;
        o.w = run;
        run += v.w;
        o4[j] = o;
        h4[j] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (t == PT_SCAN_THREADS - 1) P.ctrl[0] = inc;
    if (t < PT_RUN_SHARDS) P.ctrl[PT_CTRL_CURSOR(t)] = 0u;
}
__global__ __launch_bounds__(PT_SCAN_THREADS) void pt_bin_scan_kernel(PtPass P) { scan_body(P); }

// scatter: ray slots into bin order.  Per block tile, the slots of one bin
// take consecutive places (LDS ranks) after one global reservation.
__device__ __forceinline__ void scatter_body(const PtPass &P) {
    __shared__ uint32_t cnt[PT_BINS];
    const uint32_t n = P.n_src ? *P.n_src : P.n_src_const;
    // One contiguous run of the slots per block: count its bins in LDS,
    // reserve each bin's places with one global atomic for the whole run
    // (not one per 4096-slot tile), then read the keys again and hand out
    // the places with LDS cursors.
    const uint32_t per = ((n + gridDim.x - 1u) / gridDim.x + PT_BIN_BLOCK - 1u) & ~uint32_t(PT_BIN_BLOCK - 1);
    const uint32_t b0 = min(n, blockIdx.x * per), b1 = min(n, b0 + per);
    // (eight keys in flight per thread: the loads are issued before the LDS
    // atomics that use them)
    constexpr uint32_t U = 8u;
    hist_zero(cnt);
    for (uint32_t e0 = b0 + threadIdx.x; e0 < b1; e0 += U * PT_BIN_BLOCK) {
        uint32_t k[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            const uint32_t e = e0 + j * PT_BIN_BLOCK;
            k[j] = e < b1 ? P.key[e] : PT_BIN_NONE;
        }
#pragma unroll
        for (uint32_t j = 0; j < U; ++j)
            if (k[j] != PT_BIN_NONE) atomicAdd(&cnt[k[j]], 1u);
    }
    __syncthreads();
    for (int b = int(threadIdx.x); b < PT_BINS; b += PT_BIN_BLOCK) {
        const uint32_t c = cnt[b];
        if (c != 0u) cnt[b] = atomicAdd(&P.offs[b], c);
    }
    __syncthreads();
    for (uint32_t e0 = b0 + threadIdx.x; e0 < b1; e0 += U * PT_BIN_BLOCK) {
        uint32_t k[U];
#pragma unroll
        for (uint32_t j = 0; j < U; ++j) {
            const uint32_t e = e0 + j * PT_BIN_BLOCK;
            k[j] = e < b1 ? P.key[e] : PT_BIN_NONE;
        }
#pragma unroll
        for (uint32_t j = 0; j < U; ++j)
            if (k[j] != PT_BIN_NONE) P.idx[atomicAdd(&cnt[k[j]], 1u)] = e0 + j * PT_BIN_BLOCK;
    }
}
__global__ __launch_bounds__(PT_BIN_BLOCK) void pt_bin_scatter_kernel(PtPass P) { scatter_body(P); }

// sky (pt_set_sky): launched after a trace pass, on its
// pipeline's stream, only while a sky is set -- the scene kernels' trace and
// shade passes stay as they are, and a render without a sky pays nothing.  One
// thread per binned position of that trace pass (P as its shade pass takes
// it: rin the traced rays, n_src its count): a miss -- its hit quad (QUADS,
// taps in the shade pass) or its record's q[2] carries the traced ray's slot
// -- gathers that ray's direction, throughput and colour slot and adds
// sky_radiance(rd) * thr to the slot.  The trace pass does not carry the
// throughput, and the path's radiance lives in its colour slot (pt_binned.h),
// which every emission of the path has reached by now and the first pass's
// miss has zeroed (gen_trace).  The first pass without ray records
// (gen_norec): the position is the sample, its camera ray is made again
// (camera_ray: the same bits as the first pass's) and its throughput is 1.
// HBM-bound: 16 B read per position, 48 B gathered + 32 B of colour per miss.
template <bool QUADS>
__global__ __launch_bounds__(PT_BIN_BLOCK) void pt_bin_sky_kernel(PtPass P) {
    const PtLaunch &L = P.L;
    const uint32_t n = P.n_src ? *P.n_src : P.n_src_const;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t slot;
        if constexpr (QUADS) {
            const uint4 hq = P.hq[i];
            if (!hq_is_miss(hq)) continue;
            slot = hq_slot(hq);
        } else {
            const uint4 q2 = P.rout[i].q[2];
            if (!rec_is_miss(q2)) continue;
            slot = rec_miss_slot(q2);
        }
        pt_f3 rd, thr;
        uint32_t sid;
        if (QUADS && P.gen_norec) {
            uint32_t f, pl;
            gen_sample(uint32_t(P.frames), i, f, pl);
            int x, y;
            uint32_t rg;
            pt_f3 o;
            first_sample<PT_CAMK_ANY>(L.rank, L.nranks, L.tiles_x, L.width, L.height, L.aspect, L.fov, L.frame0,
                                      L.cam_mode, L.cam, uint32_t(P.frames), f, pl, x, y, rg, o, rd, sid);
            thr = pt_f3{1.0f, 1.0f, 1.0f};
        } else {
            const PtRay *r = P.rin + slot;
            const PathRec rec = rec_unpack(r->q[0], r->q[1], r->q[2]);
            rd = rec.rd;
            thr = rec.thr;
            sid = rec.sid;
        }
        const pt_f3 g = sky_radiance(L.sky, rd);
        float4 c = P.color[sid];
        c.x = c.x + g.x * thr.x;
        c.y = c.y + g.y * thr.y;
        c.z = c.z + g.z * thr.z;
        P.color[sid] = c;
    }
}

// fold: every pixel mixes its frames in order (test_compute.glsl:240-245).
// MOM: the fold of a path-traced, writing chunk (debug 0: the host launches
// it for nothing else) that keeps the moment image beside the accumulation
// image (pt_set_option "moments") -- each frame's colour mixed
// into the accumulation texel and its square into the moment texel.
// HBM-bound: 16 B per sample read, + 32 B per pixel for the moments.
#define PT_FOLD_SLICE 8  // frames per LDS slice of the fold
template <bool MOM>
__device__ __forceinline__ void fold_body(const PtPass &P, float *__restrict__ moments) {
    // A block folds PT_BIN_BLOCK consecutive local pixels.  Each pipeline's
    // colour region holds its frames as [pixel][frame], so the block's
    // pixels' next PT_FOLD_SLICE frames are runs of PT_FOLD_SLICE float4 per
    // pixel: the block loads them together (8 threads per 128 B run) into
    // LDS, then each thread mixes its pixel's frames in frame order.
    __shared__ float4 tile[PT_BIN_BLOCK][PT_FOLD_SLICE + 1];  // (+1: no bank conflicts between rows)
    const PtLaunch &L = P.L;
    const uint32_t t = threadIdx.x, pl0 = blockIdx.x * PT_BIN_BLOCK, pl = pl0 + t;
    const uint32_t npix = uint32_t(P.n_pix), fr = uint32_t(P.frames);
    const uint32_t nl = uint32_t(P.lanes > 0 ? P.lanes : 1);
    int x = 0, y = 0;
    bool mine = pl < npix && L.write;
    if (mine) {
        pixel_of(L, pl, x, y);
        mine = x < L.width && y < L.height;
    }
    float4 *texel = mine ? accum_texel(L, x, y) : nullptr;
    if constexpr (!MOM) {
        if (L.debug != 0) {  // direct store of the chunk's (single) frame: one pipeline, one frame
            if (mine) {
                const float4 c = P.color[pl];
                accum_store(texel, c.x, c.y, c.z);
            }
            return;
        }
    }
    float4 *mtexel = MOM && mine ? moment_texel(L, moments, texel) : nullptr;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, mr = 0.0f, mg = 0.0f, mb = 0.0f;
    if (mine) {  // (mine holds L.write; the debug views have returned)
        accum_load(texel, ar, ag, ab);
        if constexpr (MOM) accum_load(mtexel, mr, mg, mb);
    }
    uint32_t f0 = 0u;  // the chunk frame of region j's first frame
    for (uint32_t j = 0u; j < nl; ++j) {
        const uint32_t fl = fr / nl + (j < fr % nl ? 1u : 0u);
        const float4 *reg = P.color + size_t(f0) * npix;
        for (uint32_t s0 = 0u; s0 < fl; s0 += PT_FOLD_SLICE) {
            const uint32_t sn = fl - s0 < PT_FOLD_SLICE ? fl - s0 : PT_FOLD_SLICE;
            __syncthreads();  // (the previous slice's reads are done)
            for (uint32_t e = t; e < PT_BIN_BLOCK * PT_FOLD_SLICE; e += PT_BIN_BLOCK) {
                const uint32_t q = e / PT_FOLD_SLICE, k = e % PT_FOLD_SLICE;
                if (k < sn && pl0 + q < npix) tile[q][k] = reg[size_t(pl0 + q) * fl + s0 + k];
            }
            __syncthreads();
            if (mine) {
                for (uint32_t k = 0u; k < sn; ++k) {
                    const float4 c = tile[t][k];
                    const int32_t lc = int32_t(uint32_t(L.last_clear0) + f0 + s0 + k);
                    mix_frame(ar, ag, ab, pt_f3{c.x, c.y, c.z}, lc);
                    if constexpr (MOM) mix_moment(mr, mg, mb, pt_f3{c.x, c.y, c.z}, lc);
                }
            }
        }
        f0 += fl;
    }
    if (mine) {
        accum_store(texel, ar, ag, ab);
        if constexpr (MOM) accum_store(mtexel, mr, mg, mb);
    }
}
__global__ __launch_bounds__(PT_BIN_BLOCK) void pt_bin_fold_kernel(PtPass P) { fold_body<false>(P, nullptr); }
__global__ __launch_bounds__(PT_BIN_BLOCK) void pt_bin_fold_m_kernel(PtPass P, float *__restrict__ moments) {
    fold_body<true>(P, moments);
}

void pt_launch_bin(PtBinStage stage, const PtPass &P, bool stats, unsigned grid, hipStream_t stream) {
    switch (stage) {
        case PtBinStage::Gen:
            if (stats) hipLaunchKernelGGL(pt_bin_gen_kernel<true>, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P);
            else hipLaunchKernelGGL(pt_bin_gen_kernel<false>, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P);
            break;
        case PtBinStage::Shade:
            if (stats) hipLaunchKernelGGL(pt_bin_shade_kernel<true>, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P);
            else hipLaunchKernelGGL(pt_bin_shade_kernel<false>, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P);
            break;
        case PtBinStage::Scan:
            hipLaunchKernelGGL(pt_bin_scan_kernel, dim3(1), dim3(PT_SCAN_THREADS), 0, stream, P);
            break;
        case PtBinStage::Scatter:
            hipLaunchKernelGGL(pt_bin_scatter_kernel, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P);
            break;
        case PtBinStage::Trace:
            if (stats) hipLaunchKernelGGL(pt_bin_trace_kernel<true>, dim3(grid), dim3(64), 0, stream, P);
            else hipLaunchKernelGGL(pt_bin_trace_kernel<false>, dim3(grid), dim3(64), 0, stream, P);
            break;
    }
}

void pt_launch_bin_sky(const PtPass &P, bool quads, unsigned grid, hipStream_t stream) {
    if (quads) hipLaunchKernelGGL(pt_bin_sky_kernel<true>, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P);
    else hipLaunchKernelGGL(pt_bin_sky_kernel<false>, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P);
}

void pt_launch_bin_fold(const PtPass &P, float *moments, unsigned grid, hipStream_t stream) {
    if (moments) hipLaunchKernelGGL(pt_bin_fold_m_kernel, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P, moments);
    else hipLaunchKernelGGL(pt_bin_fold_kernel, dim3(grid), dim3(PT_BIN_BLOCK), 0, stream, P);
}

int pt_bin_trace_blocks_per_cu(bool stats) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, stats ? pt_bin_trace_kernel<true> : pt_bin_trace_kernel<false>,
                                                     64, 0) != hipSuccess)
        return 0;
    return n;
}
