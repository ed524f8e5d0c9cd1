// pt_bin_host.cpp -- host scheduler of the binned pipeline (pt_binned.h): the
// chunk buffers, a dispatch's plan (chunk size, lanes, kernels, grids) and
// the pass sequence of each chunk over the lanes' streams.
#include <algorithm>
#include <cstring>

#include "pt_ctx.h"

// per sample of a chunk: two ray buffers, hit quad, bin key, binned slot,
// colour (+ the high mask words and hits' high check[] words of scenes with
// > 64 entries)
constexpr size_t kBinBytesPerSample = 2 * sizeof(PtRay) + sizeof(uint4) + 2 * sizeof(uint32_t) + sizeof(float4);
constexpr size_t kBinBytesWide = sizeof(uint2) + sizeof(float4);

size_t pt_bin_bytes_per_sample(const pt_ctx *c) {
    return kBinBytesPerSample + (c->prog.n_check > 64 ? kBinBytesWide : 0);
}

static bool bin_has_wide(const BinState &b) { return b.n_lanes > 0 && b.lane[0].buf[BinState::kMaskHi].p != nullptr; }

// What the chunk buffers hold now: the wide buffers count from the first scene
// with > 64 entries on, whatever the current scene is (ensure_bin keeps them).
size_t pt_bin_bytes_held(const pt_ctx *c) {
    return c->bin.cap * size_t(c->bin.n_lanes) * (kBinBytesPerSample + (bin_has_wide(c->bin) ? kBinBytesWide : 0));
}

hipError_t EventLog::record(hipStream_t stream) {
    if (used == ev.size()) {
        hipEvent_t e;
        const hipError_t err = hipEventCreate(&e);
        if (err != hipSuccess) return err;
        ev.push_back(e);
    }
    return hipEventRecord(ev[used++], stream);
}

hipError_t EventLog::ms(double *sum) {
    *sum = 0.0;
    if (!used) return hipSuccess;
    hipError_t e = hipEventSynchronize(ev[used - 1]);
    for (size_t i = 0; e == hipSuccess && i + 1 < used; i += 2) {
        float ms = 0.0f;
        e = hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
        *sum += ms;
    }
    return e;
}

// Samples per chunk: pt_set_option "bin_samples", else automatic: 2^29 (a
// whole 256-spp 1080p render: 90 GB of HBM at 168 B per sample; every pass's
// tail is paid once per chunk, so larger chunks are faster: 64 -> 256 frames
// per chunk +5 %), at most half of the device's TOTAL memory.  The total,
// not the free memory: a torch-first process's caching allocator moves the
// free figure, and every rank of a multi-GPU run must chunk its share the
// same way whatever else it holds.  Only when the
// chunk buffers then do not fit (several contexts sharing one GPU) does the
// size fall back to half of what this context could hold -- the free
// memory plus the buffers it already owns (bin_samples_free; plan_dispatch).
// The automatic size is fixed at the context's first binned dispatch.  The
// caller's current device is left as it was.
static bool device_mem(const pt_ctx *c, size_t &free_b, size_t &total_b) {
    free_b = total_b = 0;
    int prev = -1;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    const bool ok = hipSetDevice(c->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
                    total_b != 0;
    if (have_prev) (void)hipSetDevice(prev);
    return ok;
}

size_t pt_bin_samples(pt_ctx *c) {
    if (c->bin.samples > 0) return size_t(c->bin.samples);
    if (c->bin.auto_samples) return c->bin.auto_samples;
    size_t free_b = 0, total_b = 0;
    if (!device_mem(c, free_b, total_b)) return size_t(1) << 27;
    const size_t cap = std::max<size_t>(size_t(1) << 20, total_b / 2 / pt_bin_bytes_per_sample(c));
    return std::min<size_t>(size_t(1) << 29, cap);
}

namespace {

// The fallback when pt_bin_samples()'s chunk buffers did not fit: half of the
// free memory plus what this context holds (other contexts' allocations
// count as used, so ranks sharing one GPU each size to what is left).
size_t bin_samples_free(pt_ctx *c) {
    const size_t per = pt_bin_bytes_per_sample(c);
    size_t free_b = 0, total_b = 0;
    if (!device_mem(c, free_b, total_b)) return size_t(1) << 27;
    const size_t held = pt_bin_bytes_held(c);
    const size_t cap = std::max<size_t>(size_t(1) << 20, (free_b + held) / 2 / per);
    return std::min<size_t>(size_t(1) << 29, cap);
}

void free_bin(BinState &b) {
    for (BinState::Lane &l : b.lane)
        for (DevBuf &buf : l.buf) buf.release();
    b.color.release();
    b.btab.release();
    b.n_lanes = 0;
    b.cap = b.ctrl_words = 0;
    // nothing has written the next table yet: bin_sets / bin_overflow read -1
    // until a dispatch of the matching kind has run on it (pt_options.cpp read_btab)
    b.btab_used = b.btab_counted = false;
}

// ensure_bin's result when the buffers' allocation itself failed (out of
// device memory): the one failure plan_dispatch may answer with a smaller
// chunk.  Any other HIP error (e.g. an earlier kernel's fault reported by the
// synchronisation) keeps its message and ends the dispatch.
constexpr int kBinNoMemory = -1000;

// Buffers for `lanes` pipelines of `samples` samples each.
int ensure_bin(pt_ctx *c, size_t samples, size_t passes, int lanes) {
    BinState &b = c->bin;
    const size_t words = size_t(PT_CTRL_STRIDE) * (passes + 1);
    // (mask_hi, check[] bits 64..127, exists from the first scene with > 64 entries on: like cap
    // and lanes it only grows, so a reallocation never holds less than the one before)
    const bool wide = c->prog.n_check > 64 || bin_has_wide(b);
    const bool hi_ok = !wide || bin_has_wide(b);
    if (samples <= b.cap && words <= b.ctrl_words && lanes <= b.n_lanes && hi_ok) return PT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // lane 1 joins lane 0's stream before every dispatch ends
    samples = std::max(samples, b.cap);
    lanes = std::max(lanes, b.n_lanes);
    free_bin(b);
    // a lane's buffers in bytes, by BinState::LaneBuf (0: not allocated)
    const size_t bytes[BinState::kLaneBufs] = {
        samples * sizeof(PtRay),    samples * sizeof(PtRay),    samples * sizeof(uint4),
        wide ? samples * sizeof(uint2) : 0, samples * sizeof(uint32_t), samples * sizeof(uint32_t),
        wide ? samples * sizeof(float4) : 0, PT_BINS * sizeof(uint32_t), PT_BINS * sizeof(uint32_t),
        words * sizeof(uint32_t)};
    bool ok = b.color.alloc(size_t(lanes) * samples * sizeof(float4)) == hipSuccess &&
              b.btab.alloc((PT_BINS + 1) * sizeof(unsigned long long)) == hipSuccess;  // (+ overflow count)
    for (int i = 0; ok && i < lanes; ++i)
        for (int k = 0; ok && k < BinState::kLaneBufs; ++k)
            ok = !bytes[k] || b.lane[i].buf[k].alloc(bytes[k]) == hipSuccess;
    if (!ok) {
        free_bin(b);
        (void)hipGetLastError();
        fail(c, PT_ERR_HIP, "out of device memory for the binned pipeline");
        return kBinNoMemory;
    }
    if (!b.fork_ev) HIPCHK(c, hipEventCreateWithFlags(&b.fork_ev, hipEventDisableTiming));
    b.lane[0].stream = c->stream;
    for (int i = 1; i < lanes; ++i) {
        if (!b.xstream[i]) HIPCHK(c, hipStreamCreateWithFlags(&b.xstream[i], hipStreamNonBlocking));
        if (!b.join_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&b.join_ev[i], hipEventDisableTiming));
        b.lane[i].stream = b.xstream[i];
    }
    for (int i = 0; i < lanes; ++i) {
        HIPCHK(c, hipMemsetAsync(b.lane[i].buf[BinState::kHist].p, 0, PT_BINS * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(b.lane[i].buf[BinState::kCtrl].p, 0, words * sizeof(uint32_t), c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.n_lanes = lanes;
    b.cap = samples;
    b.ctrl_words = words;
    if (!b.cu_count) HIPCHK(c, hipDeviceGetAttribute(&b.cu_count, hipDeviceAttributeMultiprocessorCount, c->device));
    return PT_OK;
}

#ifndef PT_SCATTER_ITEMS  // slots per thread of a scatter tile (BinPlan::scatter_grid; an A/B build may set it)
#define PT_SCATTER_ITEMS 16
#endif

// What every chunk of one dispatch shares.
struct BinPlan {
    uint32_t n_pix = 0, spp = 0, F = 0;  // (F: frames per chunk)
    int32_t frame0 = 0, lc0 = 0;
    int passes = 0, lanes = 0;
    bool stats = false, posed = false;
    bool use_table = false;   // bins from the table of check[] sets
    bool taps_shade = false;  // normal taps in the shade pass: march-only trace + tapping shade (scene kernels)
    float *moments = nullptr;  // the fold also keeps the moment image (pt_set_option "moments")
    const PtJitModule *jm = nullptr;
    hipFunction_t trace = nullptr, trace_first = nullptr;
    unsigned cu = 1, trace_grid = 1, trace_g_grid = 1, shade_grid = 1;

    // the stage's scene kernel (nullptr: the ahead-of-time one)
    hipFunction_t fn(PtJitStage stage, bool gen_norec = false) const {
        return jm ? pt_jit_select(*jm, stage, stats, posed, taps_shade, gen_norec) : nullptr;
    }
    unsigned item_grid(size_t n) const {
        return unsigned(std::max<size_t>(1, std::min<size_t>((n + PT_BIN_BLOCK - 1) / PT_BIN_BLOCK, 4 * cu)));
    }
    // scatter: 4 blocks per CU (8 / 16 measured equal), each one contiguous
    // run of PT_SCATTER_ITEMS-slot tiles
    unsigned scatter_grid(size_t n) const {
        const size_t tile = PT_BIN_BLOCK * PT_SCATTER_ITEMS;
        return unsigned(std::max<size_t>(1, std::min<size_t>((n + tile - 1) / tile, size_t(4) * cu)));
    }
};

// Trace blocks per CU from a kernel's occupancy: leave one wave slot per SIMD
// (4 per CU) to the other pipeline, so its shade / scatter / scan blocks run
// beside the persistent trace waves instead of waiting for a pass to drain:
// 28 of 32 with the 64-VGPR (8-wave) build (+1.5 % over 24 of 28 at 72 VGPRs),
// 24 of 28 with the 72-VGPR fallback (+1.5 % over 28 of 28)
int trace_blocks_per_cu(int occupancy) { return occupancy > 8 ? std::min(occupancy - 4, 28) : occupancy; }

// Size the chunks (frames are processed in chunks of at most pt_bin_samples()
// samples), make sure their buffers exist, and pick the kernels and grids.
int plan_dispatch(pt_ctx *c, const PtLaunch &L, bool stats, BinPlan &p) {
    BinState &b = c->bin;
    p.stats = stats;
    p.n_pix = uint32_t(L.n_tiles) * 64u;
    p.frame0 = L.frame0;
    p.lc0 = L.last_clear0;
    p.spp = uint32_t(L.spp);
    if (L.debug != 0) {  // direct stores: only the last frame survives (as the other kernels)
        p.frame0 = int32_t(uint32_t(p.frame0) + p.spp - 1);
        p.lc0 = int32_t(uint32_t(p.lc0) + p.spp - 1);
        p.spp = 1;
    }
    if (!b.samples && !b.auto_samples) b.auto_samples = pt_bin_samples(c);  // (fixed from now on)
    p.passes = L.bounces + 1;
    auto ensure_chunk = [&]() {
        p.F = uint32_t(std::max<size_t>(1, std::min<size_t>(p.spp, pt_bin_samples(c) / p.n_pix)));
        p.lanes = int(std::min<uint32_t>(uint32_t(b.lanes), p.F));
        const uint32_t per_lane = (p.F + uint32_t(p.lanes) - 1) / uint32_t(p.lanes);  // frames per lane
        return ensure_bin(c, size_t(p.n_pix) * per_lane, size_t(p.passes), p.lanes);
    };
    int rc = ensure_chunk();
    if (rc == kBinNoMemory && !b.samples && !b.fallback) {
        // the total-memory size does not fit (contexts sharing the GPU):
        // size to the free memory once, fixed from now on
        b.fallback = true;
        b.auto_samples = bin_samples_free(c);
        c->err.clear();
        rc = ensure_chunk();
    }
    if (rc == kBinNoMemory) rc = PT_ERR_HIP;  // (the message is in c->err)
    if (rc != PT_OK) return rc;
    if (!stats) b.last_chunks = (p.spp + p.F - 1) / p.F;
    p.cu = unsigned(std::max(1, b.cu_count));
    p.jm = pt_jit_active(c->jit);
    p.use_table = b.table && c->prog.n_check > uint32_t(PT_BIN_BITS) && c->prog.n_check <= 64;
    p.taps_shade = p.jm && b.shade_taps;
    // (a posed camera, pt_set_camera, takes the builds made for it: pt_host.h)
    p.posed = L.cam_mode != PT_CAM_DEFAULT;
    p.trace = p.fn(PtJitStage::Trace);
    p.trace_first = p.fn(PtJitStage::TraceFirst);
    int per_cu = 0;
    if (p.jm) HIPCHK(c, hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, p.trace, 64, 0));
    else per_cu = pt_bin_trace_blocks_per_cu(stats);
    per_cu = trace_blocks_per_cu(per_cu);
    p.trace_grid = p.trace_g_grid = p.cu * unsigned(std::max(1, per_cu));
    // the first pass's kernel may have been rebuilt at 7 waves on its own
    // (pt_jit_compile_source): the same rule on its occupancy
    if (p.trace_first) {
        int g = 0;
        HIPCHK(c, hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&g, p.trace_first, 64, 0));
        g = trace_blocks_per_cu(g);
        if (g > 0 && g < per_cu) p.trace_g_grid = p.cu * unsigned(g);
    }
    // two rounds of the tapping shade kernel's 7 resident blocks per CU
    // (measured +2 % over 8, whose last round ran on a quarter of the chip;
    // 8 / 16 at 8 waves -0.3 %); 8 for the table kernel
    const unsigned shade_cu = p.taps_shade ? 14u : 8u;
    p.shade_grid = unsigned(
        std::max<size_t>(1, std::min<size_t>((b.cap + PT_BIN_BLOCK - 1) / PT_BIN_BLOCK, size_t(shade_cu) * p.cu)));
    return PT_OK;
}

// One kernel of the pass sequence: the scene kernel f, else (nullptr) the
// ahead-of-time kernel of `aot`.
int launch_stage(pt_ctx *c, hipFunction_t f, PtBinStage aot, PtPass &P, bool stats, unsigned grid, unsigned block,
                 hipStream_t stream) {
    if (f) {
        void *args[] = {&P};
        HIPCHK(c, hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, 0, stream, args, nullptr));
    } else {
        pt_launch_bin(aot, P, stats, grid, stream);
        HIPCHK(c, hipGetLastError());
    }
    return PT_OK;
}

// Lane i's pass record for `frames` frames from frame offset `first` of the
// chunk that starts at frame `done` of the dispatch; its colours land in the
// chunk's colour buffer at that offset, so one fold mixes all lanes in frame order.
PtPass make_pass(const pt_ctx *c, const BinPlan &pl, const PtLaunch &L, int i, uint32_t done, uint32_t first,
                 uint32_t frames, unsigned long long *btab) {
    const BinState::Lane &l = c->bin.lane[i];
    PtPass p;
    std::memset(&p, 0, sizeof p);
    p.L = L;
    p.L.frame0 = int32_t(uint32_t(pl.frame0) + done + first);
    p.L.last_clear0 = int32_t(uint32_t(pl.lc0) + done + first);
    p.L.spp = int32_t(frames);
    p.rin = l.ray(0);
    p.rout = l.ray(1);
    p.hq = l.buf[BinState::kHq].as<uint4>();
    p.mask_hi = l.buf[BinState::kMaskHi].as<uint2>();
    p.key = l.buf[BinState::kKey].as<uint32_t>();
    p.idx = l.buf[BinState::kIdx].as<uint32_t>();
    p.hist = l.buf[BinState::kHist].as<uint32_t>();
    p.offs = l.buf[BinState::kOffs].as<uint32_t>();
    p.color = c->bin.color.as<float4>() + size_t(first) * pl.n_pix;
    p.hitn = l.buf[BinState::kHitn].as<float4>();
    p.ctrl = l.ctrl(0);
    p.n_src_const = uint32_t(size_t(pl.n_pix) * frames);
    p.n_pix = int32_t(pl.n_pix);
    p.frames = int32_t(frames);
    p.wide = c->prog.n_check > 64 ? 1 : 0;
    p.btab = btab;
    p.count_overflow = pl.stats ? 1 : 0;
    // trace runs of at most 512 rays (256 / 768 / 1024 equal, 128 -7 %), a
    // refill once 2 lanes are free (1 / 4 equal)
    p.run_max = 512;
    p.refill_min = 2;
    return p;
}

// Shade the hits of lane i's trace pass k (its hit quads and the rays it traced,
// ray[k & 1]; or, taps in the trace pass, its hit records in
// ray[(k + 1) & 1]): ended paths store their colour, the rest get
// their next ray in ray[(k + 1) & 1], bounds() and bin
int shade_pass(pt_ctx *c, const BinPlan &pl, const PtPass &P, int i, int k) {
    const BinState::Lane &l = c->bin.lane[i];
    PtPass S = P;
    S.bounce = k;
    S.rin = l.ray(k);
    S.rout = l.ray(k + 1);
    S.n_src = l.ctrl(size_t(k));
    if (!pl.stats) HIPCHK(c, c->bin.slog.record(l.stream));
    const int rc = launch_stage(c, pl.fn(PtJitStage::Shade, S.gen_norec != 0), PtBinStage::Shade, S, pl.stats,
                                pl.shade_grid, PT_BIN_BLOCK, l.stream);
    if (rc != PT_OK) return rc;
    if (!pl.stats) HIPCHK(c, c->bin.slog.record(l.stream));
    return PT_OK;
}

// Lane i's pass k: shade the hits of pass k-1, bin the rays of ray[k & 1]
// (gen's, or those shaded hits' next rays), trace them into the other buffer,
// and give the misses the sky.
int trace_pass(pt_ctx *c, const BinPlan &pl, PtPass &p, int i, int k) {
    BinState &b = c->bin;
    const BinState::Lane &l = b.lane[i];
    int rc;
    if (k > 0 && (rc = shade_pass(c, pl, p, i, k - 1)) != PT_OK) return rc;
    const bool first = k == 0 && p.gen_trace;
    if (k > 0) p.gen_trace = p.gen_norec = 0;  // (shade pass 0 above still had them)
    p.bounce = k;
    p.rin = l.ray(k);
    p.rout = l.ray(k + 1);
    p.ctrl = l.ctrl(size_t(k));
    p.n_src = k == 0 ? nullptr : l.ctrl(size_t(k - 1));
    if (k > 0 || !p.gen_order) {
        pt_launch_bin(PtBinStage::Scan, p, pl.stats, 1, l.stream);
        pt_launch_bin(PtBinStage::Scatter, p, pl.stats, pl.scatter_grid(k == 0 ? p.n_src_const : b.cap), l.stream);
        HIPCHK(c, hipGetLastError());
    }
    if (!pl.stats) HIPCHK(c, b.tlog.record(l.stream));
    if ((rc = launch_stage(c, first ? pl.trace_first : pl.trace, PtBinStage::Trace, p, pl.stats,
                           first ? pl.trace_g_grid : pl.trace_grid, 64, l.stream)) != PT_OK)
        return rc;
    if (!pl.stats) HIPCHK(c, b.tlog.record(l.stream));
    // a sky (pt_set_sky): the misses of this trace pass take its radiance, before the
    // shade pass of its hits (no sky, no launch; the instrumented run counts no work of
    // this pass and writes no image, so it leaves the pass out)
    if (p.L.sky_mode != PT_SKY_OFF && !pl.stats) {
        PtPass K = p;
        K.n_src = p.ctrl;  // this trace pass's ray count
        HIPCHK(c, b.klog.record(l.stream));
        pt_launch_bin_sky(K, pl.taps_shade, pl.item_grid(k == 0 ? size_t(p.n_src_const) : b.cap), l.stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, b.klog.record(l.stream));
    }
    return PT_OK;
}

// No gen pass: the first trace pass makes its windows' camera rays itself
// (scene kernels, generation order: +2.8 %); otherwise the scene's gen kernel
// (straight-line bounds(): +1.4 % over the ahead-of-time one)
int gen_pass(pt_ctx *c, const BinPlan &pl, PtPass &p, int i) {
    BinState &b = c->bin;
    if (p.gen_order && pl.taps_shade && !pl.stats && pl.trace_first) {
        p.gen_trace = 1;
        p.gen_norec = c->prog.n_check <= 32 ? 1 : 0;  // (the check[] bits ride in the hit quad)
        b.gen_trace_used = 1;
        b.gen_norec_used = p.gen_norec;
        return PT_OK;
    }
    return launch_stage(c, pl.fn(PtJitStage::Gen), PtBinStage::Gen, p, pl.stats, pl.item_grid(size_t(p.n_src_const)),
                        PT_BIN_BLOCK, b.lane[i].stream);
}

// Encode the chunk of `fr` frames that starts at frame `done`: fork the
// lanes, gen (or not), the trace / shade passes lane by lane, join, fold.
int encode_chunk(pt_ctx *c, const BinPlan &pl, const PtLaunch &L, uint32_t done, uint32_t fr) {
    BinState &b = c->bin;
    const int nl = int(std::min<uint32_t>(uint32_t(pl.lanes), fr));
    // the table of check[] sets starts empty per chunk (bin_resolve: only
    // scenes whose sets do not fit the bin index use it)
    unsigned long long *btab = nullptr;
    if (pl.use_table) {
        btab = b.btab.as<unsigned long long>();
        HIPCHK(c, hipMemsetAsync(btab, 0, PT_BINS * sizeof(unsigned long long), c->stream));
    }
    // the chunk's frames over the lanes: lane i renders fr / nl frames (the
    // first fr % nl lanes one more) from the frame offset where lane i-1 ended
    PtPass P[BinState::kMaxLanes];
    for (uint32_t i = 0, first = 0; i < uint32_t(nl); ++i) {
        const uint32_t frames = fr / uint32_t(nl) + (i < fr % uint32_t(nl) ? 1u : 0u);
        P[i] = make_pass(c, pl, L, int(i), done, first, frames, btab);
        first += frames;
    }
    if (nl > 1) {  // lanes 1.. start after everything enqueued on the context stream so far
        HIPCHK(c, hipEventRecord(b.fork_ev, c->stream));
        for (int i = 1; i < nl; ++i) HIPCHK(c, hipStreamWaitEvent(b.lane[i].stream, b.fork_ev, 0));
    }
    // the first pass takes the primary rays in generation order (gen lists
    // them, the host sets the count; no histogram, scan or scatter: +1 %)
    // -- only when every local tile lies inside the image: then every
    // generated slot is live and the list is the identity order
    const bool full_tiles = L.width % PT_TILE == 0 && L.height % PT_TILE == 0 && L.debug == 0;
    for (int i = 0; i < nl && full_tiles; ++i) {
        P[i].gen_order = 1;
        // pass 0's control words = {count, run cursors 0}: stream-ordered
        // fills, no host buffer whose lifetime the copy would have to outlast
        const hipDeviceptr_t ctrl = reinterpret_cast<hipDeviceptr_t>(b.lane[i].ctrl(0));
        HIPCHK(c, hipMemsetD32Async(ctrl, 0, PT_CTRL_STRIDE, b.lane[i].stream));
        HIPCHK(c, hipMemsetD32Async(ctrl, int(P[i].n_src_const), 1, b.lane[i].stream));
    }
    int rc;
    if (!pl.stats) b.gen_trace_used = b.gen_norec_used = 0;
    for (int i = 0; i < nl; ++i)
        if ((rc = gen_pass(c, pl, P[i], i)) != PT_OK) return rc;
    for (int k = 0; k < pl.passes; ++k)
        for (int i = 0; i < nl; ++i)
            if ((rc = trace_pass(c, pl, P[i], i, k)) != PT_OK) return rc;
    for (int i = 0; i < nl; ++i)  // the last bounce's hits end their paths
        if ((rc = shade_pass(c, pl, P[i], i, pl.passes - 1)) != PT_OK) return rc;
    for (int i = 1; i < nl; ++i) {  // the fold (and everything after) waits for every lane
        HIPCHK(c, hipEventRecord(b.join_ev[i], b.lane[i].stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, b.join_ev[i], 0));
    }
    PtPass Fp = P[0];
    Fp.L.frame0 = int32_t(uint32_t(pl.frame0) + done);
    Fp.L.last_clear0 = int32_t(uint32_t(pl.lc0) + done);
    Fp.L.spp = int32_t(fr);
    Fp.color = b.color.as<float4>();
    Fp.frames = int32_t(fr);
    Fp.lanes = nl;  // (the colour regions' split: pt_bin_kernels.hip fold_body)
    pt_launch_bin_fold(Fp, pl.moments, unsigned((pl.n_pix + PT_BIN_BLOCK - 1) / PT_BIN_BLOCK), c->stream);
    HIPCHK(c, hipGetLastError());
    return PT_OK;
}

}  // namespace

// One dispatch through the pass pipeline, chunk by chunk.
int pt_launch_binned(pt_ctx *c, PtLaunch &L, bool stats, float *moments) {
    BinState &b = c->bin;
    BinPlan pl;
    int rc = plan_dispatch(c, L, stats, pl);
    if (rc != PT_OK) return rc;
    pl.moments = moments;
    // the set table's overflow count covers the whole dispatch (the table
    // itself is cleared per chunk)
    if (pl.use_table && stats)
        HIPCHK(c, hipMemsetAsync(b.btab.as<unsigned long long>() + PT_BINS, 0, sizeof(unsigned long long), c->stream));
    if (!stats) b.btab_used = pl.use_table;
    if (stats) b.btab_counted = pl.use_table;
    for (uint32_t done = 0; done < pl.spp; done += pl.F)
        if ((rc = encode_chunk(c, pl, L, done, std::min(pl.F, pl.spp - done))) != PT_OK) return rc;
    return PT_OK;
}
