// pt_ctx.h -- the context behind the C ABI (include/pt_abi.h) and the small
// helpers its host files share: pt_runtime.hip (the entry points of the
// context and the scene), pt_post_host.cpp (the image-space entry points),
// pt_bin_host.cpp (the binned scheduler) and pt_options.cpp (the option table).
// Host only: no device header and no hipRTC source includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/pt_abi.h"
#include "pt_host.h"

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// An owning device allocation with its capacity.  Freed by release() or with
// the context (pt_destroy makes the context's device current first).
struct DevBuf : NoCopy {
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t alloc(size_t bytes) {  // exactly `bytes`, whatever was held before
        release();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

// One timed section of a stream: begin() ... end(), then ms().  The event
// pair is created on first use.
struct TimedSection : NoCopy {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;  // an end() has been recorded
    ~TimedSection() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t begin(hipStream_t s) {
        hipError_t err = hipSuccess;
        for (hipEvent_t &e : ev)
            if (!e && err == hipSuccess) err = hipEventCreate(&e);
        return err != hipSuccess ? err : hipEventRecord(ev[0], s);
    }
    hipError_t end(hipStream_t s) {
        const hipError_t err = hipEventRecord(ev[1], s);
        timed = timed || err == hipSuccess;
        return err;
    }
    // 0 before the first section; sync: wait for the end event first (the
    // section's stream was not synchronised since)
    hipError_t ms(float *out, bool sync) const {
        *out = 0.0f;
        if (!timed) return hipSuccess;
        const hipError_t err = sync ? hipEventSynchronize(ev[1]) : hipSuccess;
        return err != hipSuccess ? err : hipEventElapsedTime(out, ev[0], ev[1]);
    }
};

// HIP event pairs around a dispatch's launches of one kind (on each
// pipeline's stream): their summed device time per kernel
struct EventLog : NoCopy {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    ~EventLog() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    hipError_t record(hipStream_t stream);
    hipError_t ms(double *sum);  // summed elapsed time of the (start, end) pairs; blocks for the last
};

// the reference's fixed view as a pt_camera (what pt_get_camera reports for it)
static const pt_camera kDefaultCamera = {{0.0f, 0.0f, -3.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f},
                                         {0.0f, 0.0f, 1.0f}, 0.0f, 1.0f};

// Binned pipeline state (pt_binned.h, pt_bin_host.cpp).  A chunk's frames are
// split over up to kMaxLanes independent pipelines ("lanes"), each on its own
// stream, so one lane's memory-bound passes (shade, gen, scatter) run beside
// another's VALU-bound trace pass and fill its tail.  `cap` samples per lane;
// the colour buffer holds the whole chunk.
struct BinState {
    static constexpr int kMaxLanes = 4;
    // a lane's buffers, in allocation order.  Ray0/1 ping-pong: pass k traces ray[k & 1], its shade pass writes
    // the other; Hq: trace -> shade, the hit quads (taps in the shade pass); MaskHi: check[] bits 64..127 and
    // Hitn: trace -> shade, normal differences per position (both only for scenes with > 64 entries)
    enum LaneBuf { kRay0, kRay1, kHq, kMaskHi, kKey, kIdx, kHitn, kHist, kOffs, kCtrl, kLaneBufs };
    struct Lane {
        DevBuf buf[kLaneBufs];
        hipStream_t stream = nullptr;
        PtRay *ray(int k) const { return buf[kRay0 + (k & 1)].as<PtRay>(); }
        uint32_t *ctrl(size_t pass) const { return buf[kCtrl].as<uint32_t>() + size_t(PT_CTRL_STRIDE) * pass; }
    };
    Lane lane[kMaxLanes];
    int n_lanes = 0;  // lanes allocated
    DevBuf color;     // float4 per sample of a chunk
    DevBuf btab;      // the table of check[] sets, [PT_BINS] + overflow count (pt_binned.h bin_probe / bin_resolve), shared by the lanes
    size_t cap = 0, ctrl_words = 0;
    hipStream_t xstream[kMaxLanes] = {};  // lanes 1.. streams (created on first use; lane 0 = the context's)
    hipEvent_t fork_ev = nullptr, join_ev[kMaxLanes] = {};
    int cu_count = 0;
    // options (pt_set_option)
    int samples = 0;     // "bin_samples": samples per chunk; 0 = automatic (pt_bin_samples())
    int lanes = 2;       // "bin_lanes" (2: +6 % over 1; 3-4 equal or worse)
    int table = 1;       // "bin_table": bins from the table of check[] sets
    int shade_taps = 1;  // "shade_taps": normal taps in the shade pass
    // chunk sizing
    size_t auto_samples = 0;  // the automatic chunk size, fixed at the first binned dispatch
    bool fallback = false;    // auto_samples came from the free memory (the total-memory size did not fit)
    // what the last dispatch used
    uint32_t last_chunks = 0;    // chunks of the last timed binned dispatch
    int gen_trace_used = 0;      // the last timed dispatch's first pass made its own camera rays
    int gen_norec_used = 0;      // ... and stored no ray records (shade pass 0 made them again)
    bool btab_used = false;      // the last timed binned dispatch binned by the table of check[] sets
    bool btab_counted = false;   // the last instrumented one did, and counted its overflows
    EventLog tlog, slog, klog;   // its trace / shade / sky passes (pt_set_sky)
    ~BinState() {
        for (int i = 1; i < kMaxLanes; ++i) {
            if (xstream[i]) (void)hipStreamDestroy(xstream[i]);
            if (join_ev[i]) (void)hipEventDestroy(join_ev[i]);
        }
        if (fork_ev) (void)hipEventDestroy(fork_ev);
    }
};

struct pt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    TimedSection dispatch_time;  // pt_last_dispatch_ms
    // options (pt_set_option)
    int kernel = PT_KERNEL_AUTO;  // PT_KERNEL_*
    int shade_batch = 16;         // state-machine kernels: lanes waiting before a shading pass (measured best)
    struct Image {
        uint32_t width = 0, height = 0;
        DevBuf accum, reduced;
        DevBuf display;  // display pass output (device) and its timing
        TimedSection display_time;
        size_t bytes(size_t texel = 16) const { return size_t(width) * height * texel; }
    } img;
    struct Program {
        std::vector<pt_op> ops;
        std::vector<pt_aabb> aabbs;
        uint32_t n_check = 1;
        bool have_program = false, have_data = false;
        DevBuf nodes, boxes, mats;  // device tables (PtNode, PtAabb, PtMat)
        bool fast_bounds = false;   // every box coordinate inside the reciprocal-division guard
        float bound_k = 0.0f;       // pt_bound_k of the uploaded scene (NaN: no map() bound)
        DevBuf stats;               // 2 x PT_ST_COUNT (second half: the shade pass's normal taps)
        unsigned long long tap_stats[PT_ST_COUNT] = {};  // last pt_dispatch_stats: the shade-pass taps' share
        std::vector<PtNode> host_nodes;  // the uploaded tables, kept for the probe modules' source (pt_probe_source)
        std::vector<PtAabb> host_boxes;
    } prog;
    struct View {
        // camera (pt_set_camera); cam_mode PT_CAM_DEFAULT: the reference's fixed view
        int cam_mode = PT_CAM_DEFAULT;
        pt_camera cam = kDefaultCamera;
        // sky (pt_set_sky); sky_mode PT_SKY_OFF: the reference's void
        int sky_mode = PT_SKY_OFF;
        pt_sky sky = {};
        uint32_t rank = 0, nranks = 1;  // tiles
    } view;
    PtJitState jit;
    BinState bin;
    // denoiser (pt_render_guides / pt_denoise): the guide planes g0 = {n, t} and
    // g1 = {albedo, hit} (16 B/px each), the filter's two ping-pong images
    // (16 B/px each), grown on first use; the timing of their kernels
    struct Denoiser {
        DevBuf guides[2], filter[2];
        bool guides_valid = false;
        int lds = 1;  // pt_set_option "denoise_lds": LDS-staged taps at steps 1 and 2 (-19 % on five iterations: EXPERIMENTS.md)
        TimedSection guide_time, denoise_time;
        // the view the guides were rendered with (pt_temporal_accumulate projects through it): a lens as its pinhole
        int guide_cam_mode = PT_CAM_DEFAULT;
        pt_camera guide_cam = kDefaultCamera;
        float guide_aspect = 1.0f, guide_fov = 1.0f;
    } dn;
    // temporal accumulation (pt_temporal_accumulate): two sets of history images -- colour and
    // second moment (16 B/px each), sample count (4 B/px), a copy of the guide planes (16 B/px each) -- of which
    // set[cur] is the history and the other the next accumulate's target, allocated at the first accumulate; the
    // view the history is seen from; the accumulates since it was last dropped; the timing of its kernels
    struct History {
        struct Set {
            DevBuf h, hm, hn, g0, g1;
        } set[2];
        int cur = 0;
        bool valid = false;
        uint32_t views = 0;
        int cam_mode = PT_CAM_DEFAULT;
        pt_camera cam = kDefaultCamera;
        float aspect = 1.0f, fov = 1.0f;
        TimedSection accumulate_time, variance_time, denoise_time;
        void drop() {
            valid = false;
            views = 0;
        }
    } hist;
    // second moments (pt_set_option "moments"): the image M of each frame's squared colour,
    // mixed as the accumulation image is (16 B/px, held while the option is on); whether it and the
    // accumulation image are one render's, and of how many frames; the variance plane's two ping-pong
    // buffers (4 B/px each, grown on first use); the timing of the variance kernel and of the guided filter
    struct Moments {
        int on = 0;
        DevBuf img;
        bool valid = false;
        uint32_t frames = 0;
        DevBuf var[2];
        TimedSection variance_time, guided_time;
    } mom;
    // mesh export (pt_sample_field / pt_mesh_extract, pt_mesh_host.cpp): the extractor's
    // working memory -- per brick: flag, slot, list; per evaluated brick: corner lattice, masks, counts and
    // bases; per vertex: its cell; the counters -- and the last mesh, all grown on first use; the timing of the stages' kernels
    struct Mesher {
        DevBuf flag, slot, list, lattice, vmask, qmask, nv, nt, vbase, tbase, ctr, vcell;
        DevBuf pos, nrm, shp, tri;       // the snapshot pt_mesh_read returns
        DevBuf sample_xyz, sample_d, sample_shape;  // pt_sample_field's staging
        bool have = false;               // a pt_mesh_extract succeeded
        size_t n_vertices = 0, n_triangles = 0;
        int skip = 1;  // pt_set_option "mesh_skip": 1 skips bricks by their centre value, 0 evaluates every brick
        enum Stage { kSkip, kClassify, kScan, kEmit, kStages };
        TimedSection stage_time[kStages], sample_time;
        size_t bytes() const {
            size_t n = 0;
            for (const DevBuf *b : {&flag, &slot, &list, &lattice, &vmask, &qmask, &nv, &nt, &vbase, &tbase, &ctr, &vcell, &pos,
                                    &nrm, &shp, &tri})
                n += b->cap;
            return n;
        }
    } mesh;
    // ray queries (pt_trace_rays / pt_pick_pixels): the staging of a call's rays or pixel list
    // and of its answers, grown on first use; the timing of each entry point's kernel
    struct Rays {
        DevBuf ro, rd, xy, t, shape, normal;
        TimedSection rays_time, pick_time;
    } rays;
    // radiance queries (pt_trace_radiance): the staging of a call's rays and of their running mean
    // and moment (12 B per ray each), and a chunk's shared first hits (32 B per ray) and colours (16 B per sample, at
    // most `samples` of them in flight), grown on first use; the summed device time of the last call's kernels (a
    // pair of events per chunk) and of its first-segment kernels alone
    struct Radiance {
        DevBuf ro, rd, mean, moment, first, colour;
        int samples = 1 << 22;  // pt_set_option "radiance_samples"
        EventLog klog, flog;
        size_t bytes() const { return ro.cap + rd.cap + mean.cap + moment.cap + first.cap + colour.cap; }
    } rad;
    // preview shading (pt_render_preview): its own image, 16 B per pixel, grown on first use, and
    // the timing of its kernel
    struct Preview {
        DevBuf img;
        TimedSection time;
    } preview;
    // the probes (pt_probe_map / pt_probe_taps / pt_probe_bounds, pt_map_probe.hip): the probe
    // modules loaded so far by their generated source, how many were compiled and in how many seconds, and the
    // staging of a call's inputs and outputs, grown on first use
    struct Probe {
        enum Buf { kXyz, kRd, kCheck, kBnd, kLiveIn, kD, kShape, kLiveOut, kMask, kSkip, kBufs };
        std::map<std::string, PtProbeModule> mods;
        int compiles = 0;
        double seconds = 0.0;
        DevBuf buf[kBufs];
    } probe;
    struct Comm {
        ncclComm_t comm = nullptr;
        uint32_t nranks = 0;
    } comm;
};

inline int fail(pt_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctx, PT_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_));     \
    } while (0)

// Grow b to at least `need` bytes (at least 1; the image sites ask for 16).
inline int ensure(pt_ctx *c, DevBuf &b, size_t need) {
    void **ptr = &b.p;
    size_t &cap = b.cap;
    if (need <= cap && *ptr) return PT_OK;
    if (*ptr) HIPCHK(c, hipFree(*ptr));
    *ptr = nullptr;
    size_t bytes = std::max<size_t>(need, 1);
    HIPCHK(c, hipMalloc(ptr, bytes));
    cap = bytes;
    return PT_OK;
}

// The tail of an image readback: `need` bytes to the host on the context's
// stream, then wait.  too_small: the site's message for a missing or short
// host buffer (nullptr: the site checked already).
inline int read_back(pt_ctx *c, void *out, size_t bytes, const void *src, size_t need, const char *too_small) {
    if (too_small && (!out || bytes < need)) return fail(c, PT_ERR_SIZE, too_small);
    HIPCHK(c, hipSetDevice(c->device));
    if (need) HIPCHK(c, hipMemcpyAsync(out, src, need, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

// pt_bin_host.cpp: the binned pipeline's scheduler
size_t pt_bin_bytes_per_sample(const pt_ctx *c);  // of the current scene (chunk sizing)
size_t pt_bin_bytes_held(const pt_ctx *c);         // the chunk buffers as allocated ("bin_bytes")
size_t pt_bin_samples(pt_ctx *c);  // samples per chunk: the option, else the automatic size
// moments: the moment image the folds keep beside the accumulation image (nullptr: the plain fold)
int pt_launch_binned(pt_ctx *c, PtLaunch &L, bool stats, float *moments);
// pt_runtime.hip: the moment image sized to the accumulation image and zeroed while the option is on, and not
// valid (the option's setter, pt_resize_clear, pt_set_tiles)
int pt_moments_reset(pt_ctx *c);
// pt_map_probe.hip: unload the context's probe modules (pt_destroy, on the context's device)
void pt_probe_unload(pt_ctx *c);
