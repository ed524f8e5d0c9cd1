// pt_runtime.hip -- implementation of the C ABI in include/pt_abi.h: the context, the scene, the dispatch and the
// scene-side queries.  (The image-space entry points -- display, variance, the filters, temporal accumulation --
// are in pt_post_host.cpp, the mesh export in pt_mesh_host.cpp.)
//
// Owns what the reference's wgpu objects owned (path_tracer.rs:18-163,
// structs.rs:113-184, primitives.rs:59-157): the RGBA32F accumulation image,
// the scene program and its parameter buffer, and the dispatch.  One HIP
// stream per context; RCCL communicator for the multi-GPU image reduce.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_ctx.h"
#include "pt_device.h"
#include "pt_math.h"
#include "pt_post.h"

static_assert(sizeof(pt_constants) == 16, "Constants is 16 B (path_tracer.rs:149-155)");
static_assert(sizeof(pt_settings) == 20, "Settings is 20 B (path_tracer.rs:157-163)");
static_assert(sizeof(pt_op) == 33 * 4, "pt_op layout");
static_assert(sizeof(pt_aabb) == 14 * 4, "pt_aabb layout");
static_assert(sizeof(pt_scene_node) == 33 * 4, "pt_scene_node layout");
static_assert(PT_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "RCCL unique id size");
static_assert(sizeof(pt_camera) == 14 * 4, "pt_camera layout");
static_assert(sizeof(pt_sky) == 13 * 4, "pt_sky layout");

static int alloc_image(pt_ctx *c, uint32_t w, uint32_t h) {
    c->img.accum.release();
    c->img.reduced.release();
    c->img.width = w;
    c->img.height = h;
    const size_t bytes = std::max<size_t>(c->img.bytes(), 16);
    int rc = ensure(c, c->img.accum, bytes);
    if (rc != PT_OK) return rc;
    HIPCHK(c, hipMemsetAsync(c->img.accum.p, 0, bytes, c->stream));
    return pt_moments_reset(c);
}

// The moment image follows the accumulation image: its size, zeroed, while
// the option is on; either way the moments are no longer valid.
int pt_moments_reset(pt_ctx *c) {
    c->mom.valid = false;
    c->mom.frames = 0;
    if (!c->mom.on) return PT_OK;
    const size_t bytes = std::max<size_t>(c->img.bytes(), 16);
    const int rc = ensure(c, c->mom.img, bytes);
    if (rc != PT_OK) return rc;
    HIPCHK(c, hipMemsetAsync(c->mom.img.p, 0, bytes, c->stream));
    return PT_OK;
}

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }

int pt_create(int hip_device, uint32_t width, uint32_t height, pt_ctx **out) {
    if (!out) return PT_ERR_INVALID;
    *out = nullptr;
    pt_ctx *c = new (std::nothrow) pt_ctx();
    if (!c) return PT_ERR_INVALID;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || hip_device < 0 || hip_device >= ndev) {
        delete c;
        return PT_ERR_HIP;
    }
    c->device = hip_device;
    if (hipSetDevice(hip_device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        c->prog.stats.alloc(sizeof(unsigned long long) * 2 * PT_ST_COUNT) != hipSuccess) {
        pt_destroy(c);
        return PT_ERR_HIP;
    }
    if (alloc_image(c, width, height) != PT_OK) {
        pt_destroy(c);
        return PT_ERR_HIP;
    }
    *out = c;
    return PT_OK;
}

static int resize_clear(pt_ctx *c, uint32_t width, uint32_t height) {
    HIPCHK(c, hipSetDevice(c->device));
    if (width == c->img.width && height == c->img.height) {
        HIPCHK(c, hipMemsetAsync(c->img.accum.p, 0, std::max<size_t>(c->img.bytes(), 16), c->stream));
        return pt_moments_reset(c);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return alloc_image(c, width, height);
}

int pt_resize_clear(pt_ctx *c, uint32_t width, uint32_t height) {
    if (!c) return PT_ERR_INVALID;
    c->dn.guides_valid = false;
    if (width != c->img.width || height != c->img.height) c->hist.drop();  // (at the same size it is a clear: the history stays)
    return resize_clear(c, width, height);
}

int pt_set_program(pt_ctx *c, const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb,
                   uint32_t n_check) {
    if (!c) return PT_ERR_INVALID;
    if ((n_ops && !ops) || (n_aabb && !aabbs)) return fail(c, PT_ERR_INVALID, "null program arrays");
    if (n_check > PT_MAX_CHECK) return fail(c, PT_ERR_UNSUPPORTED, "more than 128 check[] entries");
    int depth = 0, max_depth = 0;
    for (uint32_t i = 0; i < n_ops; ++i) {
        const pt_op &o = ops[i];
        if (o.opcode == PT_OP_UNION_BEGIN) {
            max_depth = std::max(max_depth, ++depth);
        } else if (o.opcode == PT_OP_UNION_END) {
            if (--depth < 0) return fail(c, PT_ERR_INVALID, "unbalanced UNION_END");
            if (o.combine != PT_COMBINE_UNION && o.combine != PT_COMBINE_SUBTRACTION)
                return fail(c, PT_ERR_INVALID, "UNION_END combine must be union/subtraction");
        } else if (o.opcode == PT_OP_SHAPE) {
            if (depth < 1) return fail(c, PT_ERR_INVALID, "shape outside a union");
            if (o.shape == PT_NODE_PLANE) return fail(c, PT_ERR_UNSUPPORTED, "Shapes::Plane is not implemented upstream");
            if (o.shape < PT_NODE_SPHERE || o.shape > PT_NODE_OCTAHEDRON) return fail(c, PT_ERR_INVALID, "bad shape");
            if (o.combine > PT_COMBINE_SUBTRACTION) return fail(c, PT_ERR_INVALID, "bad combine");
            if (o.check >= int32_t(n_check)) return fail(c, PT_ERR_INVALID, "check index out of range");
        } else {
            return fail(c, PT_ERR_INVALID, "bad opcode");
        }
    }
    if (depth != 0) return fail(c, PT_ERR_INVALID, "unbalanced UNION_BEGIN");
    if (max_depth > PT_MAX_DEPTH) return fail(c, PT_ERR_UNSUPPORTED, "union nesting deeper than 8");
    for (uint32_t i = 0; i < n_aabb; ++i)
        if (aabbs[i].back < 0 || aabbs[i].back >= int32_t(n_check) || aabbs[i].so_kind > PT_SO_TORUS)
            return fail(c, PT_ERR_INVALID, "bad aabb record");
    c->dn.guides_valid = false;
    c->hist.drop();
    c->prog.ops.assign(ops, ops + n_ops);
    c->prog.aabbs.assign(aabbs, aabbs + n_aabb);
    c->prog.n_check = n_check;
    c->prog.have_program = true;
    c->prog.have_data = false;  // queue_compile reallocates data[] (sdf_editor.rs:36-40)
    return PT_OK;
}

int pt_set_data(pt_ctx *c, const float *data, uint32_t n) {
    if (!c) return PT_ERR_INVALID;
    if (!c->prog.have_program) return fail(c, PT_ERR_STATE, "pt_set_data before pt_set_program");
    if (n && !data) return fail(c, PT_ERR_INVALID, "null data");
    std::vector<PtNode> nodes;
    std::vector<PtAabb> boxes;
    std::vector<PtMat> mats;
    std::string err;
    int rc = pt_derive(c->prog.ops, c->prog.aabbs, data, n, nodes, boxes, mats, err);
    if (rc != PT_OK) return fail(c, rc, err);
    c->dn.guides_valid = false;
    c->hist.drop();
    HIPCHK(c, hipSetDevice(c->device));
    // stream-ordered upload: in-flight dispatches finish with the old tables
    HIPCHK(c, hipStreamSynchronize(c->stream));
    pt_ctx::Program &pr = c->prog;
    if ((rc = ensure(c, pr.nodes, nodes.size() * sizeof(PtNode))) != PT_OK) return rc;
    if ((rc = ensure(c, pr.boxes, boxes.size() * sizeof(PtAabb))) != PT_OK) return rc;
    if ((rc = ensure(c, pr.mats, mats.size() * sizeof(PtMat))) != PT_OK) return rc;
    if (!nodes.empty())
        HIPCHK(c, hipMemcpyAsync(pr.nodes.p, nodes.data(), nodes.size() * sizeof(PtNode), hipMemcpyHostToDevice, c->stream));
    if (!boxes.empty())
        HIPCHK(c, hipMemcpyAsync(pr.boxes.p, boxes.data(), boxes.size() * sizeof(PtAabb), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(pr.mats.p, mats.data(), mats.size() * sizeof(PtMat), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->prog.have_data = true;
    c->prog.bound_k = pt_bound_k(nodes);
    c->prog.fast_bounds = pt_fast_bounds(boxes);
    pt_jit_refresh(c->jit, nodes, boxes, c->prog.fast_bounds);
    c->prog.host_nodes = std::move(nodes);
    c->prog.host_boxes = std::move(boxes);
    return PT_OK;
}

int pt_set_tiles(pt_ctx *c, uint32_t rank, uint32_t nranks) {
    if (!c) return PT_ERR_INVALID;
    if (nranks == 0 || rank >= nranks) return fail(c, PT_ERR_INVALID, "rank must be < nranks");
    c->view.rank = rank;
    c->view.nranks = nranks;
    return resize_clear(c, c->img.width, c->img.height);  // (the size stays: the guide images, of every pixel, stay valid)
}

int pt_set_camera(pt_ctx *c, const pt_camera *cam) {
    if (!c) return PT_ERR_INVALID;
    if (!cam) {
        c->view.cam_mode = PT_CAM_DEFAULT;
        c->view.cam = kDefaultCamera;
        c->dn.guides_valid = false;
        return PT_OK;
    }
    float v[14];
    std::memcpy(v, cam, sizeof v);
    for (float f : v)
        if (!std::isfinite(f)) return fail(c, PT_ERR_INVALID, "camera field is not finite");
    if (cam->aperture < 0.0f) return fail(c, PT_ERR_INVALID, "camera aperture must be >= 0");
    if (cam->aperture > 0.0f && !(cam->focus > 0.0f))
        return fail(c, PT_ERR_INVALID, "camera focus must be > 0 with an aperture");
    c->view.cam = *cam;
    c->view.cam_mode = cam->aperture > 0.0f ? PT_CAM_LENS : PT_CAM_PINHOLE;
    c->dn.guides_valid = false;
    return PT_OK;
}

int pt_get_camera(const pt_ctx *c, pt_camera *out, int *is_default) {
    if (!c) return PT_ERR_INVALID;
    if (out) *out = c->view.cam;
    if (is_default) *is_default = c->view.cam_mode == PT_CAM_DEFAULT ? 1 : 0;
    return PT_OK;
}

int pt_set_sky(pt_ctx *c, const pt_sky *sky) {
    if (!c) return PT_ERR_INVALID;
    if (!sky) {
        c->view.sky_mode = PT_SKY_OFF;
        c->view.sky = pt_sky{};
        return PT_OK;
    }
    float v[13];
    std::memcpy(v, sky, sizeof v);
    for (float f : v)
        if (!std::isfinite(f)) return fail(c, PT_ERR_INVALID, "sky field is not finite");
    for (int k = 0; k < 3; ++k)
        if (sky->bottom[k] < 0.0f || sky->top[k] < 0.0f || sky->sun_color[k] < 0.0f)
            return fail(c, PT_ERR_INVALID, "sky colour component must be >= 0");
    if (sky->sun_cos < -1.0f || sky->sun_cos > 1.0f) return fail(c, PT_ERR_INVALID, "sky sun_cos must lie in [-1, 1]");
    c->view.sky = *sky;
    c->view.sky_mode = PT_SKY_ON;
    return PT_OK;
}

int pt_get_sky(const pt_ctx *c, pt_sky *out, int *is_off) {
    if (!c) return PT_ERR_INVALID;
    if (out) *out = c->view.sky;
    if (is_off) *is_off = c->view.sky_mode == PT_SKY_OFF ? 1 : 0;
    return PT_OK;
}

static bool use_binned(const PtLaunch &L) { return L.kernel == PT_KERNEL_BINNED && !pt_use_simple_kernel(L); }

// Launch one chunk: the scene-specialised wavefront kernel when loaded, else
// the ahead-of-time kernels (pt_kernel.hip, pt_bin_kernels.hip).
// moments: the launch also keeps the moment image (pt_dispatch: a path-traced
// writing launch of the binned pipeline or the simple kernel, nothing else --
// so never one of the wave kernel).
static int launch(pt_ctx *c, PtLaunch &L, bool stats, float *moments = nullptr) {
    const PtJitModule *jm = pt_jit_active(c->jit);
    if (use_binned(L)) {
        return pt_launch_binned(c, L, stats, moments);
    } else if (!pt_use_simple_kernel(L) && jm) {
        void *args[] = {&L};
        HIPCHK(c, hipModuleLaunchKernel(pt_jit_select(*jm, PtJitStage::Render, stats, false, false, false),
                                        unsigned(L.n_tiles), 1, 1, 64, 1, 1, 0, c->stream, args, nullptr));
    } else {
        pt_launch_render(L, stats, moments, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    return PT_OK;
}

static int make_launch(pt_ctx *c, const pt_constants *k, const pt_settings *s, uint32_t spp, PtLaunch &L) {
    if (!c) return PT_ERR_INVALID;
    if (!k || !s) return fail(c, PT_ERR_INVALID, "null constants/settings");
    if (!c->prog.have_program || !c->prog.have_data) return fail(c, PT_ERR_STATE, "no program/data uploaded");
    if (s->bounces < 0) return fail(c, PT_ERR_INVALID, "negative bounces");
    std::memset(&L, 0, sizeof L);
    L.nodes = c->prog.nodes.as<PtNode>();
    L.aabbs = c->prog.boxes.as<PtAabb>();
    L.fast_bounds = c->prog.fast_bounds ? 1 : 0;
    L.bound_k = c->prog.bound_k;
    L.mats = c->prog.mats.as<PtMat>();
    L.accum = c->img.accum.as<float>();
    L.n_nodes = int32_t(c->prog.ops.size());
    L.n_aabb = int32_t(c->prog.aabbs.size());
    L.width = int32_t(c->img.width);
    L.height = int32_t(c->img.height);
    L.tiles_x = int32_t((c->img.width + PT_TILE - 1) / PT_TILE);
    const int64_t tiles = int64_t(L.tiles_x) * int64_t((c->img.height + PT_TILE - 1) / PT_TILE);
    L.n_tiles = int32_t(tiles > int64_t(c->view.rank) ? (tiles - int64_t(c->view.rank) + c->view.nranks - 1) / c->view.nranks : 0);
    L.rank = int32_t(c->view.rank);
    L.nranks = int32_t(c->view.nranks);
    L.frame0 = k->frame;
    L.last_clear0 = k->last_clear;
    L.spp = int32_t(spp);
    L.debug = s->debug;
    L.bounces = s->bounces;
    L.fov = s->fov;
    L.aspect = k->aspect;
    L.write = 1;
    L.kernel = c->kernel;
    if (L.kernel == PT_KERNEL_AUTO) {
        // small dispatches take the tile-resident wave kernel: one launch, no
        // pass sequence and no per-pass tails.  Crossover measured at about
        // samples x ops = 2^27 (scripts/kernel_crossover.py: C1 3x faster at
        // 65 K samples; the 32-node scene binned from ~4 M samples on)
        const double work = double(L.n_tiles) * 64.0 * double(spp) * double(std::max<size_t>(1, c->prog.ops.size()));
        L.kernel = work < 134217728.0 ? PT_KERNEL_WAVEFRONT : PT_KERNEL_BINNED;
    }
    L.shade_batch = c->shade_batch;
    L.cam_mode = c->view.cam_mode;
    L.cam = c->view.cam;
    // (the debug views never add the sky: 1 and 2 do not path trace, 3 shows the segment count)
    L.sky_mode = s->debug == 0 ? c->view.sky_mode : PT_SKY_OFF;
    L.sky = c->view.sky;
    return PT_OK;
}

int pt_dispatch(pt_ctx *c, const pt_constants *k, const pt_settings *s, uint32_t spp) {
    PtLaunch L;
    int rc = make_launch(c, k, s, spp, L);
    if (rc != PT_OK) return rc;
    // second moments: a path-traced dispatch keeps the moment image too.  The wave kernel does
    // not serve it: the automatic choice is the binned pipeline whatever the size, and asking for the wave
    // kernel is refused before anything is touched
    const bool with_moments = c->mom.on && L.debug == 0;
    if (with_moments) {
        if (c->kernel == PT_KERNEL_WAVEFRONT)
            return fail(c, PT_ERR_UNSUPPORTED, "the wave kernel keeps no second moments: kernel 0, 1 or 3 with moments on");
        if (c->kernel == PT_KERNEL_AUTO) L.kernel = PT_KERNEL_BINNED;
    }
    float *moments = with_moments ? c->mom.img.as<float>() : nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    pt_jit_poll(c->jit, false);  // switch to the values-baked kernel once it is built
    // the moments stay valid only when this dispatch starts them (last_clear 0) or goes on from their frame
    // count; any other writing dispatch leaves the two images apart
    const uint32_t lc0 = uint32_t(k->last_clear);
    const bool moments_go_on = with_moments && (lc0 == 0 || (c->mom.valid && c->mom.frames == lc0));
    if (spp > 0) c->mom.valid = false;
    HIPCHK(c, c->dispatch_time.begin(c->stream));
    c->bin.tlog.used = c->bin.slog.used = c->bin.klog.used = 0;
    if (spp > 0 && L.n_tiles > 0) {
        // bound a single launch's length; chunks continue frame/last_clear.
        // The binned pipeline takes every frame at once: it splits by its own
        // sample budget, and larger chunks mean fuller passes (at N GPUs each
        // rank owns 1/N of the pixels and renders N times the frames).
        const uint32_t chunk = use_binned(L) ? spp : 64;
        for (uint32_t done = 0; done < spp; done += chunk) {
            PtLaunch Lc = L;
            Lc.spp = int32_t(std::min(chunk, spp - done));
            Lc.frame0 = int32_t(uint32_t(L.frame0) + done);
            Lc.last_clear0 = int32_t(uint32_t(L.last_clear0) + done);
            if (L.debug != 0 && done + chunk < spp) continue;  // direct stores: only the last frame survives
            if ((rc = launch(c, Lc, false, moments)) != PT_OK) return rc;
        }
    }
    HIPCHK(c, c->dispatch_time.end(c->stream));
    if (spp > 0 && moments_go_on) {
        c->mom.valid = true;
        c->mom.frames = lc0 + spp;
    }
    return PT_OK;
}

int pt_dispatch_stats(pt_ctx *c, const pt_constants *k, const pt_settings *s, uint32_t spp,
                      uint64_t counters[PT_STAT_COUNT]) {
    static_assert(PT_STAT_COUNT >= PT_ST_COUNT, "stat count");
    PtLaunch L;
    int rc = make_launch(c, k, s, spp, L);
    if (rc != PT_OK) return rc;
    if (!counters) return fail(c, PT_ERR_INVALID, "null counters");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(c->prog.stats.p, 0, sizeof(unsigned long long) * 2 * PT_ST_COUNT, c->stream));
    L.stats = c->prog.stats.as<unsigned long long>();
    L.write = 0;
    if (spp > 0 && L.n_tiles > 0)
        if ((rc = launch(c, L, true)) != PT_OK) return rc;
    unsigned long long host[2 * PT_ST_COUNT];  // [0, COUNT): everything else; [COUNT, 2 COUNT): shade-pass taps
    HIPCHK(c, hipMemcpyAsync(host, c->prog.stats.p, sizeof host, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < PT_STAT_COUNT; ++i) counters[i] = i < PT_ST_COUNT ? host[i] + host[PT_ST_COUNT + i] : 0;
    for (int i = 0; i < PT_ST_COUNT; ++i) c->prog.tap_stats[i] = host[PT_ST_COUNT + i];
    return PT_OK;
}

int pt_read_accum(pt_ctx *c, float *rgba, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    return read_back(c, rgba, bytes, c->img.accum.p, c->img.bytes(), "readback buffer too small");
}

int pt_write_accum(pt_ctx *c, const float *rgba, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    const size_t need = c->img.bytes();
    if (!rgba || bytes < need) return fail(c, PT_ERR_SIZE, "image buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    c->mom.valid = false;  // (pt_write_moments, after this, says what the new image's moments are)
    if (need) HIPCHK(c, hipMemcpyAsync(c->img.accum.p, rgba, need, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

// ---- second moments and variance -------------------------------
int pt_read_moments(pt_ctx *c, float *rgba, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    if (!c->mom.valid) return fail(c, PT_ERR_STATE, "no valid moments: set option moments and dispatch from last_clear 0");
    return read_back(c, rgba, bytes, c->mom.img.p, c->img.bytes(), "readback buffer too small");
}

int pt_write_moments(pt_ctx *c, const float *rgba, size_t bytes, uint32_t frames) {
    if (!c) return PT_ERR_INVALID;
    if (!c->mom.on) return fail(c, PT_ERR_STATE, "pt_write_moments needs option moments on");
    if (frames == 0) return fail(c, PT_ERR_INVALID, "moments of 0 frames");
    const size_t need = c->img.bytes();
    if (!rgba || bytes < need) return fail(c, PT_ERR_SIZE, "image buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (need) HIPCHK(c, hipMemcpyAsync(c->mom.img.p, rgba, need, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mom.valid = true;
    c->mom.frames = frames;
    return PT_OK;
}

// The launch block of one jitter-free primary ray per pixel (the guide images, the ray queries): every tile, whatever
// pt_set_tiles says; a lens as its pinhole (no lens draw, no rng at all); no sky; the image is not written (none of
// these kernels reads the flag: they store to their own planes).  Nothing of the context changes.
static int make_query_launch(pt_ctx *c, const pt_constants *k, const pt_settings *s, PtLaunch &L) {
    const int rc = make_launch(c, k, s, 1, L);
    if (rc != PT_OK) return rc;
    L.n_tiles = int32_t(int64_t(L.tiles_x) * int64_t((c->img.height + PT_TILE - 1) / PT_TILE));
    L.rank = 0;
    L.nranks = 1;
    if (L.cam_mode == PT_CAM_LENS) L.cam_mode = PT_CAM_PINHOLE;
    L.sky_mode = PT_SKY_OFF;
    L.write = 0;
    return PT_OK;
}

// ---- denoiser: the guide images (the filters are in pt_post_host.cpp) --------
int pt_render_guides(pt_ctx *c, const pt_constants *k, const pt_settings *s) {
    PtLaunch L;
    int rc = make_query_launch(c, k, s, L);
    if (rc != PT_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t plane = std::max<size_t>(c->img.bytes(), 16);
    for (DevBuf &g : c->dn.guides)
        if ((rc = ensure(c, g, plane)) != PT_OK) return rc;
    HIPCHK(c, c->dn.guide_time.begin(c->stream));
    pt_launch_guides(L, c->dn.guides[0].as<float>(), c->dn.guides[1].as<float>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->dn.guide_time.end(c->stream));
    c->dn.guides_valid = true;
    c->dn.guide_cam_mode = L.cam_mode;  // the view of these guides (pt_temporal_accumulate)
    c->dn.guide_cam = L.cam;
    c->dn.guide_aspect = L.aspect;
    c->dn.guide_fov = L.fov;
    return PT_OK;
}

int pt_read_guides(pt_ctx *c, float *g0, float *g1, size_t bytes_each) {
    if (!c) return PT_ERR_INVALID;
    if (!c->dn.guides_valid) return fail(c, PT_ERR_STATE, "guides stale: call pt_render_guides");
    const size_t need = c->img.bytes();
    if (bytes_each < need) return fail(c, PT_ERR_SIZE, "guide buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    // (either plane may be left out; one wait for both)
    if (g0 && need) HIPCHK(c, hipMemcpyAsync(g0, c->dn.guides[0].p, need, hipMemcpyDeviceToHost, c->stream));
    return read_back(c, g1, bytes_each, c->dn.guides[1].p, g1 ? need : 0, nullptr);
}

// ---- ray queries ------------------------------------------------
// the answers' staging for n rays (only what is asked for), then, after the kernel, their way back and the wait
static int query_outputs(pt_ctx *c, uint32_t n, const float *t, const int32_t *shape, const float *normal) {
    pt_ctx::Rays &r = c->rays;
    int rc;
    if (t && (rc = ensure(c, r.t, size_t(n) * 4)) != PT_OK) return rc;
    if (shape && (rc = ensure(c, r.shape, size_t(n) * 4)) != PT_OK) return rc;
    if (normal && (rc = ensure(c, r.normal, size_t(n) * 12)) != PT_OK) return rc;
    return PT_OK;
}

static int query_read_back(pt_ctx *c, uint32_t n, float *t, int32_t *shape, float *normal) {
    pt_ctx::Rays &r = c->rays;
    if (t) HIPCHK(c, hipMemcpyAsync(t, r.t.p, size_t(n) * 4, hipMemcpyDeviceToHost, c->stream));
    if (shape) HIPCHK(c, hipMemcpyAsync(shape, r.shape.p, size_t(n) * 4, hipMemcpyDeviceToHost, c->stream));
    if (normal) HIPCHK(c, hipMemcpyAsync(normal, r.normal.p, size_t(n) * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_trace_rays(pt_ctx *c, const float *ro, const float *rd, uint32_t n, float *t, int32_t *shape, float *normal) {
    if (!c) return PT_ERR_INVALID;
    if (n > PT_RAYS_MAX) return fail(c, PT_ERR_INVALID, "more than PT_RAYS_MAX rays");
    if (n && (!ro || !rd)) return fail(c, PT_ERR_INVALID, "null ray origins / directions");
    // (a query reads no constants and no settings: the launch block wants some)
    const pt_constants k = {0.0f, 0, 1.0f, 0};
    const pt_settings s = {0, 0, 1.0f, 1.0f, 0};
    PtLaunch L;
    int rc = make_query_launch(c, &k, &s, L);
    if (rc != PT_OK) return rc;
    if (!n) return PT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    pt_ctx::Rays &r = c->rays;
    if ((rc = ensure(c, r.ro, size_t(n) * 12)) != PT_OK) return rc;
    if ((rc = ensure(c, r.rd, size_t(n) * 12)) != PT_OK) return rc;
    if ((rc = query_outputs(c, n, t, shape, normal)) != PT_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(r.ro.p, ro, size_t(n) * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(r.rd.p, rd, size_t(n) * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, r.rays_time.begin(c->stream));
    pt_launch_rays(L, r.ro.as<float>(), r.rd.as<float>(), n, t ? r.t.as<float>() : nullptr,
                   shape ? r.shape.as<int32_t>() : nullptr, normal ? r.normal.as<float>() : nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, r.rays_time.end(c->stream));
    return query_read_back(c, n, t, shape, normal);
}

int pt_pick_pixels(pt_ctx *c, const pt_constants *k, const pt_settings *s, const int32_t *xy, uint32_t n, float *t,
                   int32_t *shape, float *normal) {
    if (!c) return PT_ERR_INVALID;
    if (n > PT_RAYS_MAX) return fail(c, PT_ERR_INVALID, "more than PT_RAYS_MAX pixels");
    PtLaunch L;
    int rc = make_query_launch(c, k, s, L);
    if (rc != PT_OK) return rc;
    if (!n) return PT_OK;
    const uint32_t w = c->img.width, h = c->img.height;
    if (!xy) {
        if (uint64_t(n) != uint64_t(w) * uint64_t(h))
            return fail(c, PT_ERR_INVALID, "a NULL pixel list means every pixel: n must be width * height");
    } else {
        for (uint32_t i = 0; i < n; ++i) {
            const int32_t x = xy[2 * size_t(i)], y = xy[2 * size_t(i) + 1];
            if (x < 0 || y < 0 || uint32_t(x) >= w || uint32_t(y) >= h) return fail(c, PT_ERR_INVALID, "pixel outside the image");
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    pt_ctx::Rays &r = c->rays;
    if (xy && (rc = ensure(c, r.xy, size_t(n) * 8)) != PT_OK) return rc;
    if ((rc = query_outputs(c, n, t, shape, normal)) != PT_OK) return rc;
    if (xy) HIPCHK(c, hipMemcpyAsync(r.xy.p, xy, size_t(n) * 8, hipMemcpyHostToDevice, c->stream));
    // the list: one thread per entry; every pixel: one per pixel of every tile, as the guide kernel
    const uint32_t threads = xy ? n : uint32_t(L.n_tiles) * 64u;
    HIPCHK(c, r.pick_time.begin(c->stream));
    pt_launch_pick(L, xy ? r.xy.as<int32_t>() : nullptr, threads, t ? r.t.as<float>() : nullptr,
                   shape ? r.shape.as<int32_t>() : nullptr, normal ? r.normal.as<float>() : nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, r.pick_time.end(c->stream));
    return query_read_back(c, n, t, shape, normal);
}

// ---- radiance queries ---------------------------------------------
// The launch block is a dispatch's (make_launch): debug 0, so the sky is kept; bounces from p; the image is not
// written (none of these kernels reads the flag or the image).  The rays are walked in chunks of whole rays, at
// most "radiance_samples" samples in flight: the colours and the shared first hits are a chunk's, the rays, the
// means and the moments the call's.
int pt_trace_radiance(pt_ctx *c, const float *ro, const float *rd, uint32_t n, const pt_radiance_params *p, float *mean,
                      float *moment) {
    if (!c) return PT_ERR_INVALID;
    if (!p) return fail(c, PT_ERR_INVALID, "null radiance parameters");
    if (n > PT_RAYS_MAX) return fail(c, PT_ERR_INVALID, "more than PT_RAYS_MAX rays");
    if (n && (!ro || !rd)) return fail(c, PT_ERR_INVALID, "null ray origins / directions");
    if (p->spp < 1 || p->spp > PT_RADIANCE_MAX_SPP) return fail(c, PT_ERR_INVALID, "spp outside [1, PT_RADIANCE_MAX_SPP]");
    if (uint64_t(p->sample0) + uint64_t(p->spp) > (1ull << 24)) return fail(c, PT_ERR_INVALID, "sample0 + spp beyond 1 << 24");
    if (p->bounces < 0) return fail(c, PT_ERR_INVALID, "negative bounces");
    if (p->mode != PT_RADIANCE_RAY && p->mode != PT_RADIANCE_HEMISPHERE) return fail(c, PT_ERR_INVALID, "bad radiance mode");
    if (p->sample0 > 0 && (!mean || !moment)) return fail(c, PT_ERR_INVALID, "a continuation (sample0 > 0) needs mean and moment");
    const pt_constants k = {0.0f, 0, 1.0f, 0};  // (a query reads no constants: the launch block wants some)
    const pt_settings s = {0, p->bounces, 1.0f, 1.0f, 0};
    PtLaunch L;
    int rc = make_launch(c, &k, &s, 1, L);
    if (rc != PT_OK) return rc;
    L.write = 0;
    if (!n) return PT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    pt_ctx::Radiance &r = c->rad;
    const uint32_t chunk_rays = std::min<uint32_t>(n, std::max<uint32_t>(1u, uint32_t(r.samples) / p->spp));
    const bool shared = p->mode == PT_RADIANCE_RAY;
    if ((rc = ensure(c, r.ro, size_t(n) * 12)) != PT_OK) return rc;
    if ((rc = ensure(c, r.rd, size_t(n) * 12)) != PT_OK) return rc;
    if ((mean || p->sample0) && (rc = ensure(c, r.mean, size_t(n) * 12)) != PT_OK) return rc;
    if ((moment || p->sample0) && (rc = ensure(c, r.moment, size_t(n) * 12)) != PT_OK) return rc;
    if (shared && (rc = ensure(c, r.first, size_t(chunk_rays) * 32)) != PT_OK) return rc;
    if ((rc = ensure(c, r.colour, size_t(chunk_rays) * p->spp * 16)) != PT_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(r.ro.p, ro, size_t(n) * 12, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(r.rd.p, rd, size_t(n) * 12, hipMemcpyHostToDevice, c->stream));
    if (p->sample0) {
        HIPCHK(c, hipMemcpyAsync(r.mean.p, mean, size_t(n) * 12, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(r.moment.p, moment, size_t(n) * 12, hipMemcpyHostToDevice, c->stream));
    }
    PtRadiance R = {};
    R.ro = r.ro.as<float>();
    R.rd = r.rd.as<float>();
    R.first = r.first.as<float4>();
    R.colour = r.colour.as<float4>();
    R.mean = mean ? r.mean.as<float>() : nullptr;
    R.moment = moment ? r.moment.as<float>() : nullptr;
    R.spp = p->spp;
    R.sample0 = p->sample0;
    R.seed = p->seed;
    R.mode = p->mode;
    r.klog.used = r.flog.used = 0;
    for (uint32_t done = 0; done < n; done += chunk_rays) {
        R.ray0 = done;
        R.rays = std::min(chunk_rays, n - done);
        HIPCHK(c, r.klog.record(c->stream));
        if (shared) {
            HIPCHK(c, r.flog.record(c->stream));
            pt_launch_radiance(PtRadianceStage::First, L, R, c->stream);
            HIPCHK(c, r.flog.record(c->stream));
        }
        pt_launch_radiance(PtRadianceStage::Samples, L, R, c->stream);
        pt_launch_radiance(PtRadianceStage::Fold, L, R, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, r.klog.record(c->stream));
    }
    if (mean) HIPCHK(c, hipMemcpyAsync(mean, r.mean.p, size_t(n) * 12, hipMemcpyDeviceToHost, c->stream));
    if (moment) HIPCHK(c, hipMemcpyAsync(moment, r.moment.p, size_t(n) * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

// ---- preview shading ------------------------------------------------
static_assert(sizeof(pt_preview_params) == 22 * 4, "pt_preview_params layout");

// The launch block is a guide render's (every tile, a lens as its pinhole) but with the sky kept: a miss shows it.
// The preview reads fov of the settings and nothing else, so the debug view and the bounce count do not enter.
int pt_render_preview(pt_ctx *c, const pt_constants *k, const pt_settings *s, const pt_preview_params *p, int format,
                      void *out, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    if (!k || !s) return fail(c, PT_ERR_INVALID, "null constants/settings");
    if (!p) return fail(c, PT_ERR_INVALID, "null preview parameters");
    if (format != PT_DISPLAY_RGBA32F && format != PT_DISPLAY_SRGB8 && format != PT_DENOISE_LINEAR)
        return fail(c, PT_ERR_INVALID, "bad preview format");
    for (const float *v3 : {p->light_dir, p->light_color, p->ambient_bottom, p->ambient_top, p->highlight_color})
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(v3[a])) return fail(c, PT_ERR_INVALID, "preview light, ambient and highlight colours must be finite");
    if (p->shadow_steps > PT_PREVIEW_MAX_SHADOW_STEPS) return fail(c, PT_ERR_INVALID, "preview shadow_steps must be in [0, 64]");
    if (!std::isfinite(p->shadow_k) || !(p->shadow_k > 0.0f)) return fail(c, PT_ERR_INVALID, "preview shadow_k must be finite and > 0");
    if (p->shadow_cull > 1) return fail(c, PT_ERR_INVALID, "preview shadow_cull must be 0 or 1");
    for (float v : {p->ao_strength, p->ao_radius})
        if (!std::isfinite(v) || v < 0.0f) return fail(c, PT_ERR_INVALID, "preview ao_strength and ao_radius must be finite and >= 0");
    if (p->highlight < -1) return fail(c, PT_ERR_INVALID, "preview highlight must be a shape ordinal or -1");
    if (!(p->highlight_mix >= 0.0f && p->highlight_mix <= 1.0f)) return fail(c, PT_ERR_INVALID, "preview highlight_mix must lie in [0, 1]");
    pt_settings view = *s;
    view.debug = 0;    // (make_launch keeps the sky for the path-traced view only)
    view.bounces = 0;  // (and refuses a negative count, which nothing here reads)
    PtLaunch L;
    int rc = make_query_launch(c, k, &view, L);
    if (rc != PT_OK) return rc;
    L.sky_mode = c->view.sky_mode;
    const size_t texels = size_t(c->img.width) * c->img.height;
    const size_t need = texels * (format == PT_DISPLAY_SRGB8 ? 4 : 16);
    if (!out || bytes < need) return fail(c, PT_ERR_SIZE, "preview output buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    pt_ctx::Preview &pv = c->preview;
    if ((rc = ensure(c, pv.img, std::max<size_t>(texels * 16, 16))) != PT_OK) return rc;
    if (format != PT_DENOISE_LINEAR && (rc = ensure(c, c->img.display, std::max<size_t>(need, 16))) != PT_OK) return rc;
    PtPreview V;
    V.p = *p;
    V.out = pv.img.as<float4>();
    HIPCHK(c, pv.time.begin(c->stream));
    pt_launch_preview(L, V, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, pv.time.end(c->stream));
    const void *result = pv.img.p;
    if (format != PT_DENOISE_LINEAR) {
        pt_launch_display(pv.img.as<float>(), c->img.width, c->img.height, format, c->img.display.p, c->stream);
        HIPCHK(c, hipGetLastError());
        result = c->img.display.p;
    }
    return read_back(c, out, bytes, result, need, nullptr);
}

int pt_accum_device_ptr(pt_ctx *c, void **dev_ptr, size_t *bytes) {
    if (!c || !dev_ptr || !bytes) return PT_ERR_INVALID;
    *dev_ptr = c->img.accum.p;
    *bytes = c->img.bytes();
    return PT_OK;
}

int pt_get_size(const pt_ctx *c, uint32_t *w, uint32_t *h) {
    if (!c || !w || !h) return PT_ERR_INVALID;
    *w = c->img.width;
    *h = c->img.height;
    return PT_OK;
}

int pt_comm_get_unique_id(uint8_t id[PT_COMM_ID_BYTES]) {
    if (!id) return PT_ERR_INVALID;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return PT_ERR_RCCL;
    std::memcpy(id, u.internal, PT_COMM_ID_BYTES);
    return PT_OK;
}

int pt_comm_init(pt_ctx *c, uint32_t nranks, uint32_t rank, const uint8_t id[PT_COMM_ID_BYTES]) {
    if (!c || !id || nranks == 0 || rank >= nranks) return fail(c, PT_ERR_INVALID, "bad communicator arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->comm.comm) {
        ncclCommDestroy(c->comm.comm);
        c->comm.comm = nullptr;
    }
    ncclUniqueId u;
    std::memcpy(u.internal, id, PT_COMM_ID_BYTES);
    ncclResult_t r = ncclCommInitRank(&c->comm.comm, int(nranks), u, int(rank));
    if (r != ncclSuccess) return fail(c, PT_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    c->comm.nranks = nranks;
    return PT_OK;
}

int pt_comm_size(pt_ctx *c, uint32_t *nranks) {
    if (!c || !nranks) return PT_ERR_INVALID;
    if (!c->comm.comm) return fail(c, PT_ERR_STATE, "pt_comm_init not called");
    int n = 0;
    ncclResult_t r = ncclCommCount(c->comm.comm, &n);
    if (r != ncclSuccess) return fail(c, PT_ERR_RCCL, std::string("ncclCommCount: ") + ncclGetErrorString(r));
    *nranks = uint32_t(n);
    return PT_OK;
}

int pt_reduce_accum(pt_ctx *c, int root) {
    if (!c) return PT_ERR_INVALID;
    if (!c->comm.comm) return fail(c, PT_ERR_STATE, "pt_comm_init not called");
    if (root < 0 || uint32_t(root) >= c->comm.nranks) return fail(c, PT_ERR_INVALID, "bad root");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t count = size_t(c->img.width) * c->img.height * 4;
    int rc = ensure(c, c->img.reduced, std::max<size_t>(count * 4, 16));
    if (rc != PT_OK) return rc;
    // non-owned texels are exactly 0 on every other rank, so the sum is the
    // bit-exact single-GPU image (x + 0 = x)
    ncclResult_t r = ncclReduce(c->img.accum.p, c->img.reduced.p, count, ncclFloat32, ncclSum, root, c->comm.comm, c->stream);
    if (r != ncclSuccess) return fail(c, PT_ERR_RCCL, std::string("ncclReduce: ") + ncclGetErrorString(r));
    return PT_OK;
}

int pt_read_reduced(pt_ctx *c, float *rgba, size_t bytes) {
    if (!c) return PT_ERR_INVALID;
    if (!c->img.reduced.p) return fail(c, PT_ERR_STATE, "no reduced image");
    return read_back(c, rgba, bytes, c->img.reduced.p, c->img.bytes(), "readback buffer too small");
}

int pt_sync(pt_ctx *c) {
    if (!c) return PT_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_last_dispatch_ms(pt_ctx *c, float *ms) {
    if (!c || !ms) return PT_ERR_INVALID;
    if (!c->dispatch_time.timed) return fail(c, PT_ERR_STATE, "no dispatch recorded");
    HIPCHK(c, c->dispatch_time.ms(ms, true));
    return PT_OK;
}

const char *pt_jit_log(const pt_ctx *c) { return c ? c->jit.log.c_str() : ""; }

const char *pt_last_error(const pt_ctx *c) { return c ? c->err.c_str() : "null context"; }

void pt_destroy(pt_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm.comm) ncclCommDestroy(c->comm.comm);
    pt_jit_destroy(c->jit);  // (waits for a pending tier-up build)
    pt_probe_unload(c);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;  // its buffers, events and lane streams go with their owners, on this device
}

}  // extern "C"
