/*
 * pt_abi.h -- C ABI of the MI355X-native SDF path-trace hot path.
 *
 * This is the drop-in boundary that replaces the wgpu objects owned by the
 * reference's `PathTracer` (src/path_tracer/path_tracer.rs:18-163), the
 * `data[]` storage buffer of `DataArray` (src/sdf_editor/primitives.rs:59-157)
 * and the GLSL text that `SDFEditor::compile` (src/sdf_editor/sdf_editor.rs:
 * 186-246) splices into the compute shader.  Plain C types only; every entry
 * point returns a status code (PT_OK = 0); `pt_last_error` explains failures.
 * Inputs are borrowed and copied before return; outputs are caller-owned.
 * Calls on one context are not re-entrant (the reference is single-threaded,
 * src/inbuilt/event_loop.rs:7-76).  See INTEGRATION.md for the Rust binding.
 */
#ifndef PT_ABI_H
#define PT_ABI_H

#ifndef __HIPCC_RTC__ /* also embedded in the hipRTC-compiled scene kernels */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 1

/* status codes */
#define PT_OK 0
#define PT_ERR_INVALID -1      /* bad argument / malformed program or scene */
#define PT_ERR_HIP -2          /* HIP runtime failure */
#define PT_ERR_UNSUPPORTED -3  /* e.g. Shapes::Plane (containers.rs:287,295 emits NotImplemented) */
#define PT_ERR_STATE -4        /* program/data missing, wrong call order */
#define PT_ERR_RCCL -5         /* collective failure */
#define PT_ERR_SIZE -6         /* caller buffer too small (required size written back) */

typedef struct pt_ctx pt_ctx;

/* == `Constants` UBO (path_tracer.rs:149-155, test_compute.glsl:6-11), 16 B */
typedef struct {
    float time;
    int32_t frame;
    float aspect;
    int32_t last_clear;
} pt_constants;

/* == `Settings` UBO (path_tracer.rs:157-163, test_compute.glsl:13-19), 20 B */
typedef struct {
    int32_t debug;   /* 0 path trace, 1 normals, 2 albedo, 3 bounce heat map */
    int32_t bounces;
    float scale;
    float fov;
    int32_t aabb;    /* unused by the kernel, as upstream */
} pt_settings;

/* ---------------------------------------------------------------------
 * Scene tree (the SDFEditor node graph, flattened) -> compiled program
 * --------------------------------------------------------------------- */
#define PT_NODE_UNION 0       /* containers.rs:8-15 */
#define PT_NODE_SPHERE 1      /* containers.rs:260 */
#define PT_NODE_CUBE 2        /* containers.rs:261 */
#define PT_NODE_TORUS 3       /* extension: BASELINE.json config 2 (absent upstream) */
#define PT_NODE_OCTAHEDRON 4  /* shapes.glsl:13-25 (deprecated editor format) */
#define PT_NODE_PLANE 5       /* containers.rs:262, unimplemented upstream -> PT_ERR_UNSUPPORTED */

#define PT_UNION_TYPE_UNION 0       /* containers.rs:244-252 */
#define PT_UNION_TYPE_SUBTRACTION 1

/* One Union or Shape.  A union's children are the later nodes whose `parent`
 * is its index, in array order; parent -1 = SDFEditor.header_unions. */
typedef struct {
    int32_t kind;
    int32_t parent;
    int32_t union_type;
    int32_t aabb;               /* Transform.aabb */
    float scale;                /* Transform.scale */
    float position[3];
    float rotation[3];
    float aabb_exaggeration;
    float size[3];              /* sphere [0]; cube xyz; torus (R, r); octahedron [0] */
    float material[18];         /* Material in Mat order (test_compute.glsl:45-59) */
} pt_scene_node;

#define PT_OP_UNION_BEGIN 0
#define PT_OP_SHAPE 1
#define PT_OP_UNION_END 2

#define PT_COMBINE_ASSIGN 0       /* UnionType::compile index 0 (containers.rs:245-247) */
#define PT_COMBINE_UNION 1        /* opUnion, shapes.glsl:72-74 */
#define PT_COMBINE_SUBTRACTION 2  /* opSubtraction, shapes.glsl:76-81 */

/* One statement of the generated `map()`; operands are data[] slot indices.
 * Replaces the GLSL text of Union::compile / Shape::compile. */
typedef struct {
    uint32_t opcode;
    uint32_t shape;          /* PT_NODE_* for SHAPE */
    uint32_t combine;        /* how the result joins the enclosing accumulator */
    int32_t check;           /* check[] index guarding a SHAPE, -1 = `if (true)` */
    uint32_t scale;
    uint32_t position[3];
    uint32_t rotation[3];
    uint32_t aabb_exaggeration;
    uint32_t size[3];
    uint32_t material[18];
} pt_op;

#define PT_SO_SCALAR 0  /* vec3(size[0])  sphere, octahedron */
#define PT_SO_VEC3 1    /* size.xyz       cube */
#define PT_SO_ONE 2     /* vec3(1.0)      (Plane; never reached) */
#define PT_SO_TORUS 3   /* extension: vec3(R + r, r, R + r) */

/* One `if (bool_hit(intersectAABB(...))) back[i] = true;` of the generated
 * `bounds()` (Shape::aabb_compile, containers.rs:442-463). */
typedef struct {
    int32_t back;
    uint32_t so_kind;
    uint32_t union_position[3];
    uint32_t union_scale;
    uint32_t shape_position[3];
    uint32_t shape_scale;
    uint32_t size[3];
    uint32_t aabb_exaggeration;
} pt_aabb;

/* Compile a scene tree exactly as SDFEditor::compile allocates data[] slots
 * and check[] indices (sdf_editor.rs:186-246).  Two-call pattern: any output
 * pointer may be NULL, sizes are always written; returns PT_ERR_SIZE if a
 * capacity is too small.  Host-only, no GPU needed.  Every Float gets its
 * own slot (the editor draws a fresh random hash per Float,
 * primitives.rs:12-17,220). */
int pt_compile_scene(const pt_scene_node *nodes, uint32_t n_nodes,
                     pt_op *ops, uint32_t ops_cap, uint32_t *n_ops,
                     pt_aabb *aabbs, uint32_t aabb_cap, uint32_t *n_aabb,
                     float *data, uint32_t data_cap, uint32_t *n_data,
                     uint32_t *n_check);

/* The identity of one Float: its serde `hash` (u128, primitives.rs:210).
 * DataArray::get_index (primitives.rs:117-129) gives Floats that share a hash
 * one data[] slot, holding the first one's value (cloned nodes and edited
 * JSON files share hashes).  {0, 0} = anonymous: always a fresh slot. */
typedef struct {
    uint64_t lo, hi;
} pt_float_key;
/* Keys per node: scale, position xyz, rotation xyz, aabb_exaggeration,
 * size[3], material[18] (a union uses the first 8). */
#define PT_NODE_FLOATS 29
/* pt_compile_scene with the Floats' hashes: keys[node * PT_NODE_FLOATS + k]
 * (NULL = all anonymous, the same as pt_compile_scene). */
int pt_compile_scene_keyed(const pt_scene_node *nodes, uint32_t n_nodes, const pt_float_key *keys,
                           pt_op *ops, uint32_t ops_cap, uint32_t *n_ops,
                           pt_aabb *aabbs, uint32_t aabb_cap, uint32_t *n_aabb,
                           float *data, uint32_t data_cap, uint32_t *n_data,
                           uint32_t *n_check);

/* ---------------------------------------------------------------------
 * Render context
 * --------------------------------------------------------------------- */
/* == StorageTexturePackage::new (structs.rs:113-160): RGBA32F image, zeroed.
 * Device memory is row-major, row y = 0 first, 16 B per texel. */
int pt_create(int hip_device, uint32_t width, uint32_t height, pt_ctx **out);
/* == StorageTexturePackage::remake + `last_clear = 0` (path_tracer.rs:101-106) */
int pt_resize_clear(pt_ctx *ctx, uint32_t width, uint32_t height);
/* == PathTracer::remake_pipeline(map) (path_tracer.rs:62-76): topology change */
int pt_set_program(pt_ctx *ctx, const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb,
                   uint32_t n_check);
/* == DataArray::update (primitives.rs:131-151): value-only update, no recompile */
int pt_set_data(pt_ctx *ctx, const float *data, uint32_t n);
/* Multi-GPU tile ownership (new): 8x8 tile t is rendered iff t % nranks == rank.
 * Clears the image (non-owned texels stay exactly 0). */
int pt_set_tiles(pt_ctx *ctx, uint32_t rank, uint32_t nranks);
/* Camera pose and lens (new; the reference's view is fixed, test_compute.glsl:
 * 232-235).  With ux, uy the jittered, aspect-scaled screen coordinates the
 * reference forms, a primary ray leaves `origin` along
 * normalize(right * ux + up * uy + forward * fov); the reference's camera is
 * origin (0, 0, -3) with the identity basis.  aperture > 0 is a thin lens of
 * that radius: the ray starts at a uniformly drawn point of the lens disc
 * (spanned by right and up) and passes through the pinhole ray's point at
 * distance `focus` (DESIGN.md 3.24 has the f32 steps and the draw order).
 * The basis is used as given: it is not checked for orthonormality, and a
 * skewed or scaled one shears or zooms the picture. */
typedef struct {            /* 56 bytes, 14 floats */
    float origin[3];
    float right[3], up[3], forward[3];   /* camera basis in world space */
    float aperture;         /* lens radius; 0 = pinhole */
    float focus;            /* distance along the ray to the in-focus point; used iff aperture > 0 */
} pt_camera;
/* cam == NULL: back to the reference's fixed camera.  PT_ERR_INVALID (the
 * previous camera stays in force) when a field is not finite, aperture < 0,
 * or aperture > 0 with focus <= 0.  Takes effect at the next pt_dispatch /
 * pt_dispatch_stats; does not clear the image (the caller does, as for a
 * settings change). */
int pt_set_camera(pt_ctx *ctx, const pt_camera *cam);
/* The camera in force; *is_default = 1 when it is the reference's fixed one
 * (*out then holds its pose).  Either output may be NULL. */
int pt_get_camera(const pt_ctx *ctx, pt_camera *out, int *is_default);
/* Sky light (new; in the reference a ray that leaves the scene adds nothing,
 * test_compute.glsl:106, and its AMBENT is never used).  With a sky set and
 * debug == 0, a segment whose march misses (CastRay's t > FP) adds, before
 * the path ends, g * throughput to the path's radiance, where for the
 * segment's direction rd
 *   t = rd.y * 0.5 + 0.5,  g = bottom + (top - bottom) * t,
 *   g += sun_color  where dot(rd, sun_dir) >= sun_cos
 * (DESIGN.md 3.25 has the f32 steps).  Paths that end by Russian roulette or
 * at the bounce limit add nothing, no random number is drawn, and the debug
 * views do not change. */
typedef struct {            /* 52 bytes, 13 floats */
    float bottom[3];        /* radiance looking straight down (rd.y = -1) */
    float top[3];           /* radiance looking straight up   (rd.y = +1) */
    float sun_dir[3];       /* towards the sun; used as given, not normalised */
    float sun_color[3];     /* added where dot(rd, sun_dir) >= sun_cos; all 0 = no sun */
    float sun_cos;
} pt_sky;
/* sky == NULL: off, the reference's void.  PT_ERR_INVALID (the previous sky
 * stays in force) when a field is not finite, a colour component is negative
 * or sun_cos lies outside [-1, 1].  Takes effect at the next pt_dispatch /
 * pt_dispatch_stats; does not clear the image (the caller does, as for a
 * settings change); survives pt_resize_clear, pt_set_program and pt_set_data. */
int pt_set_sky(pt_ctx *ctx, const pt_sky *sky);
/* The sky in force; *is_off = 1 when none is set (*out is then all zero).
 * Either output may be NULL. */
int pt_get_sky(const pt_ctx *ctx, pt_sky *out, int *is_off);
/* == `spp` successive (PathTracer::update, compute_pass) pairs: frame j uses
 * frame = c->frame + j and last_clear = c->last_clear + j (path_tracer.rs:
 * 110-111).  Asynchronous, ordered on the context's HIP stream. */
int pt_dispatch(pt_ctx *ctx, const pt_constants *c, const pt_settings *s, uint32_t spp);
/* == State::save_image readback (state.rs:237-303): blocking copy of the
 * local image (w*h*4 floats) into a caller buffer. */
int pt_read_accum(pt_ctx *ctx, float *rgba, size_t bytes);
/* Inverse of pt_read_accum (new): replace the local image with w*h*4 floats
 * from a caller buffer (resume a progressive render from a saved image, or
 * feed the display pass).  Blocking. */
int pt_write_accum(pt_ctx *ctx, const float *rgba, size_t bytes);
/* == the pixel transform of State::save_image (state.rs:277-289), host only:
 * `rgba` (w*h*4 floats, row 0 = y 0, as pt_read_accum returns it) to the
 * 8-bit RGBA of image.png, row 0 = top (rows flipped, :283): r, g, b =
 * (v.powf(1.0 / 2.2) * 255.0) as u8 with Rust's f32 1.0 / 2.2 and libm powf,
 * a = (v * 255.0) as u8; `as u8` saturates (NaN -> 0).  `out` holds w*h*4
 * bytes. */
int pt_save_rgba8(const float *rgba, uint32_t width, uint32_t height, uint8_t *out, size_t bytes);
/* Device pointer + size of the local image (for external collectives). */
int pt_accum_device_ptr(pt_ctx *ctx, void **dev_ptr, size_t *bytes);
int pt_get_size(const pt_ctx *ctx, uint32_t *width, uint32_t *height);

/* RCCL over xGMI (new).  The 128-byte id is produced on one rank and
 * broadcast by the caller's own channel (e.g. torch.distributed). */
#define PT_COMM_ID_BYTES 128
int pt_comm_get_unique_id(uint8_t id[PT_COMM_ID_BYTES]);
int pt_comm_init(pt_ctx *ctx, uint32_t nranks, uint32_t rank, const uint8_t id[PT_COMM_ID_BYTES]);
/* Ranks of the context's communicator as RCCL reports them (ncclCommCount):
 * the check that an N-GPU run reduced over N ranks.  PT_ERR_STATE before
 * pt_comm_init. */
int pt_comm_size(pt_ctx *ctx, uint32_t *nranks);
/* Sum of every rank's image into this context's result image on `root`
 * (out of place: the local accumulation keeps progressing). */
int pt_reduce_accum(pt_ctx *ctx, int root);
int pt_read_reduced(pt_ctx *ctx, float *rgba, size_t bytes);

int pt_sync(pt_ctx *ctx);
/* Device time (HIP events on the context stream) of the kernels of the last
 * pt_dispatch, in ms; blocks until they finished. */
int pt_last_dispatch_ms(pt_ctx *ctx, float *ms);
/* Instrumented re-run of one dispatch (does not touch the image): per-event
 * work counters for algorithmic-flop accounting, in the order
 * of compute_path_tracer_amd/_native.py STAT_NAMES. */
#define PT_STAT_COUNT 32
int pt_dispatch_stats(pt_ctx *ctx, const pt_constants *c, const pt_settings *s, uint32_t spp,
                      uint64_t counters[PT_STAT_COUNT]);
/* Display pass (replaces RenderTexturePipeline::render_pass,
 * render_texture_pipeline.rs:77-110 + render_texture_shader.wgsl:23-94):
 * ACESFilm + LinearToSRGB of the accumulation image.
 *   PT_DISPLAY_RGBA32F: fs_main's vec4 per texel, texel order (row 0 =
 *     bottom), w*h*16 bytes;
 *   PT_DISPLAY_SRGB8: the 8-bit RGBA the sRGB swapchain (setup.rs:53-59)
 *     stores -- encoded a second time, the reference's double-sRGB -- in
 *     screen order (row 0 = top), w*h*4 bytes.
 * Blocking; the output buffer is caller-owned (host memory). */
#define PT_DISPLAY_RGBA32F 0
#define PT_DISPLAY_SRGB8 1
int pt_display(pt_ctx *ctx, int format, void *out, size_t bytes);
/* Denoiser (new; DESIGN.md 3.26 has the f32 steps of both stages).
 * Guide images: one primary ray per pixel through the jitter-free screen point
 * the reference's calc_uv forms for it, from the camera in force (a
 * lens as its pinhole), no random numbers, every pixel whatever pt_set_tiles
 * says.  Two RGBA32F planes of w*h texels in the accumulation image's order:
 *   g0 = {normal.xyz, t}            (normal 0 where the ray misses)
 *   g1 = {albedo.rgb, 1 hit / 0 miss}
 * Uses c->aspect and s->fov.  Asynchronous, on the context's stream; sets the
 * context's "guides valid" flag, which pt_resize_clear, pt_set_program,
 * pt_set_data and pt_set_camera clear (pt_set_sky, pt_set_tiles, dispatches
 * and option changes do not).  PT_ERR_STATE without program or data. */
int pt_render_guides(pt_ctx *ctx, const pt_constants *c, const pt_settings *s);
/* Blocking copy of the guide planes (w*h*16 bytes each); either pointer may be
 * NULL.  PT_ERR_STATE while the guides are not valid. */
int pt_read_guides(pt_ctx *ctx, float *g0, float *g1, size_t bytes_each);
/* Edge-stopping a-trous wavelet filter (Dammertz et al. 2010) of the
 * accumulation image, steered by the guide images.  Iteration i (from 0)
 * taps a 5x5 B3 kernel at step 1 << i; a tap's weight is divided by
 * (1 + |dcolour|^2 kc_i) (1 + |dalbedo|^2 ka) (1 + dt^2 kz_i) and multiplied
 * by max(dot(n_p, n_q), 0)^(2^normal_power_log2), with
 *   kc_i = 1 / (sigma_color * 2^-i)^2, kz_i = 1 / (sigma_depth * 2^i)^2,
 *   ka = 1 / sigma_albedo^2            (a sigma of 0 switches its term off);
 * hit and miss texels never mix, and a non-finite texel stays as it is and
 * spreads nowhere. */
typedef struct {                 /* 20 bytes */
    uint32_t iterations;         /* 1..8 */
    uint32_t normal_power_log2;  /* 0..8: the clamped normal dot product is squared this many times */
    float sigma_color;           /* halved every iteration; 0 = term off */
    float sigma_depth;           /* doubled every iteration; 0 = term off */
    float sigma_albedo;          /* 0 = term off */
} pt_denoise_params;
/* Reads the accumulation image and never writes it (a progressive render goes
 * on afterwards as if it had not been called); filters through two device
 * buffers and copies the result out, blocking:
 *   PT_DENOISE_LINEAR: linear RGBA32F in accumulation order, w*h*16 bytes;
 *   PT_DISPLAY_RGBA32F / PT_DISPLAY_SRGB8: through the display pass, with
 *     pt_display's byte sizes and row orders.
 * PT_ERR_STATE while the guides are not valid; PT_ERR_INVALID for a NULL p, a
 * bad format, iterations or normal_power_log2 out of range, a negative or
 * non-finite sigma, or one whose kc_i / kz_i / ka is not finite; PT_ERR_SIZE
 * as pt_display. */
#define PT_DENOISE_LINEAR 2
#define PT_DENOISE_MAX_ITERATIONS 8
int pt_denoise(pt_ctx *ctx, const pt_denoise_params *p, int format, void *out, size_t bytes);
/* Second moments, variance and the variance-guided filter (new; DESIGN.md 3.28
 * has the f32 steps).  With option "moments" on, every writing path-traced
 * dispatch (debug == 0) mixes each frame's squared colour into a second
 * RGBA32F image M of the accumulation image's size and order, with the weights
 * the accumulation image A is mixed with (alpha 1, texels the context does not
 * own stay 0).  The binned pipeline and the simple kernel keep it; the wave
 * kernel does not: "kernel" 0 then resolves to the binned pipeline whatever
 * the size, and "kernel" 2 makes pt_dispatch return PT_ERR_UNSUPPORTED with
 * both images untouched.  M and A are "valid" together, for n frames: a
 * dispatch with moments on and debug == 0 sets n = last_clear + spp when
 * last_clear == 0, or when they were valid with n == last_clear; any other
 * writing dispatch, pt_write_accum, pt_resize_clear, pt_set_tiles and
 * switching the option off end it (the last two clears zero M as well);
 * pt_dispatch_stats touches nothing.
 * pt_read_moments: blocking copy of M (w*h*4 floats); PT_ERR_STATE unless valid. */
int pt_read_moments(pt_ctx *ctx, float *rgba, size_t bytes);
/* Replace M, say it holds `frames` frames of the accumulation image as it is
 * now, and set valid (after pt_write_accum: resume a saved render, or hand
 * over the host sum of a multi-rank render's images and moments).
 * PT_ERR_STATE with the option off, PT_ERR_INVALID for frames == 0. */
int pt_write_moments(pt_ctx *ctx, const float *rgba, size_t bytes, uint32_t frames);
/* Variance of the mean per pixel, w*h floats in the image's order:
 *   v.k = max(M.k - A.k * A.k, 0) / float(n - 1), V = (v.r + v.g) + v.b
 * (a NaN difference counts as 0).  Blocking.  PT_ERR_STATE unless valid with
 * n >= 2. */
int pt_read_variance(pt_ctx *ctx, float *v, size_t bytes);
/* pt_denoise with the colour term steered by the variance: pixel p's taps are
 * divided by (1 + |dcolour|^2 kc_p), kc_p = 1 / (sigma_variance^2 g_p + 1e-10),
 * g_p the 3x3-smoothed variance at p; the variance is filtered beside the
 * colour with the squared weights, so later iterations see what is left. */
typedef struct pt_guided_params { /* 20 bytes */
    uint32_t iterations;         /* 1..8 */
    uint32_t normal_power_log2;  /* 0..8 */
    float sigma_variance;        /* finite, > 0: larger smooths more */
    float sigma_depth;           /* doubled every iteration; 0 = term off */
    float sigma_albedo;          /* 0 = term off */
} pt_guided_params;
/* Formats, output sizes, buffer rules and refusals as pt_denoise; also
 * PT_ERR_STATE without valid moments of n >= 2 frames and PT_ERR_INVALID for
 * a sigma_variance that is not finite or <= 0.  Reads A and M, writes neither. */
int pt_denoise_guided(pt_ctx *ctx, const pt_guided_params *p, int format, void *out, size_t bytes);
/* Temporal accumulation with reprojection (new; DESIGN.md 3.30 has the f32
 * steps).  A context keeps a history of its own size: colour H and second
 * moment HM (RGBA32F), a sample count HN per pixel (f32), and a copy of the
 * guide planes with the camera, aspect and fov they were rendered with --
 * what has been accumulated, seen from the view of the last accumulate.
 * pt_temporal_accumulate merges the current view into it: the image A and its
 * moments M (valid, n >= 2 frames) with the valid guides of pt_render_guides.
 * A hit pixel's first-hit point is projected into the history's view; the four
 * history texels around it are gathered bilinearly, each one only if it is a
 * hit with a finite history whose own first-hit point lies within
 * depth_tolerance * (the point's distance to the previous eye) of the pixel's
 * tangent plane, whose normal agrees (dot >= normal_cos) and whose albedo is
 * within albedo_tolerance.  What is gathered counts as min(its samples,
 * max_history) samples beside the n of the current view; a pixel that gathers
 * nothing starts again from the current view.  The result is the new history,
 * in the current view. */
typedef struct pt_temporal_params { /* 16 bytes */
    float max_history;        /* finite, >= 0: the most samples a pixel's history may weigh; 0 = history ignored */
    float depth_tolerance;    /* finite, >= 0: plane distance allowed, as a share of the point's distance to the previous eye */
    float normal_cos;         /* in [-1, 1] */
    float albedo_tolerance;   /* finite, >= 0 */
} pt_temporal_params;
/* Asynchronous, on the context's stream; reads A, M and the guides and writes
 * none of them (a render goes on afterwards as if it had not been called).
 * The first call, and the first after the history was dropped, makes the
 * history a copy of the current view.  The history's buffers (two sets: the
 * kernel gathers from one while it writes the other) are allocated at the
 * first call.  PT_ERR_INVALID for a NULL or out-of-range parameter;
 * PT_ERR_UNSUPPORTED while pt_set_tiles leaves the context part of the image
 * (a multi-rank render writes its reduced image and moments into a context
 * first, as for the denoisers); PT_ERR_STATE without valid guides or without
 * valid moments of n >= 2 frames.  A refused call leaves the history as it
 * was.  pt_temporal_reset, pt_set_program, pt_set_data and a pt_resize_clear
 * to another size drop the history; pt_set_camera, pt_set_sky, pt_set_tiles,
 * option and settings changes, dispatches and a pt_resize_clear at the same
 * size (a clear) do not: a caller who changes the light follows it with
 * pt_temporal_reset, as they follow it with a clear. */
int pt_temporal_accumulate(pt_ctx *ctx, const pt_temporal_params *p);
int pt_temporal_reset(pt_ctx *ctx);
/* Blocking copy of the history: colour and moments w*h*4 floats each
 * (bytes_rgba bytes at least), count w*h floats.  Any pointer may be NULL.
 * PT_ERR_STATE without a history. */
int pt_read_history(pt_ctx *ctx, float *colour, float *moments, float *count, size_t bytes_rgba);
/* pt_denoise_guided's filter over the history: the colour source is H, the
 * guides are the history's own copy (so it works after pt_set_camera has
 * invalidated the live ones), and the variance plane is
 *   v.k = max(HM.k - H.k * H.k, 0) / (HN - 1), V = (v.r + v.g) + v.b.
 * Formats, sizes, parameters and refusals as pt_denoise_guided, with
 * PT_ERR_STATE for "no history" in place of its two state rules. */
int pt_denoise_history(pt_ctx *ctx, const pt_guided_params *p, int format, void *out, size_t bytes);
/* Mesh export (new; DESIGN.md 3.27 has the f32 steps and the orders).
 * Field sampling: map() at n caller points (xyz, 3 floats each) with every
 * check[] entry true (no bounds() cull).  d[i] = distance, shape[i] = ordinal
 * of the PT_OP_SHAPE op whose material map() returns (Hit.m - 1), -1 = none
 * (MDEF).  A point with a non-finite coordinate is mapped as (NaN, NaN, NaN),
 * which is what the reference's full rotation matrices make of it.  Either
 * output may be NULL.  Blocking.  n = 0 is a no-op.  PT_ERR_STATE without
 * program or data. */
int pt_sample_field(pt_ctx *ctx, const float *xyz, uint32_t n, float *d, int32_t *shape);
/* Surface-nets mesh of {p : map(p) = iso} on a caller-given grid of cubic
 * cells: one vertex per cell the surface crosses (the mean of the crossings
 * on its edges, then `project` Newton steps along the normal, clamped into
 * the cell), one quad (two triangles, wound outward) per interior grid edge
 * whose endpoints differ in sign. */
#define PT_MESH_BRICK 8        /* cells per brick edge: the unit of the skip test and of the vertex order */
#define PT_MESH_MAX_CELLS 1024 /* per axis */
#define PT_MESH_MAX_PROJECT 8
typedef struct {          /* 36 bytes */
    float origin[3];      /* grid corner (0,0,0) */
    float cell;           /* edge length, finite, > 0 */
    uint32_t cells[3];    /* 1..1024 per axis */
    float iso;            /* inside <=> map(p) < iso; 0 = the scene's surface */
    uint32_t project;     /* 0..8 projection steps per vertex */
} pt_mesh_desc;
typedef struct {          /* 48 bytes */
    uint32_t n_vertices, n_triangles;
    uint32_t clipped_edges;    /* sign-changing edges on the grid's boundary: emit nothing; > 0 = the box cuts the surface */
    uint32_t void_cells;       /* cells with a non-finite corner value: no vertex */
    uint32_t dropped_quads;    /* interior sign-changing edges next to a void cell */
    uint32_t bricks, bricks_evaluated;   /* 8x8x8-cell bricks (PT_MESH_BRICK 8); evaluated = not skipped */
    uint32_t reserved;         /* 0 */
    uint64_t corner_evals;     /* map() calls on grid corners (skip tests not counted) */
    uint64_t device_bytes;     /* working memory held by the extractor */
} pt_mesh_info;
/* Blocking; the result stays in the context, a snapshot that pt_mesh_read
 * returns until the next pt_mesh_extract or pt_destroy (scene edits do not
 * invalidate it).  The accumulation image, guides, camera, sky and options
 * are untouched.  PT_ERR_INVALID (the previous mesh stays) for a NULL
 * argument, a non-finite origin / cell / iso, cell <= 0, a cells[] entry
 * outside 1..1024 or project > 8; PT_ERR_STATE without program or data;
 * PT_ERR_UNSUPPORTED if vertices or triangles would reach 2^31. */
int pt_mesh_extract(pt_ctx *ctx, const pt_mesh_desc *g, pt_mesh_info *info);
/* The last extracted mesh: positions and normals 3 floats per vertex, shapes
 * one ordinal per vertex (as pt_sample_field's), triangles 3 vertex indices
 * each; the caps count vertices and triangles.  Any pointer may be NULL.
 * Blocking.  PT_ERR_STATE before any extract; PT_ERR_SIZE (nothing written) if
 * a cap is too small for an array that is asked for. */
int pt_mesh_read(pt_ctx *ctx, float *positions, float *normals, int32_t *shapes, uint32_t *triangles,
                 size_t vertex_cap, size_t triangle_cap);
/* Ray queries (new): what a ray hits.  For one ray (ro, rd):
 *   a non-finite component among the six: t = NaN, shape = -1, n = (0, 0, 0)
 *     (answered by definition, not traced);
 *   check = bounds(ro, rd); (t, m) = CastRay(ro, rd, check)   (STEPS, MHD, FP
 *     of the reference); hit = !(t > FP) (a NaN t is a hit, as in the render);
 *   hit:  n = calc_normal(ro + rd * t, check) (what pt_render_guides stores in
 *         g0.xyz), shape = ordinal of the PT_OP_SHAPE op (as pt_sample_field's,
 *         -1 = MDEF);
 *   miss: n = (0, 0, 0), shape = -1, t as CastRay returned it.
 * rd is used as given, not normalised: t is the march parameter, so a
 * direction longer than 1 oversteps the surface and a shorter one creeps; a
 * zero direction marches in place until t > FP or 80 steps.  No random
 * numbers; pt_set_tiles, the debug view, the sky, the accumulation image, the
 * guides and their valid flag neither enter nor change: only the outputs are
 * written.
 * pt_trace_rays: n caller rays, ro and rd 3 floats each; t and shape one
 * value per ray, normal 3 floats per ray.  Any output may be NULL.  Blocking,
 * on the context's stream.  n = 0 is a no-op.  PT_ERR_INVALID for a NULL
 * context, NULL ro or rd (n > 0) or n > PT_RAYS_MAX (refused before anything
 * is read); PT_ERR_STATE without program or data.
 * pt_pick_pixels: the same for the jitter-free primary rays of n pixels, xy 2
 * ints each (x, y), under the camera in force with a lens taken as its
 * pinhole, aspect from c and fov from s: the rays of pt_render_guides, so
 * (normal, t) of a pixel equal its g0 bit for bit and its shape's albedo is
 * g1.rgb.  xy = NULL means every pixel in image order (row y, then x) and n
 * must be width * height: the shape-id image.  PT_ERR_INVALID also for NULL c
 * or s, for a NULL list with another n and for a listed pixel outside the
 * image (checked before any launch: nothing is written). */
#define PT_RAYS_MAX 67108864 /* 1u << 26 rays or pixels per call */
int pt_trace_rays(pt_ctx *ctx, const float *ro, const float *rd, uint32_t n, float *t, int32_t *shape, float *normal);
int pt_pick_pixels(pt_ctx *ctx, const pt_constants *c, const pt_settings *s, const int32_t *xy, uint32_t n, float *t,
                   int32_t *shape, float *normal);
/* Radiance queries (new): the light the path tracer computes
 * along caller rays -- a light meter, an irradiance probe, a vertex to bake.
 * n rays, ro and rd 3 floats each; p->spp samples per ray; mean and moment 3
 * floats per ray, either may be NULL.  Per ray i and sample index
 * k = p->sample0 + s, s in [0, spp):
 *   rng = ((i * 1973 + seed * 9277 + k * 26699) mod 2^32) | 1: gen_rng's form
 *     with the ray index, the caller's seed and the sample index for a, b and
 *     frame; no jitter draw, no lens draw;
 *   PT_RADIANCE_RAY: colour = path_trace(ro, rd, rng, bounces), debug 0, with
 *     the sky in force (pt_set_sky: unlike the ray queries, this is a render);
 *     rd is used as given, not normalised, as pt_trace_rays uses it;
 *   PT_RADIANCE_HEMISPHERE: rd is a surface normal.  Two draws first, in the
 *     order and f32 steps of the path's diffuse direction: uz = f01 * 2 - 1,
 *     ua = f01 * 2pi, ur = sqrt(1 - uz * uz), (sa, ca) = sincos(ua),
 *     d = normalize(rd + (ur * ca, ur * sa, uz)), then
 *     colour = path_trace(ro, d, rng, bounces).  With a unit rd the directions
 *     are cosine-distributed about it, so the mean estimates irradiance / pi;
 *     a zero rd gives the uniform sphere;
 *   the colours enter the ray's running values in the order of k with the
 *     image's mix, last_clear = k: w = 1 / float(k + 1), mean = mean * (1 - w)
 *     + colour * w, moment = moment * (1 - w) + colour * colour * w per channel
 *     -- the bits an accumulation texel and its moment texel hold after the
 *     same colours.  sample0 = 0: mean and moment are outputs only;
 *     sample0 > 0: they are read as the running values first (in / out), so a
 *     call of 8 samples equals one of 3 then one of 5 with sample0 = 3;
 *   a non-finite colour enters the mix as it does in the image; a ray with a
 *     non-finite component among its six is not marched: its mean and moment
 *     are NaN in all channels, for any sample0.
 * Nothing else is read or written: the image, the moments, the guides and
 * their valid flag, the history, the mesh, the camera and pt_set_tiles neither
 * enter nor change.  Blocking, on the context's stream.  Device memory does not
 * grow with n * spp: the rays are walked in chunks of whole rays, at most
 * "radiance_samples" samples in flight; the results are the same bits for every
 * value of it.  n = 0 is a no-op.  Refused, in this order, before anything is
 * read or written: PT_ERR_INVALID for a NULL context or p; for
 * n > PT_RAYS_MAX; for NULL ro or rd (n > 0); for spp outside
 * [1, PT_RADIANCE_MAX_SPP], sample0 + spp > 1 << 24, bounces < 0 or an unknown
 * mode; for sample0 > 0 with a NULL mean or moment (a continuation needs
 * both); PT_ERR_STATE without program or data.  The ahead-of-time interpreter
 * serves it for every scene (no scene-specialised variant). */
#define PT_RADIANCE_RAY 0        /* the sample's first segment is (ro, rd) as given */
#define PT_RADIANCE_HEMISPHERE 1 /* rd is a surface normal: each sample's first direction is drawn about it */
#define PT_RADIANCE_MAX_SPP 65536
typedef struct pt_radiance_params { /* 20 bytes */
    uint32_t spp;     /* 1..PT_RADIANCE_MAX_SPP samples added by this call */
    uint32_t sample0; /* samples the in/out arrays already hold; 0 = start; sample0 + spp <= 1 << 24 */
    uint32_t seed;    /* caller's stream */
    int32_t bounces;  /* >= 0, as pt_settings.bounces */
    int32_t mode;     /* PT_RADIANCE_* */
} pt_radiance_params;
int pt_trace_radiance(pt_ctx *ctx, const float *ro, const float *rd, uint32_t n, const pt_radiance_params *p, float *mean,
                      float *moment);
/* Preview shading (new): a noise-free lit image for a viewport
 * -- one primary ray per pixel, a key light with a sphere-traced soft shadow,
 * five distance taps of ambient occlusion, a hemisphere ambient term.  No
 * random numbers, no accumulation, no history.  One RGBA32F texel per pixel of
 * the context's size, every pixel whatever pt_set_tiles says, under the camera
 * in force with a lens taken as its pinhole, aspect from c and fov from s: the
 * rays of pt_render_guides.  Every step is one f32 operation in the order
 * written, nothing contracted; gmin / gmax are fminf / fmaxf (a NaN operand is
 * dropped); map(p, ck).d is the interpreted map() under the check[] set ck,
 * "all" every entry set (as pt_sample_field); l = light_dir as given, not
 * normalised.  For pixel (x, y):
 *   (ro, rd) = the pixel's jitter-free primary ray; (t, n, mat) = its first hit
 *     (bounds, CastRay, calc_normal normalised: n and t are g0's bits);
 *   miss (t > FP): rgb = sky_radiance(rd) with a sky set (pt_set_sky), else 0;
 *     alpha 0;
 *   hit (a NaN t is a hit): hp = ro + rd * t; q = hp + n * 0.03;
 *     ndl = gmax((n.x * l.x + n.y * l.y) + n.z * l.z, 0);
 *     shadow: sh = 1; only if shadow_steps > 0 and ndl > 0: ck = bounds(q, l)
 *       with shadow_cull, else all; s = 0.05; at most shadow_steps times:
 *       d = map(q + l * s, ck).d; if d < 0.001: sh = 0, stop;
 *       sh = gmin(sh, (shadow_k * d) / s); s = s + gmax(d, 0.02);
 *       if s > 100: stop;
 *     occlusion: ao = 1; only if ao_strength > 0: occ = 0, w = 1; for i = 0..4:
 *       h = 0.01 + ao_radius * (float(i) * 0.25); d = map(hp + n * h, all).d;
 *       occ = occ + (h - d) * w; w = w * 0.95;
 *       then ao = gmin(gmax(1 - ao_strength * occ, 0), 1);
 *     light: u = n.y * 0.5 + 0.5; per channel k:
 *       amb = ambient_bottom + (ambient_top - ambient_bottom) * u;
 *       lit = ndl * sh;
 *       c = (col * ((amb * ao) + (light_color * lit))) + emis, col and emis
 *       the hit material's albedo and emission (normalize(light) * brightness);
 *     highlight: if highlight >= 0 and the hit shape's PT_OP_SHAPE ordinal (as
 *       pt_pick_pixels reports it) equals it:
 *       c = c + (highlight_color - c) * highlight_mix;
 *     alpha 1.
 * A NaN distance leaves sh as it is and steps on by 0.02; a NaN occ gives
 * ao = 0; the only non-finite outputs are those the material or the sky
 * carries.  The shadow march runs at all checks by default: its penumbra term
 * needs the shapes near the ray, and bounds() knows only those whose box the
 * ray's line enters, so shadow_cull = 1, the cheaper variant, cuts penumbrae
 * at box silhouettes.  The occlusion taps are always at all checks.
 * Formats, output sizes and row orders are pt_denoise's: PT_DENOISE_LINEAR, or
 * PT_DISPLAY_RGBA32F / PT_DISPLAY_SRGB8 (the preview through the display
 * pass).  Blocking, on the context's stream; out is caller-owned.  It writes
 * its own 16 B per pixel device buffer (and the display pass's output buffer),
 * held in the context from the first call on, and nothing else: the image, the
 * moments, the guides and their valid flag, the history, the mesh, the camera
 * and the sky neither change nor enter, except that the sky is read.  Refused,
 * in this order, before anything is read or written: PT_ERR_INVALID for a NULL
 * context, c, s or p, a bad format, or a field outside the ranges below (any
 * non-finite float is); PT_ERR_STATE without program or data; PT_ERR_SIZE for
 * a NULL or short out, as pt_display.  The ahead-of-time interpreter serves it
 * for every scene (no scene-specialised variant). */
#define PT_PREVIEW_MAX_SHADOW_STEPS 64
typedef struct pt_preview_params { /* 88 bytes, 22 words */
    float light_dir[3], light_color[3];
    float ambient_bottom[3], ambient_top[3];
    uint32_t shadow_steps; /* 0..PT_PREVIEW_MAX_SHADOW_STEPS; 0 = no shadow */
    float shadow_k;        /* finite, > 0: larger = harder edge */
    uint32_t shadow_cull;  /* 0 | 1 */
    float ao_strength;     /* finite, >= 0; 0 = no taps */
    float ao_radius;       /* finite, >= 0 */
    int32_t highlight;     /* PT_OP_SHAPE ordinal as pt_pick_pixels reports it; -1 = none */
    float highlight_color[3];
    float highlight_mix;   /* in [0, 1] */
} pt_preview_params;
int pt_render_preview(pt_ctx *ctx, const pt_constants *c, const pt_settings *s, const pt_preview_params *p,
                      int format, void *out, size_t bytes);
/* Tuning knobs: "kernel" (0 auto = 3, 1 simple one-path-per-lane, 2 tile-
 * resident wavefront state machine, 3 mask-binned passes: per bounce, the
 * rays of a chunk of frames are grouped by their bounds() check set before
 * they are marched), "shade_batch" (state-machine kernels: lanes that must
 * wait before a shading pass runs, 1..64), "bin_samples" (binned kernel:
 * samples per chunk, >= 64; device memory = 168 B per sample, 192 B for
 * scenes with > 64 check[] entries; default 2^29 samples, at most half of
 * the device's total memory -- or, when that does not fit beside other
 * contexts on the same GPU, half of what this context could hold -- fixed at
 * the context's first binned dispatch), "bin_lanes"
 * (binned kernel: 1..4 pipelines, each on its own stream, over which a
 * chunk's frames are split, so one's memory-bound passes overlap another's
 * trace pass), "bin_table" (binned kernel, scenes with 13..64 check[]
 * entries: 1, the default, bins each set in a slot of its own from a table
 * of the sets seen; 0: hashed bins, which two sets share now and then), "jit" (1:
 * per-scene hipRTC build of the state-machine kernels, compiled at
 * pt_set_data when the topology or an identity flag changed -- the analogue
 * of remake_pipeline; 0: op-list interpreter), "jit_bake" (0: node values
 * read from the table; 1: baked into the kernel as literals, recompiled on
 * every value edit; 2, the default: tier-up -- the table kernel runs at
 * once, and a values-baked build compiled on a worker thread replaces it
 * while the values stay unchanged) and "jit_wait" (block until a pending
 * tier-up build is installed) and "denoise_lds" (pt_denoise: 1, the default,
 * stages a block's tile and halo in LDS for the iterations of step 1 and 2;
 * 0 loads every tap directly) and "mesh_skip" (pt_mesh_extract: 1, the
 * default, skips a brick whose centre value proves it holds no surface; 0
 * evaluates every brick) and "radiance_samples" (pt_trace_radiance: samples
 * in flight per chunk of whole rays, 65536..2^28, default 2^22; device memory
 * = 16 B per sample).  Results are bit-identical for every value.
 * "moments" (0, the default: a dispatch launches what it always did; 1: the
 * second-moment image above is kept -- the image itself does not change). */
int pt_set_option(pt_ctx *ctx, const char *key, int value);
/* Read back: "jit_active" (1 when the scene-specialised kernel is loaded),
 * "jit_seconds" (last hipRTC compile time), "jit_tier_active" /
 * "jit_tier_seconds" (values-baked build in use / its compile time),
 * "kernel", "shade_batch",
 * "bin_samples", "bin_lanes", "bin_table", "bin_bytes" (device memory held by the binned
 * pipeline), "bin_chunks" (chunks of the last binned dispatch), "bin_fallback"
 * (1: the chunk size came from the free memory), "trace_ms" / "trace_launches" (device time and count of the last
 * dispatch's binned trace passes, HIP events on each pipeline's stream),
 * "shade_ms" / "shade_launches" (the same for its shade passes), "sky_ms" /
 * "sky_launches" (the same for its sky passes, pt_set_sky; 0 without a sky), "display_ms"
 * (device time of the last pt_display's kernel), "guide_ms" / "denoise_ms"
 * (device time of the last pt_render_guides' kernel / of all iterations of the
 * last pt_denoise, without its display pass), "mesh_skip", "sample_ms" (the
 * last pt_sample_field's kernel), "mesh_ms" (the last pt_mesh_extract's
 * kernels, the sum of "mesh_skip_ms", "mesh_classify_ms", "mesh_scan_ms" and
 * "mesh_emit_ms"), "rays_ms" / "pick_ms" (the last pt_trace_rays' /
 * pt_pick_pixels' kernel), "radiance_samples", "radiance_ms" (device time of
 * the last pt_trace_radiance's kernels, summed over its chunks),
 * "radiance_first_ms" (the shared first segments' part of it; 0 in hemisphere
 * mode), "radiance_bytes" (device memory the radiance queries hold),
 * "preview_ms" (device time of the last pt_render_preview's kernel, without
 * its display pass),
 * "guides_valid", "moments", "moments_valid", "moment_frames"
 * (n; 0 while not valid), "variance_ms" (the last variance kernel, of
 * pt_read_variance or pt_denoise_guided), "guided_ms" (all iterations of the
 * last pt_denoise_guided, as "denoise_ms"), "history_valid", "history_views"
 * (the accumulates since the history was last dropped), "temporal_ms" (the last
 * pt_temporal_accumulate's kernel), "history_variance_ms" / "history_denoise_ms"
 * (the last pt_denoise_history's variance kernel / all its iterations),
 * "gen_trace" / "gen_norec"
 * (the last timed binned dispatch's first pass made its own camera rays /
 * and stored no ray records for shade pass 0). */
int pt_get_option(pt_ctx *ctx, const char *key, double *value);
/* Log of the last failed scene-kernel build ("" if none). */
const char *pt_jit_log(const pt_ctx *ctx);
/* Build the scene-specialised kernel for (program, data) with hipRTC without
 * a device (validation / cache warm-up); *code_bytes = code object size. */
int pt_jit_compile(const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb, const float *data,
                   uint32_t n_data, char *log, size_t log_cap, size_t *code_bytes);
/* The scene kernel source pt_jit_compile would build for (program, data),
 * without compiling it (the counterpart of the reference's spliced-shader dump
 * shader_out/test_compute.glsl, glsl_preprocessor.rs:5-15).  baked != 0: node
 * values as literals (the tier-up build).  Host only; two-call pattern, *len
 * includes the terminating NUL. */
int pt_scene_kernel_source(const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb,
                           const float *data, uint32_t n_data, int baked, char *out, size_t cap, size_t *len);
const char *pt_last_error(const pt_ctx *ctx);
void pt_destroy(pt_ctx *ctx);
int pt_abi_version(void);

/* Device arithmetic probes for the semantics contract (tests only):
 * out[i] = op(a[i], b[i]) computed by the kernels' own device functions. */
#define PT_MATH_MAX 0
#define PT_MATH_MIN 1
#define PT_MATH_SQRT 2   /* the kernels' fast correctly rounded sqrt */
#define PT_MATH_SQRTF 3  /* the compiler's IEEE sqrtf */
#define PT_MATH_SIN 4
#define PT_MATH_COS 5
#define PT_MATH_DIV 6
#define PT_MATH_FMA 7    /* fmaf(a, b, 1) */
int pt_device_math(int hip_device, int op, const float *a, const float *b, float *out, uint32_t n);
/* The kernels' sqrt vs IEEE sqrtf over all 2^32 inputs (NaN payloads aside). */
int pt_check_sqrt_exhaustive(int hip_device, uint64_t *mismatches, uint32_t *first_bad);
/* bounds()' reciprocal division (q = a*y, r = fma(-q,b,a), fma(r,y,q) with
 * y = 1/b) vs IEEE a / b for every a = 1.(a0..a0+na-1), b = 1.(b0..b0+nb-1)
 * significand pair (na, nb <= 2^23); first_bad = b bits << 32 | a bits. */
int pt_check_div_exhaustive(int hip_device, uint32_t a0, uint32_t na, uint32_t b0, uint32_t nb,
                            uint64_t *mismatches, uint64_t *first_bad);
/* The same on n random operands drawn inside the bounds() guards (a = x - o
 * of two guarded coordinates, guarded divisor); a zero quotient may differ in
 * sign only. */
int pt_check_div_random(int hip_device, uint32_t seed, uint32_t n, uint64_t *mismatches, uint64_t *first_bad);
/* The margin-decided slab test of bounds() on n random
 * guarded (box, ray) pairs; mode 1 puts the ray through a box edge (near
 * ties).  counts[0]: decided pairs whose answer differs from the IEEE slab
 * test, [1]: undecided pairs whose exact fallback differs, [2]: undecided
 * pairs, [3]: pairs drawn outside the guards (skipped). */
int pt_check_box_random(int hip_device, uint32_t seed, uint32_t n, int mode, uint64_t *counts);
/* Self-test: pt_div_k(a, b, RN(1/b)) (the baked scene kernels' division by a
 * scale constant, |b| in [2^-4, 2^4]) against the IEEE a / b, bit for bit,
 * for the na patterns a0 .. a0 + na - 1 (na a multiple of 256). */
int pt_check_div_k(int hip_device, float b, uint32_t a0, uint32_t na, uint64_t *mismatches, uint64_t *first_bad);
/* Calibration probes for rocprofv3's FETCH_SIZE / WRITE_SIZE on the
 * pipeline's access shapes (pt_probe.hip): 2^log2n items (16..26) of, in
 * order, a 64 B record gather, a 16 B coalesced read, a 16 B scattered store
 * and a 64 B record store; ms[k] = device time, bytes[k] = bytes moved. */
int pt_traffic_probe(int hip_device, uint32_t log2n, float ms[4], uint64_t bytes[4]);

/* Point probes (tests only): the scene's map() and bounds() on
 * caller-supplied inputs, one thread per input in 64-thread waves, results
 * per input.  kind: PT_PROBE_INTERP runs the ahead-of-time interpreter
 * (InterpMap, bounds_mask); PT_PROBE_TABLE / PT_PROBE_BAKED run the scene's own
 * generated code -- the text of pt_scene_kernel_source up to its kernel list,
 * values read from the node table / baked as literals -- under probe kernels
 * in modules of their own (that text and the one kernel a call runs),
 * compiled with hipRTC at the first call that needs them, once per distinct
 * source per context (pt_get_option "probe_compiles", "probe_seconds"),
 * outside the on-disk cache.  The pipeline kernels are not
 * what runs here: the image tests remain the check of those as compiled.
 * Blocking.  n = 0 is a no-op.  PT_ERR_INVALID for a NULL context, a missing
 * input or a value outside the defines; PT_ERR_STATE without program or
 * data; PT_ERR_HIP when the probe module does not build (pt_jit_log has the
 * compile log).  Every lane of a wave takes part in the wave-level steps; the
 * lanes beyond n carry an empty mask.  counters (PT_STAT_COUNT words, may be
 * NULL): the call's work counters, as pt_dispatch_stats counts; with
 * counters the instrumented build of the same code runs. */
#define PT_PROBE_INTERP 0
#define PT_PROBE_TABLE 1
#define PT_PROBE_BAKED 2
#define PT_PROBE_MAP 0     /* JitMap: the march steps' map() */
#define PT_PROBE_MAP_B0 1  /* JitMapB0: the shade pass's first tap (bound rule, records `live`) */
#define PT_PROBE_MAP_B1 2  /* JitMapB1: its other five taps (evaluates what `live` names) */
/* One map() call per point.  check: [n][2] check[] bits 0..63 and 64..127
 * (NULL: every bit set); bnd: [n] the map() bound of the B variants (NULL:
 * +inf; NaN: rule off), widened about the point itself as the shade pass
 * widens it about the hit; live_in: [n] (NULL: 0).  union_mode 0: the wave's
 * union of masks is "no information" (all ones); 1: the OR of the wave's
 * masks, as the trace pass forms it.  d, shape (as pt_sample_field's) and
 * live_out may each be NULL.  A point with a non-finite coordinate is mapped as
 * (NaN, NaN, NaN), as pt_sample_field maps it. */
int pt_probe_map(pt_ctx *ctx, int kind, int variant, uint32_t n, const float *xyz, const uint64_t *check,
                 const float *bnd, const uint64_t *live_in, int union_mode, float *d, int32_t *shape,
                 uint64_t *live_out, uint64_t *counters);
/* The shade pass's six normal taps around each hit point, in its order (+x,
 * -x, +y, -y, +z, -z at 1e-4): d6 / shape6 [n][6], live [n] = the live mask
 * the first tap recorded.  Each output may be NULL. */
int pt_probe_taps(pt_ctx *ctx, int kind, uint32_t n, const float *hit, const uint64_t *check, const float *bnd,
                  float *d6, int32_t *shape6, uint64_t *live, uint64_t *counters);
/* bounds() per ray: mask [n][4], check[] bit k = word k / 32, bit k % 32.
 * skip_mode 1: each full wave of 64 rays first asks which boxes none of its
 * rays can hit (the first pass's primary_box_skip) and leaves those out;
 * skip [ceil(n / 64)] = that word per wave (0 for a ragged wave; may be NULL). */
int pt_probe_bounds(pt_ctx *ctx, int kind, uint32_t n, const float *ro, const float *rd, int skip_mode,
                    uint32_t *mask, uint64_t *skip, uint64_t *counters);
/* The probe module's source for (program, data), as pt_scene_kernel_source
 * returns the scene kernels' (host only, same two-call pattern). */
int pt_probe_kernel_source(const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb,
                           const float *data, uint32_t n_data, int baked, char *out, size_t cap, size_t *len);
/* Build that source as pt_probe_map builds it, without a device (validation):
 * log = the compile log, *code_bytes = code object size. */
int pt_probe_jit_compile(const pt_op *ops, uint32_t n_ops, const pt_aabb *aabbs, uint32_t n_aabb, const float *data,
                         uint32_t n_data, int baked, char *log, size_t log_cap, size_t *code_bytes);

#ifdef __cplusplus
}
#endif
#endif
