"""Host mirror of the reference's ``PathTracer`` (src/path_tracer/path_tracer.rs).

Same public surface -- ``new``/``remake_pipeline``/``update``/``compute_pass``,
the ``Constants``/``Settings`` blocks with the reference defaults, the
``changed`` flag -- but the wgpu pipeline, UBOs and storage texture are
replaced by one native context (``include/pt_abi.h``) driving the HIP kernel.
``render(spp)`` is the batched form: it is exactly ``spp`` repetitions of
``update()`` + ``compute_pass()`` with no reset in between, executed as one
launch that keeps the accumulation texel in registers.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import _native as N
from .mesh import Mesh, mesh_grid
from .sdf_editor import Program
from .view import look_at_camera, preview_light, sky_light


class RayHits(NamedTuple):
    """What ``trace_rays`` / ``pick_pixels`` / ``id_image`` return, each array
    shaped like the query's leading dimensions: ``t`` float32 (the march
    parameter; a miss keeps CastRay's value, > 100), ``hit`` bool
    (``~(t > 100)``: a NaN t is a hit, as in the render), ``shape`` int32 (the
    ordinal of the program's SHAPE op, -1 = none), ``normal`` float32 [..., 3]
    (zeros where not hit), ``point`` float32 [..., 3] (origin + direction * t,
    NaN rows where not hit)."""

    t: np.ndarray
    hit: np.ndarray
    shape: np.ndarray
    normal: np.ndarray
    point: np.ndarray


class Radiance(NamedTuple):
    """What ``trace_radiance`` / ``bake_mesh`` return: ``mean`` and ``moment``
    float32 [..., 3], the running mean of the samples' colours and of their
    squares per ray, shaped like the query's leading dimensions; ``samples``,
    how many they hold; ``mode`` ("ray" or "hemisphere").  A ray with a
    non-finite component has NaN rows."""

    mean: np.ndarray
    moment: np.ndarray
    samples: int
    mode: str

    @property
    def variance(self) -> np.ndarray:
        """The variance of the mean per ray, float32 [...]: the sum over r, g,
        b of max(moment - mean * mean, 0) / (samples - 1) -- pt_read_variance's
        formula in float32 on the host (the max drops a NaN; one sample has
        no estimate: NaN or inf)."""
        F = np.float32
        with np.errstate(all="ignore"):
            v = np.fmax(self.moment - self.mean * self.mean, F(0.0)) / F(self.samples - 1)
            return (v[..., 0] + v[..., 1]) + v[..., 2]


class Pick(NamedTuple):
    """One pixel's ``pick``: ``hit``, ``t``, ``point`` and ``normal`` (float32
    [3]), ``shape`` (ordinal, -1 = none) and ``node``, the editor's ``Shape``
    behind it (None on a miss or without an editor)."""

    hit: bool
    t: float
    point: np.ndarray
    normal: np.ndarray
    shape: int
    node: object


def default_settings() -> N.Settings:
    """defaults_and_sliders_gui!(Settings, ...) (path_tracer.rs:157-163)."""
    return N.Settings(debug=1, bounces=8, scale=1.0, fov=1.0, aabb=0)


class PathTracer:
    def __init__(self, width: int, height: int, program: Optional[Program] = None, data: Optional[np.ndarray] = None,
                 device: int = 0, settings: Optional[N.Settings] = None, options: Optional[dict] = None):
        """PathTracer::new (path_tracer.rs:28-60) + the storage texture it binds
        (StorageTexturePackage::new, structs.rs:113-160).  ``width``/``height``
        are the window size; the image is window * settings.scale."""
        self._L = N.lib()
        self.window = (int(width), int(height))
        self.constants = N.Constants(time=0.0, frame=0, aspect=0.0, last_clear=0)
        self.settings = settings if settings is not None else default_settings()
        self.changed = False
        self.device = device
        self.size = self._scaled_size()
        ctx = ctypes.c_void_p()
        N.check("pt_create", self._L.pt_create(device, self.size[0], self.size[1], ctypes.byref(ctx)))
        self._ctx = ctx
        for k, v in (options or {}).items():
            self.set_option(k, v)
        if program is not None:
            self.remake_pipeline(program)
            self.set_data(program.data if data is None else data)

    # -- lifecycle -----------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._L.pt_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, fn: str, rc: int) -> None:
        N.check(fn, rc, self._ctx)

    def _scaled_size(self):
        s = np.float32(self.settings.scale)
        return (int(np.float32(self.window[0]) * s), int(np.float32(self.window[1]) * s))

    def _aspect(self) -> float:
        """The window's aspect in float32 (setup.rs:84-86)."""
        return float(np.float32(self.window[0]) / np.float32(self.window[1]))

    def _constants(self, ahead: int) -> N.Constants:
        """The Constants block ``ahead`` frames after the one in force."""
        return N.Constants(time=self.constants.time, frame=self.constants.frame + ahead, aspect=self._aspect(),
                           last_clear=self.constants.last_clear + ahead)

    def _image(self, dtype=np.float32, src=None):
        """(array, its pointer, its byte count) of an [height][width][4] image
        of ``dtype``: a fresh one to read into, or ``src`` checked to be one."""
        w, h = self.size
        if src is None:
            a = np.empty((h, w, 4), dtype=dtype)
        else:
            a = np.ascontiguousarray(src, dtype)
            if a.shape != (h, w, 4):
                raise ValueError(f"image must be ({h}, {w}, 4), got {a.shape}")
        return a, N.ptr(a, np.ctypeslib.as_ctypes_type(dtype)), a.nbytes

    # -- reference surface ---------------------------------------------------
    def remake_pipeline(self, program: Program) -> None:
        """path_tracer.rs:62-76: a topology change (queue_compile)."""
        self._chk("pt_set_program", self._L.pt_set_program(self._ctx, program.ops, program.n_ops, program.aabbs,
                                                            program.n_aabb, program.n_check))

    def set_data(self, data: np.ndarray) -> None:
        """DataArray::update (primitives.rs:131-151): value-only upload."""
        arr = np.ascontiguousarray(data, dtype=np.float32)
        self._chk("pt_set_data", self._L.pt_set_data(self._ctx, N.fptr(arr), arr.size))

    def update(self, resized: bool = False, reset: bool = False, time: float = 0.0,
               window: Optional[tuple] = None) -> None:
        """path_tracer.rs:97-118: reset on resize/settings change/Space, then
        advance frame and last_clear."""
        if window is not None:
            self.window = (int(window[0]), int(window[1]))
        if resized or self.changed or reset:
            self.size = self._scaled_size()
            self._chk("pt_resize_clear", self._L.pt_resize_clear(self._ctx, self.size[0], self.size[1]))
            self.constants.last_clear = 0
        self.constants.time = float(time)
        self.constants.aspect = self._aspect()
        self.constants.frame += 1
        self.constants.last_clear += 1
        self.changed = False

    def compute_pass(self) -> None:
        """path_tracer.rs:128-146: one frame (1 spp) with the current blocks."""
        self._chk("pt_dispatch", self._L.pt_dispatch(self._ctx, ctypes.byref(self.constants),
                                                      ctypes.byref(self.settings), 1))

    # -- batched / multi-GPU ----------------------------------------------
    def render(self, spp: int) -> None:
        """``spp`` x (update(); compute_pass()) without resets, one dispatch."""
        if spp <= 0:
            return
        if self.changed:
            self.update()
            self.constants.frame -= 1
            self.constants.last_clear -= 1
        c = self._constants(1)
        self.constants.aspect = c.aspect
        self._chk("pt_dispatch", self._L.pt_dispatch(self._ctx, ctypes.byref(c), ctypes.byref(self.settings), spp))
        self.constants.frame += spp
        self.constants.last_clear += spp

    def dispatch(self, constants: N.Constants, spp: int) -> None:
        """Raw pt_dispatch with explicit constants (frame j = frame + j)."""
        self._chk("pt_dispatch", self._L.pt_dispatch(self._ctx, ctypes.byref(constants), ctypes.byref(self.settings),
                                                      spp))

    def stats(self, constants: N.Constants, spp: int) -> dict:
        buf = (ctypes.c_uint64 * N.PT_STAT_COUNT)()
        self._chk("pt_dispatch_stats", self._L.pt_dispatch_stats(self._ctx, ctypes.byref(constants),
                                                                  ctypes.byref(self.settings), spp, buf))
        return dict(zip(N.STAT_NAMES, (int(v) for v in buf)))

    def tap_stats(self) -> dict:
        """The share of the last stats() run done by the shade pass's normal
        taps (shade_taps on; zeros otherwise)."""
        return {name: int(self.get_option(f"tap_stat_{k}")) for k, name in enumerate(N.STAT_NAMES)
                if k < N.PT_ST_COUNT}

    KERNELS = {"auto": 0, "simple": 1, "wave": 2, "jit": 2, "binned": 3}

    def set_option(self, key: str, value) -> None:
        if key == "kernel" and isinstance(value, str):
            value = self.KERNELS[value]
        self._chk("pt_set_option", self._L.pt_set_option(self._ctx, key.encode(), int(value)))

    def get_option(self, key: str) -> float:
        v = ctypes.c_double()
        self._chk("pt_get_option", self._L.pt_get_option(self._ctx, key.encode(), ctypes.byref(v)))
        return float(v.value)

    def jit_log(self) -> str:
        raw = self._L.pt_jit_log(self._ctx)
        return raw.decode() if raw else ""

    def set_tiles(self, rank: int, nranks: int) -> None:
        self._chk("pt_set_tiles", self._L.pt_set_tiles(self._ctx, rank, nranks))
        self._tiles = (int(rank), int(nranks))

    # -- camera (new: the reference's view is fixed) ------------------------
    def _set_camera(self, cam: Optional[N.Camera]) -> None:
        self._chk("pt_set_camera", self._L.pt_set_camera(self._ctx, ctypes.byref(cam) if cam is not None else None))
        self.changed = True  # the next update() clears the image, as for a settings change

    def set_camera(self, origin, right, up, forward, aperture: float = 0.0, focus: float = 1.0) -> N.Camera:
        """pt_set_camera: a primary ray leaves ``origin`` along
        normalize(right * ux + up * uy + forward * fov); ``aperture`` > 0 is a
        thin lens of that radius focused at distance ``focus``.  The basis is
        used as given (look_at builds an orthonormal one)."""
        cam = N.Camera(aperture=float(aperture), focus=float(focus))
        for name, v in (("origin", origin), ("right", right), ("up", up), ("forward", forward)):
            if len(v) != 3:
                raise ValueError(f"{name} must have three components, got {v!r}")
            for k in range(3):
                getattr(cam, name)[k] = float(v[k])
        self._set_camera(cam)
        return cam

    def look_at(self, eye, target, up=(0.0, 1.0, 0.0), aperture: float = 0.0, focus: Optional[float] = None) -> N.Camera:
        """Place the camera at ``eye`` looking at ``target`` (look_at_camera);
        returns the Camera it set."""
        cam = look_at_camera(eye, target, up, aperture, focus)
        self._set_camera(cam)
        return cam

    def reset_camera(self) -> None:
        """Back to the reference's fixed camera."""
        self._set_camera(None)

    def get_camera(self):
        """(Camera in force, True when it is the reference's fixed one)."""
        cam, dflt = N.Camera(), ctypes.c_int()
        self._chk("pt_get_camera", self._L.pt_get_camera(self._ctx, ctypes.byref(cam), ctypes.byref(dflt)))
        return cam, bool(dflt.value)

    # -- sky (new: in the reference a ray that leaves the scene adds nothing) --
    def _set_sky(self, sky: Optional[N.Sky]) -> None:
        self._chk("pt_set_sky", self._L.pt_set_sky(self._ctx, ctypes.byref(sky) if sky is not None else None))
        self.changed = True  # the next update() clears the image, as for a settings change

    def set_sky(self, bottom, top=None, sun_direction=None, sun_color=(0.0, 0.0, 0.0), sun_angle: float = 0.0) -> N.Sky:
        """pt_set_sky: light for rays that leave the scene -- a vertical
        gradient from ``bottom`` to ``top`` and a sun disc (sky_light's
        arguments), or a ready ``Sky`` as the only argument, passed on as it
        is.  Returns the Sky it set."""
        sky = bottom if isinstance(bottom, N.Sky) else sky_light(bottom, top, sun_direction, sun_color, sun_angle)
        self._set_sky(sky)
        return sky

    def clear_sky(self) -> None:
        """Back to the reference's void: a ray that leaves the scene adds nothing."""
        self._set_sky(None)

    def get_sky(self):
        """(Sky in force, True when none is set)."""
        sky, off = N.Sky(), ctypes.c_int()
        self._chk("pt_get_sky", self._L.pt_get_sky(self._ctx, ctypes.byref(sky), ctypes.byref(off)))
        return sky, bool(off.value)

    def clear(self) -> None:
        self._chk("pt_resize_clear", self._L.pt_resize_clear(self._ctx, self.size[0], self.size[1]))
        self.constants.last_clear = 0

    def sync(self) -> None:
        self._chk("pt_sync", self._L.pt_sync(self._ctx))

    def last_dispatch_ms(self) -> float:
        ms = ctypes.c_float()
        self._chk("pt_last_dispatch_ms", self._L.pt_last_dispatch_ms(self._ctx, ctypes.byref(ms)))
        return float(ms.value)

    def read_image(self) -> np.ndarray:
        """The accumulation image as float32 [height][width][4], row 0 = y 0."""
        out, p, nbytes = self._image()
        self._chk("pt_read_accum", self._L.pt_read_accum(self._ctx, p, nbytes))
        return out

    def write_image(self, img: np.ndarray) -> None:
        """Replace the accumulation image (pt_write_accum): float32 [h][w][4]."""
        _, p, nbytes = self._image(src=img)
        self._chk("pt_write_accum", self._L.pt_write_accum(self._ctx, p, nbytes))

    def display(self, srgb8: bool = False) -> np.ndarray:
        """The display pass (RenderTexturePipeline::render_pass,
        render_texture_shader.wgsl:23-94) on the device.  srgb8=False: fs_main's
        RGBA32F per texel [height][width][4], row 0 = bottom.  srgb8=True: the
        sRGB swapchain's 8-bit RGBA [height][width][4], row 0 = top of screen."""
        out, p, nbytes = self._image(np.uint8 if srgb8 else np.float32)
        fmt = N.PT_DISPLAY_SRGB8 if srgb8 else N.PT_DISPLAY_RGBA32F
        self._chk("pt_display", self._L.pt_display(self._ctx, fmt, p, nbytes))
        return out

    # -- denoiser (new: guide images + an edge-stopping a-trous wavelet) ------
    def render_guides(self, constants: Optional[N.Constants] = None) -> None:
        """pt_render_guides: the first-hit normal / depth / albedo images of
        the view in force (one jitter-free primary ray per pixel, a lens as
        its pinhole).  Aspect as ``render`` / ``update`` form it from the
        window, fov from the settings; or explicit ``constants``.  Needed
        again after a resize or clear, a scene change or a camera move."""
        c = self._constants(0) if constants is None else constants
        self._chk("pt_render_guides", self._L.pt_render_guides(self._ctx, ctypes.byref(c), ctypes.byref(self.settings)))

    def read_guides(self):
        """(g0, g1), float32 [height][width][4] each, rows as read_image:
        g0 = (normal.xyz, t), g1 = (albedo.rgb, 1 hit / 0 miss)."""
        (g0, p0, nbytes), (g1, p1, _) = self._image(), self._image()
        self._chk("pt_read_guides", self._L.pt_read_guides(self._ctx, p0, p1, nbytes))
        return g0, g1

    DENOISE_OUTPUTS = {"linear": N.PT_DENOISE_LINEAR, "display": N.PT_DISPLAY_RGBA32F, "srgb8": N.PT_DISPLAY_SRGB8}

    def _filter(self, fn: str, params, output: str, **fields) -> np.ndarray:
        """One filter call: the library's ``fn`` with a ``params`` block of
        ``fields`` (the two counts as int, the sigmas as float), into an image
        of ``output``'s kind."""
        if output not in self.DENOISE_OUTPUTS:
            raise ValueError(f"output must be one of {sorted(self.DENOISE_OUTPUTS)}, got {output!r}")
        counts = ("iterations", "normal_power_log2")
        p = params(**{k: int(v) if k in counts else float(v) for k, v in fields.items()})
        out, po, nbytes = self._image(np.uint8 if output == "srgb8" else np.float32)
        self._chk(fn, getattr(self._L, fn)(self._ctx, ctypes.byref(p), self.DENOISE_OUTPUTS[output], po, nbytes))
        return out

    def denoise(self, iterations: int = 5, sigma_color: float = 2.0, sigma_depth: float = 0.05,
                sigma_albedo: float = 0.1, normal_power_log2: int = 5, output: str = "linear") -> np.ndarray:
        """pt_denoise: the accumulation image through ``iterations`` passes of
        the edge-stopping a-trous wavelet (step 1, 2, 4, ...), steered by the
        guide images of ``render_guides``; the image itself is left as it is.
        ``output``: "linear" (float32 [h][w][4], rows as read_image),
        "display" / "srgb8" (the result through the display pass, as
        ``display(srgb8=False / True)`` returns it).  A sigma of 0 switches
        its term off."""
        return self._filter("pt_denoise", N.DenoiseParams, output, iterations=iterations, sigma_color=sigma_color,
                            sigma_depth=sigma_depth, sigma_albedo=sigma_albedo, normal_power_log2=normal_power_log2)

    # -- second moments, variance and the variance-guided filter (new) --------
    def read_moments(self) -> np.ndarray:
        """pt_read_moments: the image of the frames' squared colours, mixed as
        the accumulation image is (``set_option("moments", 1)`` before the
        render); float32 [height][width][4], rows as read_image."""
        out, p, nbytes = self._image()
        self._chk("pt_read_moments", self._L.pt_read_moments(self._ctx, p, nbytes))
        return out

    def write_moments(self, m: np.ndarray, frames: int) -> None:
        """pt_write_moments: replace the moment image and say it holds
        ``frames`` frames of the accumulation image as it is now (after
        write_image: resume a saved render, or hand over the host sum of a
        multi-rank render)."""
        _, p, nbytes = self._image(src=m)
        self._chk("pt_write_moments", self._L.pt_write_moments(self._ctx, p, nbytes, int(frames)))

    def variance(self) -> np.ndarray:
        """pt_read_variance: the variance of the mean per pixel, summed over
        r, g, b; float32 [height][width].  Needs valid moments of >= 2 frames."""
        w, h = self.size
        v = np.empty((h, w), np.float32)
        self._chk("pt_read_variance", self._L.pt_read_variance(self._ctx, N.fptr(v), v.nbytes))
        return v

    def owned(self) -> np.ndarray:
        """bool [height][width]: the texels of the 8x8 tiles this context renders (set_tiles)."""
        w, h = self.size
        rank, nranks = getattr(self, "_tiles", (0, 1))
        ty, tx = np.arange(h)[:, None] // 8, np.arange(w)[None, :] // 8
        return (ty * ((w + 7) // 8) + tx) % nranks == rank

    def noise(self, percentile: float = 95.0) -> float:
        """How noisy the image still is (host numpy): the ``percentile``, over
        the owned and finite texels, of sqrt(variance) / (luminance + 0.01),
        the luminance the plain mean of r, g, b."""
        v, img = self.variance(), self.read_image()
        with np.errstate(all="ignore"):
            rel = np.sqrt(v) / (img[..., :3].mean(-1) + np.float32(0.01))
        rel = rel[self.owned() & np.isfinite(rel)]
        return float(np.percentile(rel, percentile)) if rel.size else 0.0

    def denoise_guided(self, iterations: int = 5, sigma_variance: float = 2.0, sigma_depth: float = 0.05,
                       sigma_albedo: float = 0.1, normal_power_log2: int = 5, output: str = "linear") -> np.ndarray:
        """pt_denoise_guided: ``denoise`` with the colour term steered by the
        per-pixel variance -- a tap's colour difference counts against
        ``sigma_variance`` times the local standard deviation of the mean, so
        a converged pixel keeps its detail and a noisy one is smoothed.  Needs
        ``render_guides`` and valid moments of >= 2 frames; ``output`` as
        ``denoise``.  Both images are left as they are."""
        return self._filter("pt_denoise_guided", N.GuidedParams, output, iterations=iterations,
                            sigma_variance=sigma_variance, sigma_depth=sigma_depth, sigma_albedo=sigma_albedo,
                            normal_power_log2=normal_power_log2)

    def render_until(self, noise: float, max_spp: int, batch: int = 16) -> int:
        """Render "until the noise is below ``noise``": clear the image, switch
        ``moments`` on, and dispatch ``batch`` frames at a time (a plain running
        mean: the first frame's last_clear is 0) until ``noise()`` drops below
        the bar or ``max_spp`` frames are in.  Returns the frames rendered;
        ``render`` goes on from them."""
        if max_spp < 2 or batch < 1:
            raise ValueError("render_until needs max_spp >= 2 and batch >= 1")
        self.set_option("moments", 1)
        self.clear()
        self.changed = False
        done = 0
        while done < max_spp:
            n = min(batch, max_spp - done)
            if done + n < 2:  # (a variance needs two frames)
                n = 2 - done
            c = self._constants(1 + done)
            c.last_clear = done
            self.constants.aspect = c.aspect
            self.dispatch(c, n)
            done += n
            if self.noise() < noise:
                break
        self.constants.frame += done
        self.constants.last_clear = done - 1  # render()'s next frame mixes with last_clear = done
        return done

    # -- temporal accumulation (new: a history reprojected across camera moves) --
    def accumulate_history(self, max_history: float = 16.0, depth_tolerance: float = 0.05, normal_cos: float = 0.9,
                           albedo_tolerance: float = 0.1) -> None:
        """pt_temporal_accumulate: merge the current view -- the image, its
        moments (>= 2 frames) and the guides of ``render_guides`` -- into the
        context's history.  Each hit pixel's first-hit point is projected into
        the view of the last accumulate and takes, bilinearly, the history
        texels there that show the same surface (within ``depth_tolerance``
        of its tangent plane as a share of the distance, normals agreeing to
        ``normal_cos``, albedo to ``albedo_tolerance``), weighing at most
        ``max_history`` samples; a pixel that finds none starts again.  The
        image, moments and guides are left as they are.  A camera move keeps
        the history; a scene change or a resize drops it, and a change of the
        light wants ``reset_history``."""
        p = N.TemporalParams(max_history=float(max_history), depth_tolerance=float(depth_tolerance),
                             normal_cos=float(normal_cos), albedo_tolerance=float(albedo_tolerance))
        self._chk("pt_temporal_accumulate", self._L.pt_temporal_accumulate(self._ctx, ctypes.byref(p)))

    def reset_history(self) -> None:
        """pt_temporal_reset: drop the history; the next accumulate starts it from its view."""
        self._chk("pt_temporal_reset", self._L.pt_temporal_reset(self._ctx))

    def read_history(self):
        """pt_read_history: (colour, moments, count) -- float32 [height][width][4]
        twice, rows as read_image, and the samples per pixel, float32 [height][width]."""
        (hc, pc, nbytes), (hm, pm, _) = self._image(), self._image()
        w, h = self.size
        hn = np.empty((h, w), np.float32)
        self._chk("pt_read_history", self._L.pt_read_history(self._ctx, pc, pm, N.fptr(hn), nbytes))
        return hc, hm, hn

    def denoise_history(self, iterations: int = 5, sigma_variance: float = 2.0, sigma_depth: float = 0.05,
                        sigma_albedo: float = 0.1, normal_power_log2: int = 5, output: str = "linear") -> np.ndarray:
        """pt_denoise_history: ``denoise_guided`` over the history -- its
        colour, the variance of its moments and per-pixel sample count, and
        its own copy of the guides, so it works after a camera move has made
        the live guides stale.  ``output`` as ``denoise``."""
        return self._filter("pt_denoise_history", N.GuidedParams, output, iterations=iterations,
                            sigma_variance=sigma_variance, sigma_depth=sigma_depth, sigma_albedo=sigma_albedo,
                            normal_power_log2=normal_power_log2)

    def render_view(self, spp: int, camera: Optional[N.Camera] = None, **accumulate) -> None:
        """One view of an interactive loop in one call: set ``camera`` if one
        is given, clear the image, switch ``moments`` on, render ``spp`` (>= 2)
        frames as a plain running mean (the first frame's last_clear is 0),
        ``render_guides``, ``accumulate_history(**accumulate)``.  The frame
        counter goes on, so successive views draw distinct samples;
        ``read_history`` / ``denoise_history`` show the result."""
        if spp < 2:
            raise ValueError("render_view needs spp >= 2 (the moments of one frame have no variance)")
        if camera is not None:
            self._set_camera(camera)
        self.clear()
        self.changed = False
        self.set_option("moments", 1)
        c = self._constants(1)
        c.last_clear = 0
        self.constants.aspect = c.aspect
        self.dispatch(c, spp)
        self.constants.frame += spp
        self.constants.last_clear = spp - 1  # render()'s next frame mixes with last_clear = spp
        self.render_guides()
        self.accumulate_history(**accumulate)

    # -- mesh export (new: field sampling and a surface-nets extractor) -------
    def sample_field(self, points):
        """pt_sample_field: map() at ``points`` (float [n][3]) with every
        check[] entry true.  Returns (d float32 [n], shape int32 [n]): the
        distance, and the ordinal of the SHAPE op whose material map() returns
        there (-1 = none)."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        d, s = np.empty(len(p), np.float32), np.empty(len(p), np.int32)
        self._chk("pt_sample_field", self._L.pt_sample_field(self._ctx, N.fptr(p), len(p), N.fptr(d),
                                                              N.ptr(s, ctypes.c_int32)))
        return d, s

    # -- ray queries (new: what a ray hits) ----------------------------------
    @staticmethod
    def _ray_hits(lead, origins, directions, t, shape, normal) -> RayHits:
        with np.errstate(all="ignore"):
            hit = ~(t > np.float32(100.0))
            point = origins + directions * t[:, None]  # (float32: one rounding per step)
        point[~hit] = np.nan
        return RayHits(t.reshape(lead), hit.reshape(lead), shape.reshape(lead), normal.reshape(*lead, 3),
                       point.reshape(*lead, 3))

    def trace_rays(self, origins, directions) -> RayHits:
        """pt_trace_rays: bounds / CastRay / calc_normal along caller rays
        (float [..., 3] each, the same shape).  A direction is used as given,
        not normalised; a ray with a non-finite component is not traced
        (t = NaN, shape -1, zero normal: a hit by the NaN rule)."""
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(directions, np.float32)
        if o.shape != d.shape or o.ndim < 1 or o.shape[-1] != 3:
            raise ValueError(f"origins and directions must both be (..., 3), got {o.shape} and {d.shape}")
        lead, o, d = o.shape[:-1], o.reshape(-1, 3), d.reshape(-1, 3)
        n = len(o)
        t, shape, normal = np.empty(n, np.float32), np.empty(n, np.int32), np.empty((n, 3), np.float32)
        self._chk("pt_trace_rays", self._L.pt_trace_rays(self._ctx, N.fptr(o), N.fptr(d), n, N.fptr(t),
                                                          N.ptr(shape, ctypes.c_int32), N.fptr(normal)))
        return self._ray_hits(lead, o, d, t, shape, normal)

    def _pixel_rays(self, xy, constants):
        """(origins, directions) float32 [n][3] of pixels' jitter-free primary
        rays, in the steps the guide kernel takes (a lens as its pinhole)."""
        F = np.float32
        w, h = self.size
        cam, dflt = self.get_camera()
        with np.errstate(all="ignore"):
            ux = ((xy[:, 0].astype(F) / F(w)) * F(2.0) - F(1.0)) * F(constants.aspect)
            uy = (xy[:, 1].astype(F) / F(h)) * F(2.0) - F(1.0)
            fov = F(self.settings.fov)
            if dflt:
                v = np.stack([ux, uy, np.full(len(xy), fov, F)], -1)
                o = np.tile(np.array([0.0, 0.0, -3.0], F), (len(xy), 1))
            else:
                r, u, f = (np.array(list(a), F) for a in (cam.right, cam.up, cam.forward))
                v = (r * ux[:, None] + u * uy[:, None]) + f * fov
                o = np.tile(np.array(list(cam.origin), F), (len(xy), 1))
            l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            return o, (v / l[:, None]).astype(F)

    def pick_pixels(self, xy=None, constants: Optional[N.Constants] = None) -> RayHits:
        """pt_pick_pixels: the first hit under pixels ``xy`` (int [..., 2] of
        (x, y); None: every pixel, shaped (height, width)) along the rays
        ``render_guides`` casts -- jitter-free, the camera in force with a lens
        as its pinhole, aspect as ``render_guides`` forms it (or explicit
        ``constants``) -- so ``normal`` and ``t`` are the guide plane g0 bit
        for bit.  Nothing of the context changes."""
        c = self._constants(0) if constants is None else constants
        w, h = self.size
        if xy is None:
            lead = (h, w)
            ys, xs = np.divmod(np.arange(w * h, dtype=np.int32), np.int32(max(w, 1)))
            p, pp = np.stack([xs, ys], -1).astype(np.int32), None
        else:
            p = np.ascontiguousarray(xy, np.int32)
            if p.ndim < 1 or p.shape[-1] != 2:
                raise ValueError(f"xy must be (..., 2), got {p.shape}")
            lead, p = p.shape[:-1], p.reshape(-1, 2)
            pp = N.ptr(p, ctypes.c_int32)
        n = len(p)
        t, shape, normal = np.empty(n, np.float32), np.empty(n, np.int32), np.empty((n, 3), np.float32)
        self._chk("pt_pick_pixels", self._L.pt_pick_pixels(self._ctx, ctypes.byref(c), ctypes.byref(self.settings), pp, n,
                                                            N.fptr(t), N.ptr(shape, ctypes.c_int32), N.fptr(normal)))
        o, d = self._pixel_rays(p, c)
        return self._ray_hits(lead, o, d, t, shape, normal)

    def id_image(self, constants: Optional[N.Constants] = None) -> RayHits:
        """The shape-id image: ``pick_pixels`` of every pixel, arrays shaped
        (height, width), rows as read_image."""
        return self.pick_pixels(None, constants)

    def pick(self, x: int, y: int, editor=None) -> Pick:
        """What is under pixel (x, y): a click in an editor.  ``editor`` (the
        SDFEditor the program was compiled from) maps the shape ordinal to its
        ``Shape`` node (``editor.shape_nodes()``)."""
        r = self.pick_pixels([(int(x), int(y))])
        shape, hit = int(r.shape[0]), bool(r.hit[0])
        node = editor.shape_nodes()[shape] if editor is not None and hit and shape >= 0 else None
        return Pick(hit, float(r.t[0]), r.point[0], r.normal[0], shape, node)

    # -- preview shading (new: a noise-free lit image for a viewport) ------------
    def preview(self, light_direction=None, light_color=None, ambient=None, shadow_steps: int = 32,
                shadow_softness: float = 8.0, shadow_cull: bool = False, ao_strength: float = 2.0,
                ao_radius: float = 0.5, highlight=None, highlight_color=(1.0, 0.55, 0.1), highlight_mix: float = 0.5,
                output: str = "linear", constants: Optional[N.Constants] = None) -> np.ndarray:
        """pt_render_preview: the "solid" view of the scene under the camera
        in force -- one jitter-free primary ray per pixel (``render_guides``'
        rays), shaded with a key light and its sphere-traced soft shadow
        (``shadow_steps`` map() calls at most, 0: none; ``shadow_softness``:
        larger = harder edge), five occlusion taps out to ``ao_radius``
        (``ao_strength`` 0: none) and an ambient gradient ``ambient`` =
        (bottom, top) over the normal's height.  No random numbers and no
        accumulation: the same bits on every call, at once after ``set_data``.
        A miss shows the sky (black without one) with alpha 0; a hit has alpha 1.
        ``light_direction`` points towards the light and is used as given;
        arguments left None come from ``preview_light`` (the sky's sun, else a
        light off the camera's shoulder).  ``shadow_cull`` marches the shadow
        under the check[] set of its ray (cheaper; cuts penumbrae at box
        silhouettes).  ``highlight``: a shape ordinal or a ``Pick`` whose
        pixels are mixed ``highlight_mix`` of the way to ``highlight_color``.
        ``output`` and the array returned are ``denoise``'s.  Nothing of the
        context changes."""
        if output not in self.DENOISE_OUTPUTS:
            raise ValueError(f"output must be one of {sorted(self.DENOISE_OUTPUTS)}, got {output!r}")
        default = None
        if any(v is None for v in (light_direction, light_color, ambient)):
            cam, dflt = self.get_camera()
            sky, off = self.get_sky()
            default = preview_light(None if dflt else cam, None if off else sky)
        direction = default.direction if light_direction is None else light_direction
        color = default.color if light_color is None else light_color
        bottom, top = (default.ambient_bottom, default.ambient_top) if ambient is None else ambient
        if isinstance(highlight, Pick):
            highlight = highlight.shape if highlight.hit else None
        p = N.PreviewParams(shadow_steps=int(shadow_steps), shadow_k=float(shadow_softness), shadow_cull=int(bool(shadow_cull)),
                            ao_strength=float(ao_strength), ao_radius=float(ao_radius),
                            highlight=-1 if highlight is None else int(highlight), highlight_mix=float(highlight_mix))
        for name, v in (("light_dir", direction), ("light_color", color), ("ambient_bottom", bottom), ("ambient_top", top),
                        ("highlight_color", highlight_color)):
            if len(v) != 3:
                raise ValueError(f"{name} must have three components, got {v!r}")
            for k in range(3):
                getattr(p, name)[k] = float(v[k])
        c = self._constants(0) if constants is None else constants
        out, po, nbytes = self._image(np.uint8 if output == "srgb8" else np.float32)
        self._chk("pt_render_preview", self._L.pt_render_preview(self._ctx, ctypes.byref(c), ctypes.byref(self.settings),
                                                                  ctypes.byref(p), self.DENOISE_OUTPUTS[output], po, nbytes))
        return out

    # -- radiance queries (new: the light along a ray) ---------------------------
    RADIANCE_MODES = {"ray": N.PT_RADIANCE_RAY, "hemisphere": N.PT_RADIANCE_HEMISPHERE}

    def trace_radiance(self, origins, directions, spp: int, bounces: Optional[int] = None, seed: int = 0,
                       mode: str = "ray", previous: Optional[Radiance] = None) -> Radiance:
        """pt_trace_radiance: ``spp`` path-traced samples along each caller ray
        (float [..., 3] each, the same shape), with the sky in force, folded
        per ray into a running mean and second moment as the image folds
        frames.  ``mode`` "ray": the path starts along the ray as given (a
        direction is not normalised); "hemisphere": ``directions`` are surface
        normals and each sample's first direction is drawn about its normal
        (cosine-distributed for a unit normal: the mean is irradiance / pi).
        ``bounces`` None: the settings' value.  ``seed`` picks the stream of
        random numbers.  ``previous``: a ``Radiance`` of the same rays, seed
        and mode to go on from -- 3 samples then 5 more equal 8 at once, bit
        for bit.  A ray with a non-finite component is not traced (NaN)."""
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(directions, np.float32)
        if o.shape != d.shape or o.ndim < 1 or o.shape[-1] != 3:
            raise ValueError(f"origins and directions must both be (..., 3), got {o.shape} and {d.shape}")
        if mode not in self.RADIANCE_MODES:
            raise ValueError(f"mode must be one of {sorted(self.RADIANCE_MODES)}, got {mode!r}")
        lead, o, d = o.shape[:-1], o.reshape(-1, 3), d.reshape(-1, 3)
        n, sample0 = len(o), 0
        if previous is None:
            mean, moment = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        else:
            if previous.mean.shape != (*lead, 3) or previous.moment.shape != (*lead, 3) or previous.mode != mode:
                raise ValueError("previous must be a Radiance of the same rays and mode")
            sample0 = int(previous.samples)
            mean = np.array(previous.mean, np.float32).reshape(n, 3)  # (copies: the call updates them in place)
            moment = np.array(previous.moment, np.float32).reshape(n, 3)
        p = N.RadianceParams(spp=int(spp), sample0=sample0, seed=int(seed) & 0xFFFFFFFF,
                             bounces=int(self.settings.bounces if bounces is None else bounces),
                             mode=self.RADIANCE_MODES[mode])
        self._chk("pt_trace_radiance", self._L.pt_trace_radiance(self._ctx, N.fptr(o), N.fptr(d), n, ctypes.byref(p),
                                                                  N.fptr(mean), N.fptr(moment)))
        return Radiance(mean.reshape(*lead, 3), moment.reshape(*lead, 3), sample0 + int(spp), mode)

    def irradiance(self, points, normals, spp: int, bounces: Optional[int] = None, seed: int = 0,
                   offset: float = 0.03) -> np.ndarray:
        """Irradiance at surface points, float32 [..., 3]: pi x the hemisphere
        mean of ``trace_radiance`` from ``points + normals * offset`` about
        ``normals`` (unit; float [..., 3] each).  0.03 is the path's own bounce
        offset, so the probe starts where a path leaving the point would."""
        F = np.float32
        pts, nrm = np.asarray(points, F), np.asarray(normals, F)
        r = self.trace_radiance(pts + nrm * F(offset), nrm, spp, bounces, seed, "hemisphere")
        return r.mean * F(np.pi)

    def bake_mesh(self, mesh: Mesh, spp: int, mode: str = "irradiance", offset: float = 0.03, **kw) -> Radiance:
        """The light at every vertex of ``mesh``: ``trace_radiance`` over
        ``mesh.bake_rays(mode, offset)`` -- "irradiance": the hemisphere about
        the vertex normal; "view": what a viewer looking straight at the vertex
        sees, emission and speculars included.  ``Mesh.lit_colors`` turns the
        result into vertex colours.  ``kw``: ``bounces``, ``seed``, ``previous``."""
        o, d = mesh.bake_rays(mode, offset)
        return self.trace_radiance(o, d, spp, mode="hemisphere" if mode == "irradiance" else "ray", **kw)

    # -- point probes (tests: the scene's map() and bounds() per input) ---------
    PROBE_KINDS = {"interp": N.PT_PROBE_INTERP, "table": N.PT_PROBE_TABLE, "baked": N.PT_PROBE_BAKED}
    PROBE_VARIANTS = {"map": N.PT_PROBE_MAP, "b0": N.PT_PROBE_MAP_B0, "b1": N.PT_PROBE_MAP_B1}

    @staticmethod
    def _probe_in(a, dtype, shape):
        """An optional input as a contiguous array of `shape` (None stays None)."""
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype).reshape(shape)
        return a, N.ptr(a, {np.float32: ctypes.c_float, np.uint64: ctypes.c_uint64}[dtype])

    def _probe_counters(self, counters: bool):
        c = np.zeros(N.PT_STAT_COUNT, np.uint64) if counters else None
        return c, (N.ptr(c, ctypes.c_uint64) if counters else None)

    @staticmethod
    def _stat_dict(c):
        return {name: int(c[k]) for k, name in enumerate(N.STAT_NAMES)}

    def probe_map(self, kind, points, check=None, bnd=None, live_in=None, variant="map", union_mode: int = 0,
                  counters: bool = False):
        """pt_probe_map: one map() call per point (float [n][3]) of the
        interpreter ("interp") or of the scene's generated code ("table",
        "baked"); ``check`` uint64 [n][2] (None: every bit set), ``bnd`` float
        [n] (None: +inf), ``live_in`` uint64 [n] (None: 0).  Returns (d float32
        [n], shape int32 [n], live uint64 [n]), with ``counters`` also the
        call's work counters by name."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(p)
        ck, ckp = self._probe_in(check, np.uint64, (n, 2))
        b, bp = self._probe_in(bnd, np.float32, (n,))
        li, lip = self._probe_in(live_in, np.uint64, (n,))
        d, s, lo = np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.uint64)
        c, cp = self._probe_counters(counters)
        self._chk("pt_probe_map", self._L.pt_probe_map(
            self._ctx, self.PROBE_KINDS[kind], self.PROBE_VARIANTS[variant], n, N.fptr(p), ckp, bp, lip, int(union_mode),
            N.fptr(d), N.ptr(s, ctypes.c_int32), N.ptr(lo, ctypes.c_uint64), cp))
        return (d, s, lo, self._stat_dict(c)) if counters else (d, s, lo)

    def probe_taps(self, kind, hits, check=None, bnd=None, counters: bool = False):
        """pt_probe_taps: the shade pass's six normal taps around each hit
        point.  Returns (d6 float32 [n][6], shape6 int32 [n][6], live uint64
        [n]), with ``counters`` also the work counters."""
        p = np.ascontiguousarray(hits, np.float32).reshape(-1, 3)
        n = len(p)
        ck, ckp = self._probe_in(check, np.uint64, (n, 2))
        b, bp = self._probe_in(bnd, np.float32, (n,))
        d, s, lo = np.empty((n, 6), np.float32), np.empty((n, 6), np.int32), np.empty(n, np.uint64)
        c, cp = self._probe_counters(counters)
        self._chk("pt_probe_taps", self._L.pt_probe_taps(self._ctx, self.PROBE_KINDS[kind], n, N.fptr(p), ckp, bp,
                                                          N.fptr(d), N.ptr(s, ctypes.c_int32),
                                                          N.ptr(lo, ctypes.c_uint64), cp))
        return (d, s, lo, self._stat_dict(c)) if counters else (d, s, lo)

    def probe_bounds(self, kind, ro, rd, skip_mode: int = 0, counters: bool = False):
        """pt_probe_bounds: bounds() per ray.  Returns (mask uint64 [n][2]:
        check[] bits 0..63 and 64..127, skip uint64 [ceil(n / 64)]: each wave's
        skip word, zeros with skip_mode 0), with ``counters`` also the work counters."""
        o = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(rd, np.float32).reshape(-1, 3)
        if len(o) != len(r):
            raise ValueError("one direction per origin")
        n = len(o)
        mask, skip = np.zeros((n, 4), np.uint32), np.zeros((n + 63) // 64, np.uint64)
        c, cp = self._probe_counters(counters)
        self._chk("pt_probe_bounds", self._L.pt_probe_bounds(self._ctx, self.PROBE_KINDS[kind], n, N.fptr(o), N.fptr(r),
                                                              int(skip_mode), N.ptr(mask, ctypes.c_uint32),
                                                              N.ptr(skip, ctypes.c_uint64), cp))
        m64 = mask.view(np.uint64).reshape(n, 2)  # (little endian: words 0-1 and 2-3)
        return (m64, skip, self._stat_dict(c)) if counters else (m64, skip)

    def extract_mesh(self, box_min=None, box_max=None, resolution: int = 128, iso: float = 0.0, project: int = 2,
                     grid=None) -> Mesh:
        """pt_mesh_extract + pt_mesh_read: the surface map(p) = ``iso`` inside
        the box as a triangle mesh (surface nets on mesh_grid's cubic cells,
        ``project`` Newton steps per vertex).  ``grid`` = (origin, cell, cells)
        gives the grid itself instead of a box.  The mesh is a snapshot; the
        image, guides, camera, sky and options are untouched."""
        origin, cell, cells = grid if grid is not None else mesh_grid(box_min, box_max, resolution)
        desc = N.MeshDesc(cell=float(cell), iso=float(iso), project=int(project))
        for k in range(3):
            desc.origin[k], desc.cells[k] = float(origin[k]), int(cells[k])
        info = N.MeshInfo()
        self._chk("pt_mesh_extract", self._L.pt_mesh_extract(self._ctx, ctypes.byref(desc), ctypes.byref(info)))
        return self.read_mesh({name: int(getattr(info, name)) for name, _ in N.MeshInfo._fields_})

    def read_mesh(self, info: dict) -> Mesh:
        """pt_mesh_read: the last extracted mesh; ``info`` as extract_mesh made it (its counts size the arrays)."""
        nv, nt = info["n_vertices"], info["n_triangles"]
        pos, nrm = np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32)
        shp, tri = np.empty(nv, np.int32), np.empty((nt, 3), np.uint32)
        self._chk("pt_mesh_read", self._L.pt_mesh_read(self._ctx, N.fptr(pos), N.fptr(nrm), N.ptr(shp, ctypes.c_int32),
                                                        N.ptr(tri, ctypes.c_uint32), nv, nt))
        return Mesh(pos, nrm, shp, tri, info)

    # -- RCCL ------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (ctypes.c_uint8 * N.PT_COMM_ID_BYTES)()
        N.check("pt_comm_get_unique_id", N.lib().pt_comm_get_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks: int, rank: int, uid: bytes) -> None:
        buf = (ctypes.c_uint8 * N.PT_COMM_ID_BYTES).from_buffer_copy(uid)
        self._chk("pt_comm_init", self._L.pt_comm_init(self._ctx, nranks, rank, buf))

    def comm_size(self) -> int:
        """Ranks of the context's RCCL communicator (ncclCommCount)."""
        n = ctypes.c_uint32()
        self._chk("pt_comm_size", self._L.pt_comm_size(self._ctx, ctypes.byref(n)))
        return int(n.value)

    def reduce(self, root: int = 0) -> None:
        self._chk("pt_reduce_accum", self._L.pt_reduce_accum(self._ctx, root))

    def save_image(self) -> np.ndarray:
        """State::save_image (state.rs:237-303) without the PNG encoder: the
        blocking readback plus the 8-bit gamma transform (row 0 = top)."""
        return save_image_rgba8(self.read_image())

    def read_reduced(self) -> np.ndarray:
        out, p, nbytes = self._image()
        self._chk("pt_read_reduced", self._L.pt_read_reduced(self._ctx, p, nbytes))
        return out


def save_image_rgba8(img: np.ndarray) -> np.ndarray:
    """State::save_image pixel transform (state.rs:277-289) on the host, in
    the library (pt_save_rgba8): (v.powf(1.0 / 2.2) * 255.0) as u8 with
    Rust's f32 1.0 / 2.2 and libm powf, alpha * 255, `as u8` saturating (NaN
    -> 0), rows flipped (row 0 = top)."""
    a = np.ascontiguousarray(img, np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"image must be (h, w, 4), got {a.shape}")
    h, w = a.shape[:2]
    out = np.empty((h, w, 4), np.uint8)
    N.check("pt_save_rgba8", N.lib().pt_save_rgba8(N.fptr(a), w, h, N.ptr(out, ctypes.c_uint8), out.nbytes))
    return out


def save_png(img: np.ndarray, path: str) -> None:
    from PIL import Image

    Image.fromarray(save_image_rgba8(img), mode="RGBA").save(path)
