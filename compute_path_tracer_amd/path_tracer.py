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
from typing import Optional

import numpy as np

from . import _native as N
from .sdf_editor import Program


def default_settings() -> N.Settings:
    """defaults_and_sliders_gui!(Settings, ...) (path_tracer.rs:157-163)."""
    return N.Settings(debug=1, bounces=8, scale=1.0, fov=1.0, aabb=0)


def look_at_camera(eye, target, up=(0.0, 1.0, 0.0), aperture: float = 0.0, focus: Optional[float] = None) -> N.Camera:
    """The ``pt_camera`` at ``eye`` looking at ``target``, in float32 steps:
    forward = normalize(target - eye), right = normalize(cross(up, forward)),
    the camera's up = cross(forward, right) (oriented as the reference's +x
    right / +y up / +z forward view); ``focus`` defaults to |target - eye|.
    ``look_at_camera((0, 0, -3), (0, 0, 0))`` is the reference's camera.  Host
    arithmetic only (no context)."""
    F = np.float32

    def vec(v, name):
        a = np.asarray(v, dtype=np.float32)
        if a.shape != (3,) or not np.isfinite(a).all():
            raise ValueError(f"{name} must be three finite numbers, got {v!r}")
        return a

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=F)

    def length(a):
        return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])

    e, t, u = vec(eye, "eye"), vec(target, "target"), vec(up, "up")
    d = t - e
    dist = length(d)
    if not dist > 0:
        raise ValueError("eye and target coincide")
    fwd = d / dist
    r = cross(u, fwd)
    rl = length(r)
    if not rl > F(1e-6) * length(u):
        raise ValueError(f"up {up!r} is parallel to the view direction")
    right = r / rl
    cup = cross(fwd, right)
    cam = N.Camera(aperture=float(aperture), focus=float(dist if focus is None else focus))
    for k in range(3):
        cam.origin[k], cam.right[k], cam.up[k], cam.forward[k] = e[k], right[k], cup[k], fwd[k]
    return cam


def sky_light(bottom, top=None, sun_direction=None, sun_color=(0.0, 0.0, 0.0), sun_angle: float = 0.0) -> N.Sky:
    """The ``pt_sky`` with radiance ``bottom`` looking straight down and
    ``top`` straight up (default: ``bottom``, a uniform ambient light), and a
    sun of radiance ``sun_color`` within ``sun_angle`` degrees of
    ``sun_direction`` (towards the sun; normalised here in float32 steps, and
    (0, 1, 0) without one): sun_cos = float32(cos(radians(sun_angle))).  Host
    arithmetic only (no context)."""
    F = np.float32

    def vec(v, name):
        a = np.asarray(v, dtype=np.float32)
        if a.shape != (3,) or not np.isfinite(a).all():
            raise ValueError(f"{name} must be three finite numbers, got {v!r}")
        return a

    def colour(v, name):
        a = vec(v, name)
        if (a < 0).any():
            raise ValueError(f"{name} must not be negative, got {v!r}")
        return a

    b = colour(bottom, "bottom")
    t = b if top is None else colour(top, "top")
    sc = colour(sun_color, "sun_color")
    d = vec((0.0, 1.0, 0.0) if sun_direction is None else sun_direction, "sun_direction")
    dl = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if not dl > 0:
        raise ValueError("sun_direction is zero")
    d = d / dl
    if not 0.0 <= float(sun_angle) <= 180.0:
        raise ValueError(f"sun_angle must lie in [0, 180] degrees, got {sun_angle!r}")
    sky = N.Sky(sun_cos=float(F(np.cos(np.radians(float(sun_angle))))))
    for k in range(3):
        sky.bottom[k], sky.top[k], sky.sun_dir[k], sky.sun_color[k] = b[k], t[k], d[k], sc[k]
    return sky


def mesh_grid(box_min, box_max, resolution: int):
    """The grid ``extract_mesh`` lays over a box, in float32 steps: cubic cells
    of edge cell = max(box_max - box_min) / resolution, so the longest axis
    gets ``resolution`` cells and every other axis ceil(extent / cell) (at
    least 1); origin = box_min.  Returns (origin float32[3], cell float32,
    cells (nx, ny, nz)).  Host arithmetic only (no context)."""
    F = np.float32
    lo, hi = np.asarray(box_min, dtype=F), np.asarray(box_max, dtype=F)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"box corners must be three finite numbers each, got {box_min!r}, {box_max!r}")
    ext = hi - lo
    if not (ext > 0).all():
        raise ValueError(f"box_max must exceed box_min on every axis, got {box_min!r}, {box_max!r}")
    if not 1 <= int(resolution) <= N.PT_MESH_MAX_CELLS:
        raise ValueError(f"resolution must lie in [1, {N.PT_MESH_MAX_CELLS}], got {resolution!r}")
    cell = F(ext.max() / F(int(resolution)))
    cells = tuple(int(min(N.PT_MESH_MAX_CELLS, max(1, np.ceil(e / cell)))) for e in ext)
    return lo, cell, cells


class Mesh:
    """A triangle mesh as ``PathTracer.extract_mesh`` returns it: ``positions``
    and ``normals`` float32 [n][3], ``shapes`` int32 [n] (ordinal of the
    program's SHAPE op whose material map() returns at the vertex, -1 = none),
    ``triangles`` uint32 [m][3] wound outward, ``info`` the extractor's counts
    (a dict of pt_mesh_info's fields)."""

    def __init__(self, positions, normals, shapes, triangles, info=None):
        self.positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        self.shapes = np.ascontiguousarray(shapes, np.int32).reshape(-1)
        self.triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        self.info = dict(info or {})

    def vertex_colors(self, program: Program, data: Optional[np.ndarray] = None) -> np.ndarray:
        """Each vertex's albedo, float32 [n][3]: the first three material slots
        of its shape op in ``data`` (default: the program's own values); MDEF's
        black where no shape claims the vertex."""
        d = np.asarray(program.data if data is None else data, np.float32)
        slots = [list(program.ops[i].material[:3]) for i in range(program.n_ops)
                 if program.ops[i].opcode == N.PT_OP_SHAPE]
        table = np.zeros((len(slots) + 1, 3), np.float32)  # row 0: shape -1
        for k, s in enumerate(slots):
            table[k + 1] = d[s]
        if len(self.shapes) and (self.shapes.min() < -1 or self.shapes.max() >= len(slots)):
            raise ValueError("mesh shape ordinal outside the program's shape ops")
        return table[self.shapes + 1]

    def save_obj(self, path: str) -> None:
        """Wavefront OBJ: ``v``, ``vn`` and ``f a//a b//b c//c`` records (1-based)."""
        with open(path, "w") as f:
            f.write("# compute_path_tracer_amd mesh export\n")
            for p in self.positions:
                f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
            for n in self.normals:
                f.write("vn %.9g %.9g %.9g\n" % tuple(float(x) for x in n))
            for t in self.triangles:
                a, b, c = (int(i) + 1 for i in t)
                f.write(f"f {a}//{a} {b}//{b} {c}//{c}\n")

    def save_ply(self, path: str, colors: Optional[np.ndarray] = None) -> None:
        """Binary little-endian PLY: x y z nx ny nz per vertex (+ uchar red
        green blue from ``colors``, float [n][3] in 0..1), a uchar count and
        three int32 indices per face."""
        nv, nt = len(self.positions), len(self.triangles)
        fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header = ["ply", "format binary_little_endian 1.0", "comment compute_path_tracer_amd mesh export",
                  f"element vertex {nv}"] + [f"property float {n}" for n, _ in fields]
        if colors is not None:
            col = np.asarray(colors, np.float32)
            if col.shape != (nv, 3):
                raise ValueError(f"colors must be ({nv}, 3), got {col.shape}")
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
            header += ["property uchar red", "property uchar green", "property uchar blue"]
        header += [f"element face {nt}", "property list uchar int vertex_indices", "end_header"]
        v = np.zeros(nv, dtype=np.dtype(fields))
        for k, name in enumerate(("x", "y", "z")):
            v[name] = self.positions[:, k]
            v["n" + name] = self.normals[:, k]
        if colors is not None:
            c8 = np.rint(np.clip(np.nan_to_num(col), 0.0, 1.0) * 255.0).astype(np.uint8)
            v["red"], v["green"], v["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
        fc = np.zeros(nt, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
        fc["n"] = 3
        fc["i"] = self.triangles.astype(np.int32)
        with open(path, "wb") as f:
            f.write(("\n".join(header) + "\n").encode("ascii"))
            f.write(v.tobytes())
            f.write(fc.tobytes())


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

    # -- reference surface ---------------------------------------------------
    def remake_pipeline(self, program: Program) -> None:
        """path_tracer.rs:62-76: a topology change (queue_compile)."""
        self._chk("pt_set_program", self._L.pt_set_program(self._ctx, program.ops, program.n_ops, program.aabbs,
                                                            program.n_aabb, program.n_check))

    def set_data(self, data: np.ndarray) -> None:
        """DataArray::update (primitives.rs:131-151): value-only upload."""
        arr = np.ascontiguousarray(data, dtype=np.float32)
        self._chk("pt_set_data", self._L.pt_set_data(self._ctx, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                      arr.size))

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
        self.constants.aspect = float(np.float32(self.window[0]) / np.float32(self.window[1]))  # setup.rs:84-86
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
        c = N.Constants(time=self.constants.time, frame=self.constants.frame + 1,
                        aspect=float(np.float32(self.window[0]) / np.float32(self.window[1])),
                        last_clear=self.constants.last_clear + 1)
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
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.float32)
        self._chk("pt_read_accum", self._L.pt_read_accum(self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                          out.nbytes))
        return out

    def write_image(self, img: np.ndarray) -> None:
        """Replace the accumulation image (pt_write_accum): float32 [h][w][4]."""
        w, h = self.size
        a = np.ascontiguousarray(img, np.float32)
        if a.shape != (h, w, 4):
            raise ValueError(f"image must be ({h}, {w}, 4), got {a.shape}")
        self._chk("pt_write_accum", self._L.pt_write_accum(self._ctx, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                            a.nbytes))

    def display(self, srgb8: bool = False) -> np.ndarray:
        """The display pass (RenderTexturePipeline::render_pass,
        render_texture_shader.wgsl:23-94) on the device.  srgb8=False: fs_main's
        RGBA32F per texel [height][width][4], row 0 = bottom.  srgb8=True: the
        sRGB swapchain's 8-bit RGBA [height][width][4], row 0 = top of screen."""
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.uint8 if srgb8 else np.float32)
        fmt = N.PT_DISPLAY_SRGB8 if srgb8 else N.PT_DISPLAY_RGBA32F
        self._chk("pt_display", self._L.pt_display(self._ctx, fmt, out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return out

    # -- denoiser (new: guide images + an edge-stopping a-trous wavelet) ------
    def render_guides(self, constants: Optional[N.Constants] = None) -> None:
        """pt_render_guides: the first-hit normal / depth / albedo images of
        the view in force (one jitter-free primary ray per pixel, a lens as
        its pinhole).  Aspect as ``render`` / ``update`` form it from the
        window, fov from the settings; or explicit ``constants``.  Needed
        again after a resize or clear, a scene change or a camera move."""
        c = constants
        if c is None:
            c = N.Constants(time=self.constants.time, frame=self.constants.frame,
                            aspect=float(np.float32(self.window[0]) / np.float32(self.window[1])),
                            last_clear=self.constants.last_clear)
        self._chk("pt_render_guides", self._L.pt_render_guides(self._ctx, ctypes.byref(c), ctypes.byref(self.settings)))

    def read_guides(self):
        """(g0, g1), float32 [height][width][4] each, rows as read_image:
        g0 = (normal.xyz, t), g1 = (albedo.rgb, 1 hit / 0 miss)."""
        w, h = self.size
        g0, g1 = np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.float32)
        fp = ctypes.POINTER(ctypes.c_float)
        self._chk("pt_read_guides", self._L.pt_read_guides(self._ctx, g0.ctypes.data_as(fp), g1.ctypes.data_as(fp),
                                                            g0.nbytes))
        return g0, g1

    DENOISE_OUTPUTS = {"linear": N.PT_DENOISE_LINEAR, "display": N.PT_DISPLAY_RGBA32F, "srgb8": N.PT_DISPLAY_SRGB8}

    def denoise(self, iterations: int = 5, sigma_color: float = 2.0, sigma_depth: float = 0.05,
                sigma_albedo: float = 0.1, normal_power_log2: int = 5, output: str = "linear") -> np.ndarray:
        """pt_denoise: the accumulation image through ``iterations`` passes of
        the edge-stopping a-trous wavelet (step 1, 2, 4, ...), steered by the
        guide images of ``render_guides``; the image itself is left as it is.
        ``output``: "linear" (float32 [h][w][4], rows as read_image),
        "display" / "srgb8" (the result through the display pass, as
        ``display(srgb8=False / True)`` returns it).  A sigma of 0 switches
        its term off."""
        if output not in self.DENOISE_OUTPUTS:
            raise ValueError(f"output must be one of {sorted(self.DENOISE_OUTPUTS)}, got {output!r}")
        p = N.DenoiseParams(iterations=int(iterations), normal_power_log2=int(normal_power_log2),
                            sigma_color=float(sigma_color), sigma_depth=float(sigma_depth),
                            sigma_albedo=float(sigma_albedo))
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.uint8 if output == "srgb8" else np.float32)
        self._chk("pt_denoise", self._L.pt_denoise(self._ctx, ctypes.byref(p), self.DENOISE_OUTPUTS[output],
                                                    out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return out

    # -- mesh export (new: field sampling and a surface-nets extractor) -------
    def sample_field(self, points):
        """pt_sample_field: map() at ``points`` (float [n][3]) with every
        check[] entry true.  Returns (d float32 [n], shape int32 [n]): the
        distance, and the ordinal of the SHAPE op whose material map() returns
        there (-1 = none)."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        d, s = np.empty(len(p), np.float32), np.empty(len(p), np.int32)
        self._chk("pt_sample_field", self._L.pt_sample_field(
            self._ctx, p.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(p),
            d.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return d, s

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
        fp = ctypes.POINTER(ctypes.c_float)
        self._chk("pt_mesh_read", self._L.pt_mesh_read(
            self._ctx, pos.ctypes.data_as(fp), nrm.ctypes.data_as(fp), shp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            tri.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), nv, nt))
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
        w, h = self.size
        out = np.empty((h, w, 4), dtype=np.float32)
        self._chk("pt_read_reduced", self._L.pt_read_reduced(self._ctx, out.ctypes.data_as(
            ctypes.POINTER(ctypes.c_float)), out.nbytes))
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
    N.check("pt_save_rgba8", N.lib().pt_save_rgba8(a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), w, h,
                                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out.nbytes))
    return out


def save_png(img: np.ndarray, path: str) -> None:
    from PIL import Image

    Image.fromarray(save_image_rgba8(img), mode="RGBA").save(path)
