"""Shared by the GPU test files and the CPU files that pin their references:
the kernel variants, the contexts the tests render on, cached oracle images,
bit comparisons, and the camera pose and sky of the camera and sky tests.
Importing it needs no GPU and no library state of its own."""
import functools

import numpy as np

from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData, SDFEditor
from oracle import oracle as O

KERNELS = {"simple": {"kernel": "simple", "jit": 0}, "wave": {"kernel": "wave", "jit": 0},
           "jit": {"kernel": "wave", "jit": 1, "jit_bake": 0}, "binned": {"kernel": "binned", "jit": 0},
           "binned_jit": {"kernel": "binned", "jit": 1, "jit_bake": 0},
           "binned_bake": {"kernel": "binned", "jit": 1, "jit_bake": 1},
           "binned_tier": {"kernel": "binned", "jit": 1, "jit_bake": 2},
           # normal taps in the trace pass instead of the shade pass
           "binned_trace_taps": {"kernel": "binned", "jit": 1, "jit_bake": 2, "shade_taps": 0},
           "binned_jit_trace_taps": {"kernel": "binned", "jit": 1, "jit_bake": 0, "shade_taps": 0}}
INTERPRETERS = ["simple", "wave", "binned"]
SCENE_KERNELS = ["jit", "binned_jit", "binned_bake", "binned_tier", "binned_trace_taps"]
ALL = ["simple", "wave", "jit", "binned", "binned_jit", "binned_bake", "binned_tier", "binned_trace_taps"]

# the camera and sky tests' pose, views and sky
EYE, TARGET = (2.0, 1.5, -2.5), (0.0, 0.0, 0.0)
LOOK = {"default": None, "pinhole": {}, "lens": {"aperture": 0.05, "focus": 3.0}}
SKY = dict(bottom=(0.9, 0.8, 0.7), top=(0.25, 0.45, 0.9), sun_direction=(0.4, 0.7, -0.6), sun_color=(8.0, 7.0, 5.0),
           sun_angle=30.0)


def camera(kind):
    """The Camera of LOOK[kind] (None: the reference's fixed one), as look_at_camera rounds it."""
    from compute_path_tracer_amd.path_tracer import look_at_camera  # host arithmetic: needs no context

    return None if LOOK[kind] is None else look_at_camera(EYE, TARGET, **LOOK[kind])


def sky():
    """The Sky of SKY, as sky_light rounds it."""
    from compute_path_tracer_amd.path_tracer import sky_light

    return sky_light(**SKY)


def aspect(w, h):
    return float(np.float32(w) / np.float32(h))


def constants(w, h, frame=1, last_clear=1):
    return N.Constants(time=0.0, frame=frame, aspect=aspect(w, h), last_clear=last_clear)


def ready(pt, opts):
    """No quiet fall-back: the scene kernel serves, and jit_bake 2 runs on its values-baked build."""
    if opts.get("jit"):
        assert pt.get_option("jit_active") == 1.0, pt.jit_log()
    if opts.get("jit_bake") == 2:
        pt.set_option("jit_wait", 1)
        assert pt.get_option("jit_tier_active") == 1.0, pt.jit_log()


def tracer(scene, w, h, bounces, kernel=None, debug=0, extra=None, **settings):
    """A PathTracer on `scene` (a SCENES name, an editor, a compiled Program,
    or None for a context without one) with the options of KERNELS[kernel]
    and `extra`, checked by ready() when it has a program."""
    from compute_path_tracer_amd.path_tracer import PathTracer

    if isinstance(scene, str):
        scene = scenes.SCENES[scene]()
    prog = scene.compile(CompData()) if isinstance(scene, SDFEditor) else scene
    opts = dict(KERNELS[kernel]) if kernel is not None else {}
    opts.update(extra or {})
    st = dict(debug=debug, bounces=bounces, scale=1.0, fov=1.0, aabb=0)
    st.update(settings)
    pt = PathTracer(w, h, prog, settings=N.Settings(**st), options=opts)
    if prog is not None:
        ready(pt, opts)
    return pt


def oracle_image(scene, w, h, spp, bounces, debug=0, counters=False, fov=1.0):
    """The C oracle's image of frame 1 on a cleared image (with counters: the
    image and the work counters).  The image of a SCENES name is computed once
    and shared, read-only; an editor is rendered as it is now."""
    if isinstance(scene, str):
        return _named_oracle_image(scene, w, h, spp, bounces, debug, counters, fov)
    return O.OracleScene(scene.rows()).render(w, h, O.Constants(0.0, 1, aspect(w, h), 1),
                                              O.Settings(debug, bounces, 1.0, fov, 0), spp, counters=counters)


@functools.lru_cache(maxsize=None)
def _named_oracle_image(name, *args):
    got = oracle_image(scenes.SCENES[name](), *args)
    (got[0] if isinstance(got, tuple) else got).setflags(write=False)
    return got


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    """The share of values that agree bit for bit."""
    return float(np.mean(bits(a) == bits(b)))


def same_or_nan(a, b):
    """Elementwise: the same bits, or a NaN in both."""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def first_difference(got, want):
    """None when the images agree bit for bit (a NaN equal only to a NaN in
    the same place), else "(x, y): got ... want ..." of the first texel that differs."""
    bad = np.argwhere(~same_or_nan(got, want).all(-1))
    if not len(bad):
        return None
    y, x = (int(v) for v in bad[0])
    return f"{len(bad)} texels differ, first (x={x}, y={y}): got {got[y, x].tolist()} want {want[y, x].tolist()}"


def pixels_changed(a, b):
    """Pixels whose bits differ between two oracle images."""
    return int((bits(a) != bits(b)).any(-1).sum())
