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


def assert_same(got, want, what):
    """Bit equality of two arrays of one shape and type (float32 by its bits: a
    NaN equals only the same NaN), the failure naming `what`, how many values
    differ and the first one."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape}, want {want.dtype}{want.shape}"
    same = bits(got) == bits(want) if got.dtype == np.float32 else got == want
    if not same.all():
        at = tuple(int(v) for v in np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} values differ, first at {at}: "
                             f"got {got[at]!r} want {want[at]!r}")


def refused(fn, *args, **kw):
    """(code, message) of the NativeError the call must raise."""
    try:
        fn(*args, **kw)
    except N.NativeError as e:
        return e.code, str(e)
    raise AssertionError(f"{getattr(fn, '__name__', fn)} was not refused")


def shape_albedo(prog, data, shape):
    """The albedo of the product's shape ordinals under `prog` with `data` (black for -1), float32 [n][3]."""
    from compute_path_tracer_amd.mesh import Mesh

    s = np.asarray(shape, np.int32).reshape(-1)
    return Mesh(np.zeros((len(s), 3)), np.zeros((len(s), 3)), s, np.zeros((0, 3))).vertex_colors(prog, data)


def assert_queries(pt, scene, guides, picks, what):
    """id_image() of `pt` bit for bit against the expected guide planes
    (g0, g1) and, where `picks` is given, against rayref.pick's (t, node,
    normal) of every pixel.  scene: (program, data, rows); a shape number is
    compared through its albedo, as test_gpu_rays.py does."""
    import meshref

    prog, data, rows = scene
    g0, g1 = guides
    h, w = g0.shape[:2]
    got = pt.id_image()
    albedo = shape_albedo(prog, data, got.shape).reshape(h, w, 3)
    assert_same(got.t, g0[..., 3], f"{what}: id_image t against g0")
    assert_same(got.normal, g0[..., :3], f"{what}: id_image normal against g0")
    assert_same(got.hit.astype(np.float32), g1[..., 3], f"{what}: id_image hit against g1")
    assert_same(albedo, g1[..., :3], f"{what}: id_image shape's albedo against g1")
    if picks is not None:
        t, node, nrm = picks
        assert_same(got.t, t, f"{what}: id_image t against rayref.pick")
        assert_same(got.normal, nrm, f"{what}: id_image normal against rayref.pick")
        assert_same(albedo, meshref.node_albedo(rows, node).reshape(h, w, 3), f"{what}: shape against rayref.pick")
        assert np.array_equal(got.hit, ~(t > np.float32(100.0))), f"{what}: hit against rayref.pick"
