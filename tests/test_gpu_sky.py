"""GPU: the sky (pt_set_sky) through every kernel variant,
bit for bit against tests/camref.py -- pyref's path arithmetic with the miss
term over the oracle's map() and bounds(), pinned to the oracle by
tests/test_sky_ref.py.  Every comparison is view(np.uint32) equality of the
whole image.

The sky is sky_light((0.9, 0.8, 0.7), (0.25, 0.45, 0.9), sun towards
(0.4, 0.7, -0.6), sun colour (8, 7, 5), sun angle 30 degrees).  The float32
values sky_light returned go to the GPU and to camref alike, so sky_light's
own rounding is not under test here.  The cameras are test_gpu_camera.py's.
"""
import ctypes
import functools

import numpy as np
import pytest

import camref
import gpuharness as G
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.sdf_editor import CompData
from gpuharness import ALL, EYE, LOOK, SKY, TARGET

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(name, w, h, spp, bounces, kind="default", debug=0, sky=True):
    """camref's image, computed once per case and shared (read-only)."""
    img = camref.render(scenes.SCENES[name]().rows(), w, h, 1, 1, G.aspect(w, h), bounces, spp, debug=debug,
                        camera=G.camera(kind), sky=G.sky() if sky else None)
    img.setflags(write=False)
    return img


def _set_view(pt, kind):
    if LOOK[kind] is not None:
        pt.look_at(EYE, TARGET, **LOOK[kind])


def _render(name, w, h, spp, bounces, kernel, kind="default", debug=0, extra=None):
    """The GPU image with the test sky (and camera), and the dispatch's sky pass count."""
    pt = G.tracer(name, w, h, bounces, kernel, debug, extra)
    _set_view(pt, kind)
    sky = pt.set_sky(**SKY)
    assert bytes(sky) == bytes(G.sky())  # the values camref gets
    got, off = pt.get_sky()
    assert bytes(got) == bytes(sky) and not off
    pt.dispatch(G.constants(w, h), spp)
    img = pt.read_image()
    launches = pt.get_option("sky_launches")
    pt.close()
    return img, launches


def _check_reference(ref, name, w, h, spp, bounces, kind="default", debug=0):
    """The reference is finite and shows the sky: it is not the sky-off image."""
    assert np.isfinite(ref).all() and ref[..., :3].mean() > 0
    dark = G.oracle_image(name, w, h, spp, bounces, debug) if kind == "default" else \
        _ref(name, w, h, spp, bounces, kind, debug, sky=False)
    assert not np.array_equal(ref.view(np.uint32), dark.view(np.uint32))


CASES = [("c2", 24, 16, 2, 4), ("c3", 24, 16, 2, 8),
         ("c2", 20, 13, 2, 4),  # partial tiles: the binned kernels take the gen pass
         ("empty", 16, 8, 2, 4)]  # every ray misses at once
VIEWS = [(c, k) for c in CASES for k in ("default", "lens")] + [(("c3", 24, 16, 2, 8), "pinhole")]


@pytest.mark.parametrize("kernel", ALL)
@pytest.mark.parametrize("case,kind", VIEWS, ids=[f"{c[0]}-{c[1]}x{c[2]}-{k}" for c, k in VIEWS])
def test_sky_every_kernel(gpu, case, kind, kernel):
    name, w, h, spp, bounces = case
    ref = _ref(name, w, h, spp, bounces, kind)
    _check_reference(ref, name, w, h, spp, bounces, kind)
    img, launches = _render(name, w, h, spp, bounces, kernel, kind)
    exact = G.same_bits(img, ref)
    print(f"{kernel} {name} {w}x{h} {kind}: bit-exact={exact:.5f} mean={ref[..., :3].mean():.5f} "
          f"sky passes={launches:.0f}")
    assert exact == 1.0
    # one sky pass after every trace pass of every pipeline (here: one chunk, min(2, spp) pipelines)
    assert launches == (2 * (bounces + 1) if kernel.startswith("binned") else 0)


@pytest.mark.parametrize("kernel", ["binned", "binned_jit"])
def test_sky_wide_scene(gpu, kernel):
    """124 check[] entries: the high mask words ride beside the records the
    sky pass gathers.  (The scene's kernel is test_gpu_parity.py's: in the
    suite it comes from the process's cache; run alone, this file compiles it,
    about a minute.)"""
    name, w, h, spp, bounces = "wide", 48, 32, 2, 6
    ref = _ref(name, w, h, spp, bounces)
    _check_reference(ref, name, w, h, spp, bounces)
    img, _ = _render(name, w, h, spp, bounces, kernel)
    assert G.same_bits(img, ref) == 1.0


@pytest.mark.parametrize("kernel", ["binned_jit", "binned_tier"])
@pytest.mark.parametrize("bin_lanes", [1, 2])
@pytest.mark.parametrize("kind", ["default", "lens"])
def test_sky_one_pixel_over_64_frames(gpu, kind, bin_lanes, kernel):
    """70 frames of an 8x8 image: a first-pass window is one pixel over 64
    frames, the first pass writes no ray records (the sky pass makes the
    camera rays of its misses again), and each pipeline adds to its own
    colour region."""
    ref = _ref("c2", 8, 8, 70, 4, kind)
    _check_reference(ref, "c2", 8, 8, 70, 4, kind)
    pt = G.tracer("c2", 8, 8, 4, kernel, extra={"bin_lanes": bin_lanes})
    _set_view(pt, kind)
    pt.set_sky(**SKY)
    pt.dispatch(G.constants(8, 8), 70)
    img = pt.read_image()
    flags = (pt.get_option("gen_trace"), pt.get_option("gen_norec"), pt.get_option("sky_launches"))
    pt.close()
    assert flags == (1.0, 1.0, float(bin_lanes * 5))
    assert G.same_bits(img, ref) == 1.0


@pytest.mark.parametrize("kernel", ["binned", "binned_jit"])
def test_sky_several_chunks(gpu, kernel):
    """bin_samples 128 < 24 * 16: one frame per chunk, so two chunks per dispatch."""
    name, w, h, spp, bounces = "c3", 24, 16, 2, 8
    pt = G.tracer(name, w, h, bounces, kernel, extra={"bin_samples": 128})
    pt.set_sky(**SKY)
    pt.dispatch(G.constants(w, h), spp)
    img = pt.read_image()
    chunks, launches = pt.get_option("bin_chunks"), pt.get_option("sky_launches")
    pt.close()
    assert chunks == 2.0 and launches == 2.0 * (bounces + 1)
    assert G.same_bits(img, _ref(name, w, h, spp, bounces)) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned_jit"])
@pytest.mark.parametrize("debug", [1, 2, 3])
def test_debug_views_ignore_the_sky(gpu, debug, kernel):
    """Views 1 and 2 never path trace and view 3 shows the segment count: the oracle's sky-off image."""
    ref = G.oracle_image("c3", 24, 16, 2, 8, debug)
    assert np.array_equal(_ref("c3", 24, 16, 2, 8, "default", debug).view(np.uint32), ref.view(np.uint32))
    img, launches = _render("c3", 24, 16, 2, 8, kernel, debug=debug)
    assert launches == 0.0
    assert G.same_bits(img, ref) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned_tier"])
def test_clear_sky_restores_the_void(gpu, kernel):
    w, h, spp, bounces = 24, 16, 2, 8
    pt = G.tracer("c3", w, h, bounces, kernel)
    sky, off = pt.get_sky()
    assert off and bytes(sky) == bytes(N.Sky())
    pt.set_sky(**SKY)
    assert not pt.get_sky()[1]
    pt.clear_sky()
    sky, off = pt.get_sky()
    assert off and bytes(sky) == bytes(N.Sky())
    is_off = ctypes.c_int(-1)
    assert N.lib().pt_get_sky(pt._ctx, None, ctypes.byref(is_off)) == N.PT_OK and is_off.value == 1
    pt.dispatch(G.constants(w, h), spp)
    img = pt.read_image()
    assert pt.get_option("sky_launches") == 0.0
    pt.close()
    assert G.same_bits(img, G.oracle_image("c3", w, h, spp, bounces)) == 1.0


@pytest.mark.parametrize("kernel", ["jit", "binned_tier"])
def test_sky_survives_resets_and_rebuilds(gpu, kernel):
    """update(reset=True), remake_pipeline + set_data and, on the tier-up
    build, a value edit followed by jit_wait all keep the sky."""
    w, h, spp, bounces = 24, 16, 2, 4
    ed = scenes.SCENES["c2"]()
    cd = CompData()
    prog = ed.compile(cd)
    pt = G.tracer(prog, w, h, bounces, kernel)
    sky = pt.set_sky(**SKY)
    ref = _ref("c2", w, h, spp, bounces)

    def check(want):
        pt.clear()
        pt.dispatch(G.constants(w, h), spp)
        got, off = pt.get_sky()
        assert bytes(got) == bytes(sky) and not off
        assert G.same_bits(pt.read_image(), want) == 1.0

    check(ref)
    pt.update(reset=True)
    check(ref)
    pt.remake_pipeline(prog)
    pt.set_data(prog.data)
    if kernel == "binned_tier":
        pt.set_option("jit_wait", 1)
    check(ref)
    if kernel == "binned_tier":
        # a value edit drops the values-baked build; the rebuilt one renders the edited scene under the same sky
        ed.header_unions[0].children_shapes[1].transform.position.x.set(-0.25)
        ed.data_update(cd)
        pt.set_data(cd.data_array.as_array())
        assert pt.get_option("jit_tier_active") == 0.0
        pt.set_option("jit_wait", 1)
        assert pt.get_option("jit_tier_active") == 1.0
        edited = camref.render(ed.rows(), w, h, 1, 1, G.aspect(w, h), bounces, spp, sky=G.sky())
        assert not np.array_equal(edited, ref)
        check(edited)
    pt.close()


@pytest.mark.parametrize("kernel", ["jit", "binned_jit"])
def test_tile_split_with_sky_and_lens(gpu, kernel):
    """Two contexts that own alternate tiles, both with the sky and the lens
    camera: their sum is the one-context image (the sky is per context, and a
    sample depends on its pixel and frame only, whoever renders it)."""
    w, h, spp, bounces = 24, 16, 2, 8
    ref = _ref("c3", w, h, spp, bounces, "lens")
    total = np.zeros((h, w, 4), np.float32)
    for rank in range(2):
        pt = G.tracer("c3", w, h, bounces, kernel)
        pt.set_tiles(rank, 2)
        _set_view(pt, "lens")
        pt.set_sky(**SKY)
        pt.dispatch(G.constants(w, h), spp)
        part = pt.read_image()
        pt.close()
        assert np.any(part != 0) and np.any(np.all(part == 0, axis=-1))  # owns some tiles, not all
        total += part
    assert G.same_bits(total, ref) == 1.0


def test_invalid_skies_are_refused(gpu):
    w, h, spp, bounces = 24, 16, 2, 8
    pt = G.tracer("c3", w, h, bounces, "jit")
    good = pt.set_sky(**SKY)
    L = N.lib()

    def variant(field, k, v):
        sky = N.Sky.from_buffer_copy(bytes(good))
        if k is None:
            setattr(sky, field, v)
        else:
            getattr(sky, field)[k] = v
        return sky

    bad = [variant("top", 1, float("nan")), variant("sun_dir", 0, float("inf")), variant("bottom", 2, -0.5),
           variant("sun_color", 0, -1.0), variant("sun_cos", None, 1.5), variant("sun_cos", None, -1.5),
           variant("sun_cos", None, float("nan"))]
    for sky in bad:
        assert L.pt_set_sky(pt._ctx, ctypes.byref(sky)) == N.PT_ERR_INVALID
        assert b"sky" in L.pt_last_error(pt._ctx)
        got, off = pt.get_sky()
        assert bytes(got) == bytes(good) and not off  # the previous sky stays in force
    with pytest.raises(N.NativeError) as e:
        pt.set_sky(bad[4])  # a ready Sky goes to the library as it is
    assert e.value.code == N.PT_ERR_INVALID
    pt.dispatch(G.constants(w, h), spp)
    img = pt.read_image()
    pt.close()
    assert G.same_bits(img, _ref("c3", w, h, spp, bounces)) == 1.0


def test_sky_calls_mark_the_renderer_changed(gpu):
    """set_sky and clear_sky set `changed`, so the next update() clears the
    image as for a settings change: render() after a sky change starts a
    fresh accumulation."""
    w, h, spp, bounces = 24, 16, 2, 8
    pt = G.tracer("c3", w, h, bounces, "jit")
    for call in (lambda: pt.set_sky(**SKY), lambda: pt.set_sky(G.sky()), pt.clear_sky):
        pt.changed = False
        call()
        assert pt.changed is True
    pt.update()
    assert pt.changed is False
    pt.render(3)  # frames 2..4 without a sky, to be discarded
    pt.set_sky(**SKY)
    pt.constants.frame = 0  # the next frame is 1, as in the reference image
    pt.render(spp)
    img = pt.read_image()
    pt.close()
    assert pt.constants.last_clear == spp
    assert G.same_bits(img, _ref("c3", w, h, spp, bounces)) == 1.0


@pytest.mark.parametrize("kernel", ["simple", "jit", "binned", "binned_jit"])
def test_stats_with_a_sky(gpu, kernel):
    """The instrumented run counts every sample, leaves the image untouched,
    and counts the work it counted without a sky (the sky adds no counter)."""
    w, h, spp, bounces = 24, 16, 2, 8
    pt = G.tracer("c3", w, h, bounces, kernel)
    dark = pt.stats(G.constants(w, h), spp)
    pt.set_sky(**SKY)
    pt.dispatch(G.constants(w, h), spp)
    before = pt.read_image()
    st = pt.stats(G.constants(w, h), spp)
    after = pt.read_image()
    pt.close()
    assert st["samples"] == w * h * spp
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert G.same_bits(after, _ref("c3", w, h, spp, bounces)) == 1.0
    # the work counters (samples .. rr_break, and the first shade pass's hits): the rest are wave clock
    # readings and wave-level tallies of the persistent waves' schedule, which differ between any two dispatches
    work = N.STAT_NAMES[:N.STAT_NAMES.index("rr_break") + 1] + ("shaded_first",)
    assert {k: st[k] for k in work} == {k: dark[k] for k in work}
    assert st["shaded"] > 0 and st["segments"] > st["samples"]
