"""Pins tests/previewref.py, the CPU reference of the preview shading
(DESIGN.md 3.33), without a GPU: its neutral setting against denoiseref.guides,
the make-up of the c2 case the GPU tests lean on, the shadow and highlight
switches, and preview_light's two branches."""
import functools

import numpy as np
import pytest

import denoiseref as D
import gpuharness as G
import previewref as PR
import pyref as P
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.view import look_at_camera, preview_light, sky_light

F = np.float32
LIGHT = PR.normalized((-0.6, 0.5, -0.6))
C2 = PR.Params(light_dir=LIGHT)
# shadow and occlusion off, ambient 1 / 1, no key light: what is left is albedo * 1 + emission
NEUTRAL = PR.Params(light_dir=LIGHT, light_color=(0, 0, 0), ambient_bottom=(1, 1, 1), ambient_top=(1, 1, 1),
                    shadow_steps=0, ao_strength=0.0)


def _rows(name="c2"):
    return scenes.SCENES[name]().rows()


@functools.lru_cache(maxsize=None)
def _c2(cull=0, **changes):
    """The c2 case at 16 x 16 under look_at(EYE, TARGET) and the tests' sky, computed once per setting."""
    return PR.preview(_rows(), 16, 16, G.aspect(16, 16), 1.0, G.camera("pinhole"), G.sky(),
                      C2._replace(shadow_cull=cull, **changes))


@pytest.mark.parametrize("view", ["default", "pinhole", "lens"])
def test_the_neutral_setting_is_albedo_plus_emission(view):
    rows, w, h = _rows(), 12, 8
    cam = G.camera(view)
    g0, g1 = D.guides(rows, w, h, G.aspect(w, h), 1.0, cam)
    pv = PR.preview(rows, w, h, G.aspect(w, h), 1.0, cam, None, NEUTRAL)
    sc = P.Scene(rows)
    want = np.zeros((h, w, 3), np.float32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if g1[y, x, 3]:
                    mt = sc.mat(int(pv.node[y, x]))
                    nl = P.normalize(mt["light"])
                    want[y, x] = [g1[y, x, k] + nl[k] * mt["br"] for k in range(3)]
    assert 0.1 < g1[..., 3].mean() < 0.9  # hits and misses both occur
    assert G.same_or_nan(pv.image[..., :3], want).all()
    assert np.array_equal(pv.image[..., 3], g1[..., 3])
    assert ((pv.cls == PR.MISS) == (g1[..., 3] == 0)).all() and (pv.node[pv.cls == PR.MISS] == -1).all()
    assert (pv.sh == 1).all() and (pv.ao == 1).all()


def test_the_c2_case_holds_every_class():
    a, b = _c2(0), _c2(1)
    assert PR.class_counts(a) == {"miss": 97, "away": 25, "shadowed": 13, "penumbra": 33, "lit": 88}
    assert int((a.ao < 1).sum()) == 19 and int((a.ao == 0).sum()) == 4
    assert not np.isnan(a.image).any() and not np.isnan(b.image).any()
    # culling cuts penumbrae at box silhouettes: the march differs, the first hit and the occlusion do not
    assert int((G.bits(a.sh) != G.bits(b.sh)).sum()) == 21
    assert (G.bits(a.image) != G.bits(b.image)).any(-1).sum() > 0
    assert np.array_equal(a.ao, b.ao) and np.array_equal(a.node, b.node)
    assert ((a.cls == PR.MISS) == (b.cls == PR.MISS)).all() and ((a.cls == PR.AWAY) == (b.cls == PR.AWAY)).all()
    # a miss is the sky along the ray, alpha 0; a hit has alpha 1
    miss = a.cls == PR.MISS
    assert (a.image[miss][:, 3] == 0).all() and (a.image[~miss][:, 3] == 1).all() and (a.image[miss][:, :3] > 0).all()
    # a penumbra pixel lies strictly between its shadowed and its lit value
    pen = a.cls == PR.PENUMBRA
    assert ((a.sh[pen] > 0) & (a.sh[pen] < 1)).all()


def test_no_shadow_steps_is_a_shadow_of_one():
    a, z = _c2(0), _c2(0, shadow_steps=0)
    assert (z.sh == 1).all() and np.array_equal(z.ao, a.ao)
    unshadowed = a.sh == 1
    assert G.same_or_nan(z.image[unshadowed], a.image[unshadowed]).all()
    assert (z.image[~unshadowed][:, :3] >= a.image[~unshadowed][:, :3]).all()
    assert (G.bits(z.image[~unshadowed]) != G.bits(a.image[~unshadowed])).any(-1).all()
    assert PR.class_counts(z)["shadowed"] == PR.class_counts(z)["penumbra"] == 0


def test_a_highlight_changes_only_its_shape():
    rows, a = _rows(), _c2(0)
    order = PR.shape_rows(rows)
    seen = [k for k, r in enumerate(order) if (a.node == r).any()]
    assert len(seen) >= 2  # more than one shape in view
    for k in seen:
        on = a.node == order[k]
        half = _c2(0, highlight=k)
        changed = (G.bits(half.image) != G.bits(a.image)).any(-1)
        assert (changed <= on).all() and changed.sum() >= 0.9 * on.sum() > 0
        with np.errstate(all="ignore"):
            c = a.image[on][:, :3]
            want = c + (np.array(C2.highlight_color, F) - c) * F(0.5)
        assert G.same_or_nan(half.image[on][:, :3], want).all()
    k = seen[0]
    on = a.node == order[k]
    assert G.same_or_nan(_c2(0, highlight=k, highlight_mix=0.0).image, a.image).all()
    # mix 1: c + (colour - c) is the colour itself where the subtraction is exact -- for black always
    # (c + (0 - c) = 0), for another colour wherever c lies within a factor of two of it
    full = _c2(0, highlight=k, highlight_mix=1.0, highlight_color=(0.0, 0.0, 0.0))
    assert (full.image[on][:, :3] == 0).all() and (full.image[on][:, 3] == 1).all()
    assert G.same_or_nan(full.image[~on], a.image[~on]).all()
    assert G.same_or_nan(_c2(0, highlight=len(order)).image, a.image).all()  # an ordinal no shape has


def test_preview_light_takes_the_suns_direction():
    sky = G.sky()
    got = preview_light(look_at_camera(G.EYE, G.TARGET), sky)
    # sun_dir normalised again in float32 steps: a few ulp from the sky's own (2^-24 per step)
    assert np.allclose(got.direction, np.array(list(sky.sun_dir), F), rtol=0, atol=1e-6)
    assert abs(float(np.linalg.norm(got.direction.astype(np.float64))) - 1.0) < 1e-6
    assert np.array_equal(got.color, np.array([0.9, 0.9, 0.9], F))
    assert np.array_equal(got.ambient_bottom, np.array(list(sky.bottom), F) * F(0.35))
    assert np.array_equal(got.ambient_top, np.array(list(sky.top), F) * F(0.35))
    assert all(a.dtype == np.float32 and a.shape == (3,) for a in got)


def test_preview_light_without_a_sun_sits_off_the_cameras_shoulder():
    cam = look_at_camera(G.EYE, G.TARGET)
    r, u, f = (np.array(list(a), np.float64) for a in (cam.right, cam.up, cam.forward))
    want = -f + 0.5 * u + 0.3 * r
    want /= np.linalg.norm(want)
    for sky in (None, sky_light((0.2, 0.2, 0.3))):  # no sky; a sky whose sun is black
        got = preview_light(cam, sky)
        assert np.allclose(got.direction, want, atol=1e-6)
        assert float(np.dot(got.direction, f)) < 0 < float(np.dot(got.direction, u))  # towards the viewer, from above
    none = preview_light(cam, None)
    assert np.array_equal(none.ambient_bottom, np.array([0.10, 0.10, 0.12], F))
    assert np.array_equal(none.ambient_top, np.array([0.30, 0.32, 0.36], F))
    dim = preview_light(cam, sky_light((0.2, 0.2, 0.3)))
    assert np.array_equal(dim.ambient_bottom, np.array([0.2, 0.2, 0.3], F) * F(0.35))
    # the reference's fixed camera: the identity basis
    fixed = preview_light(None, None)
    want = np.array([0.3, 0.5, -1.0]) / np.linalg.norm([0.3, 0.5, -1.0])
    assert np.allclose(fixed.direction, want, atol=1e-6)
    assert isinstance(preview_light(N.Camera(right=(1, 0, 0), up=(0, 1, 0), forward=(0, 0, 1)), None).direction, np.ndarray)
