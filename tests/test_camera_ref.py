"""The moved camera on the CPU (no GPU): tests/camref.py, the reference the
GPU camera tests compare with, against the C oracle where the oracle can
render (the default camera), and the look_at arithmetic of the Python mirror.
"""
import numpy as np
import pytest

import camref
import gpuharness as G
from compute_path_tracer_amd import scenes
from oracle import oracle as O

F = np.float32


@pytest.mark.parametrize("name,w,h,spp,bounces", [
    ("c2", 24, 16, 2, 4),
    ("c2", 20, 13, 2, 4),
    ("c2", 8, 8, 70, 4),
    ("c3", 24, 16, 2, 8),
])
def test_camref_default_camera_equals_oracle(name, w, h, spp, bounces):
    """camref's render loop with the default camera is pto_render, bit for bit."""
    rows = scenes.SCENES[name]().rows()
    a = G.aspect(w, h)
    got = camref.render(rows, w, h, 1, 1, a, bounces, spp)
    ref = O.OracleScene(rows).render(w, h, O.Constants(0.0, 1, a, 1), O.Settings(0, bounces, 1.0, 1.0, 0), spp)
    assert ref[..., :3].mean() > 0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("debug", [1, 2, 3])
def test_camref_debug_views_equal_oracle(debug):
    rows = scenes.SCENES["c3"]().rows()
    w, h = 12, 8
    a = G.aspect(w, h)
    got = camref.render(rows, w, h, 1, 1, a, 8, 1, debug=debug)
    ref = O.OracleScene(rows).render(w, h, O.Constants(0.0, 1, a, 1), O.Settings(debug, 8, 1.0, 1.0, 0), 1)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _look_at(*args, **kw):
    from compute_path_tracer_amd.path_tracer import look_at_camera  # host arithmetic: needs no context

    return look_at_camera(*args, **kw)


def test_look_at_reference_pose_is_identity():
    cam = _look_at((0, 0, -3), (0, 0, 0))
    assert list(cam.origin) == [0.0, 0.0, -3.0]
    assert list(cam.right) == [1.0, 0.0, 0.0]
    assert list(cam.up) == [0.0, 1.0, 0.0]
    assert list(cam.forward) == [0.0, 0.0, 1.0]
    assert cam.aperture == 0.0 and cam.focus == 3.0


def test_look_at_basis_is_orthonormal():
    cam = G.camera("lens")
    r, u, f = (np.array(list(v), np.float64) for v in (cam.right, cam.up, cam.forward))
    for a in (r, u, f):
        assert abs(np.dot(a, a) - 1.0) < 1e-6
    assert abs(np.dot(r, u)) < 1e-6 and abs(np.dot(r, f)) < 1e-6 and abs(np.dot(u, f)) < 1e-6
    # oriented like the reference's view (x right, y up, z forward), and forward points at the target
    assert np.allclose(np.cross(r, u), f, atol=1e-6)
    eye = np.array(G.EYE)
    assert np.allclose(f, -eye / np.linalg.norm(eye), atol=1e-6)
    assert list(cam.origin) == [2.0, 1.5, -2.5]
    assert cam.aperture == float(F(0.05)) and cam.focus == 3.0
    # focus defaults to the distance to the target, in float32
    d = G.camera("pinhole").focus
    assert d == float(np.sqrt(F(2.0) * F(2.0) + F(1.5) * F(1.5) + F(2.5) * F(2.5)))


@pytest.mark.parametrize("eye,target,up", [
    ((0, -3, 0), (0, 0, 0), (0, 1, 0)),   # looking straight up
    ((0, 3, 0), (0, 0, 0), (0, 1, 0)),    # straight down
    ((1, 1, 1), (3, 3, 3), (-2, -2, -2)),
])
def test_look_at_rejects_parallel_up(eye, target, up):
    with pytest.raises(ValueError):
        _look_at(eye, target, up)


@pytest.mark.parametrize("name,w,h,spp,pinhole,lens", [
    ("c2", 24, 16, 2, 441, 440),
    ("c3", 24, 16, 2, 729, 730),
])
def test_test_camera_sees_the_scene(name, w, h, spp, pinhole, lens):
    """The GPU tests' camera frames the scenes: the primary rays that hit, as
    recorded when the camera was chosen (a wrong basis or draw order moves
    these counts)."""
    rows = scenes.SCENES[name]().rows()
    a = G.aspect(w, h)
    assert camref.primary_hits(rows, w, h, 1, a, spp, camera=G.camera("pinhole")) == pinhole
    assert camref.primary_hits(rows, w, h, 1, a, spp, camera=G.camera("lens")) == lens
