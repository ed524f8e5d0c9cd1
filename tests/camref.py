"""CPU reference for a moved camera and a sky (test infrastructure).

The C oracle's pto_render has the reference's fixed camera and, like the
reference shader, adds nothing for a ray that leaves the scene.  So a posed
or thin-lens view and a render with a sky (pt_set_sky,
DESIGN.md 3.25) are made here: pyref's render loop and path arithmetic (pure
Python, float32 scalars) over the oracle's C map() and bounds(), which take
any ray.  With the default camera and no sky the result equals
O.OracleScene.render bit for bit (tests/test_camera_ref.py,
tests/test_sky_ref.py), which pins this helper.
"""
from __future__ import annotations

import numpy as np

import pyref as P
from oracle import oracle as O

F = np.float32


class CamScene(P.Scene):
    """pyref.Scene (slots, materials) with map() and bounds() from the oracle."""

    def __init__(self, rows):
        super().__init__(rows)
        self._osc = O.OracleScene(rows)

    def map(self, p, check):
        d, m = self._osc.map([float(v) for v in p], [1 if c else 0 for c in check])
        return F(d), m

    def bounds(self, ro, rd):
        ck, dbg = self._osc.bounds([float(v) for v in ro], [float(v) for v in rd])
        return [bool(c) for c in ck], F(dbg[0])


def primary_hits(rows, w, h, frame, aspect, spp, fov=1.0, camera=None):
    """How many of the w * h * spp primary rays hit the scene (first segments only)."""
    sc = CamScene(rows)
    cam = P.camera_fields(camera)
    hits = 0
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                for j in range(spp):
                    ro, rd, _ = P.primary_ray(cam, x, y, frame + j, w, h, F(aspect), F(fov))
                    check, _ = sc.bounds(ro, rd)
                    hits += int(not P.cast_ray(sc, ro, rd, check)[0] > F(100.0))
    return hits


def render(rows, w, h, frame, last_clear, aspect, bounces, spp, debug=0, fov=1.0, camera=None, sky=None, counts=None):
    """pyref.render_scene over the oracle-backed scene: `camera` a Camera
    struct (None: the fixed one), `sky` a Sky struct (None: the reference's
    void), `counts` a dict for the miss and sun tallies."""
    return P.render_scene(CamScene(rows), w, h, frame, last_clear, aspect, bounces, spp, debug, fov, camera, sky,
                          counts)
