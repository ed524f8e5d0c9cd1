"""CPU reference for a moved camera (test infrastructure).

The C oracle's pto_render has the reference's fixed camera, so a posed or
thin-lens view is rendered here: pyref's path arithmetic (cast_ray,
calc_normal, path_trace: pure Python, float32 scalars) over the oracle's C
map() and bounds(), which take any ray.  The render loop restates
pyref.render with the camera formulas of DESIGN.md 3.24.  With the default
camera the result equals O.OracleScene.render bit for bit
(tests/test_camera_ref.py), which pins this helper.
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


def camera_fields(cam):
    """A Camera (ctypes) or None -> (origin, right, up, forward, aperture, focus) in float32, or None."""
    if cam is None:
        return None
    return ([F(v) for v in cam.origin], [F(v) for v in cam.right], [F(v) for v in cam.up],
            [F(v) for v in cam.forward], F(cam.aperture), F(cam.focus))


def camera_ray(cam, ux, uy, fov, rng):
    """(ro, rd) of screen point (ux, uy); draws the lens's two numbers from rng."""
    if cam is None:  # the reference's fixed camera
        return [F(0.0), F(0.0), F(-3.0)], P.normalize([ux, uy, fov])
    origin, right, up, fwd, aperture, focus = cam
    rd = P.normalize([(right[k] * ux + up[k] * uy) + fwd[k] * fov for k in range(3)])
    ro = list(origin)
    if aperture > F(0.0):
        u1 = rng.f01()
        u2 = rng.f01()
        r = F(np.sqrt(u1)) * aperture
        a = u2 * P.PI2
        sa, ca = P.sincos(a)
        lx = r * ca
        ly = r * sa
        pf = [origin[k] + rd[k] * focus for k in range(3)]
        ro = [(origin[k] + right[k] * lx) + up[k] * ly for k in range(3)]
        rd = P.normalize([pf[k] - ro[k] for k in range(3)])
    return ro, rd


def _primary(cam, x, y, frame, w, h, aspect, fov):
    """(ro, rd, rng) of pixel (x, y) in `frame`: gen_rng, jitter, calc_uv, camera."""
    rng = P.Rng(P.gen_rng(x, y, frame, w, h))
    jx = rng.f01() - F(0.5)
    jy = rng.f01() - F(0.5)
    ux = ((F(x) + jx) / F(w)) * F(2.0) - F(1.0)
    uy = ((F(y) + jy) / F(h)) * F(2.0) - F(1.0)
    ux = ux * aspect
    ro, rd = camera_ray(cam, ux, uy, fov, rng)
    return ro, rd, rng


def primary_hits(rows, w, h, frame, aspect, spp, fov=1.0, camera=None):
    """How many of the w * h * spp primary rays hit the scene (first segments only)."""
    sc = CamScene(rows)
    cam = camera_fields(camera)
    hits = 0
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                for j in range(spp):
                    ro, rd, _ = _primary(cam, x, y, frame + j, w, h, F(aspect), F(fov))
                    check, _ = sc.bounds(ro, rd)
                    hits += int(not P.cast_ray(sc, ro, rd, check)[0] > F(100.0))
    return hits


def render(rows, w, h, frame, last_clear, aspect, bounces, spp, debug=0, fov=1.0, camera=None):
    """pyref.render with a camera: `camera` a Camera struct (None: the fixed one)."""
    sc = CamScene(rows)
    cam = camera_fields(camera)
    img = np.zeros((h, w, 4), np.float32)
    fov, aspect = F(fov), F(aspect)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                for j in range(spp):
                    ro, rd, rng = _primary(cam, x, y, frame + j, w, h, aspect, fov)
                    if debug in (0, 3):
                        col = P.path_trace(sc, ro, rd, rng, bounces, debug)
                    elif debug == 1:
                        check, dbg = sc.bounds(ro, rd)
                        t, m = P.cast_ray(sc, ro, rd, check)
                        if t > F(100.0):
                            col = [dbg] * 3
                        else:
                            hp = [ro[k] + rd[k] * t for k in range(3)]
                            nn = P.normalize(P.calc_normal(sc, hp, check))
                            col = [(nn[k] * F(0.5) + F(0.5)) * F(0.2) + dbg for k in range(3)]
                    elif debug == 2:
                        check, _ = sc.bounds(ro, rd)
                        t, m = P.cast_ray(sc, ro, rd, check)
                        col = sc.mat(m)["col"]
                    else:
                        col = [F(0.0)] * 3
                    px = img[y, x]
                    if debug != 0:
                        px[:3] = col
                    else:
                        wgt = F(1.0) / F(last_clear + j + 1)
                        for k in range(3):
                            px[k] = F(px[k]) * (F(1.0) - wgt) + F(col[k]) * wgt
                    px[3] = F(1.0)
    return img
