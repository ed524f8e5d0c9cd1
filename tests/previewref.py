"""CPU reference of the preview shading (test infrastructure).

preview(): the contract over camref.CamScene (pyref's scene with the oracle's
map() and bounds()), pyref.cast_ray / calc_normal / camera_ray / sky_radiance /
gmin / gmax, and the pixel's ray exactly as rayref.pick and denoiseref.guides
build it.  Its own arithmetic is the shadow march, the occlusion taps, the
light and the highlight -- every step one float32 operation in the order
DESIGN.md 3.33 writes it.  tests/test_preview_ref.py pins it against
denoiseref.guides.

Shape numbering: the oracle's map() reports a shape's row in the editor tree,
the product the ordinal of the PT_OP_SHAPE op; ordinal k is the k-th row that
is a shape (SDFEditor.shape_nodes' order, pinned by tests/test_ray_ref.py).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import camref
import pyref as P

F = np.float32
FP = F(100.0)
MISS, AWAY, SHADOWED, PENUMBRA, LIT = range(5)
CLASSES = ("miss", "away", "shadowed", "penumbra", "lit")


class Params(NamedTuple):
    """pt_preview_params, with the defaults of the tests' c2 case."""

    light_dir: tuple = (-0.6, 0.5, -0.6)
    light_color: tuple = (0.9, 0.9, 0.9)
    ambient_bottom: tuple = (0.10, 0.10, 0.12)
    ambient_top: tuple = (0.30, 0.32, 0.36)
    shadow_steps: int = 32
    shadow_k: float = 2.0
    shadow_cull: int = 0
    ao_strength: float = 3.0
    ao_radius: float = 0.5
    highlight: int = -1
    highlight_color: tuple = (1.0, 0.55, 0.1)
    highlight_mix: float = 0.5


class Preview(NamedTuple):
    """image float32 (h, w, 4); cls int8 (h, w), one of MISS .. LIT; sh and ao
    float32 (h, w), 1 where not computed; node int32 (h, w), the hit shape's
    row (-1: none)."""

    image: np.ndarray
    cls: np.ndarray
    sh: np.ndarray
    ao: np.ndarray
    node: np.ndarray


def normalized(v):
    """v / |v| in float32 steps (pyref.normalize), as a tuple of Python floats."""
    return tuple(float(c) for c in P.normalize([F(c) for c in v]))


def shape_rows(rows):
    """Row index of shape ordinal k."""
    return [i for i, r in enumerate(rows) if r["kind"] != 0]


def shadow(sc, q, l, steps, k, check):
    sh, s = F(1.0), F(0.05)
    for _ in range(steps):
        d = sc.map([q[a] + l[a] * s for a in range(3)], check)[0]
        if d < F(0.001):
            return F(0.0)
        sh = P.gmin(sh, (k * d) / s)
        s = s + P.gmax(d, F(0.02))
        if s > FP:
            break
    return sh


def occlusion(sc, hp, n, strength, radius, all_checks):
    occ, w = F(0.0), F(1.0)
    for i in range(5):
        h = F(0.01) + radius * (F(i) * F(0.25))
        d = sc.map([hp[a] + n[a] * h for a in range(3)], all_checks)[0]
        occ = occ + (h - d) * w
        w = w * F(0.95)
    return P.gmin(P.gmax(F(1.0) - strength * occ, F(0.0)), F(1.0))


def preview(rows, w, h, aspect, fov=1.0, camera=None, sky=None, params=Params(), ys=None) -> Preview:
    """pt_render_preview's image of `rows` at w x h.  camera: a Camera struct or
    None; sky: a Sky struct or None; ys: the rows to compute (default all; the
    others stay zero, class MISS)."""
    sc = camref.CamScene(rows)
    cam = P.camera_fields(camera)
    if cam is not None:  # a lens as its pinhole: no lens draw, no rng at all
        cam = cam[:4] + (F(0.0), cam[5])
    sk = P.sky_fields(sky)
    aspect, fov = F(aspect), F(fov)
    p = params
    l = [F(v) for v in p.light_dir]
    lc, ab, at, hc = ([F(v) for v in c] for c in (p.light_color, p.ambient_bottom, p.ambient_top, p.highlight_color))
    k, strength, radius, mix = F(p.shadow_k), F(p.ao_strength), F(p.ao_radius), F(p.highlight_mix)
    all_checks = [True] * sc.n_check
    hl_row = shape_rows(rows)[p.highlight] if 0 <= p.highlight < len(shape_rows(rows)) else None
    img = np.zeros((h, w, 4), np.float32)
    cls = np.zeros((h, w), np.int8)
    shs, aos = np.ones((h, w), np.float32), np.ones((h, w), np.float32)
    nodes = np.full((h, w), -1, np.int32)
    with np.errstate(all="ignore"):
        for y in (range(h) if ys is None else ys):
            for x in range(w):
                ux = ((F(x) / F(w)) * F(2.0) - F(1.0)) * aspect
                uy = (F(y) / F(h)) * F(2.0) - F(1.0)
                ro, rd = P.camera_ray(cam, ux, uy, fov, None)
                check, _ = sc.bounds(ro, rd)
                t, m = P.cast_ray(sc, ro, rd, check)
                if t > FP:  # (a NaN t is a hit, as everywhere)
                    if sk is not None:
                        img[y, x, :3] = P.sky_radiance(sk, rd)[0]
                    continue
                hp = [ro[a] + rd[a] * t for a in range(3)]
                n = P.calc_normal(sc, hp, check)
                q = [hp[a] + n[a] * F(0.03) for a in range(3)]
                ndl = P.gmax((n[0] * l[0] + n[1] * l[1]) + n[2] * l[2], F(0.0))
                sh = F(1.0)
                if p.shadow_steps > 0 and ndl > F(0.0):
                    ck = sc.bounds(q, l)[0] if p.shadow_cull else all_checks
                    sh = shadow(sc, q, l, p.shadow_steps, k, ck)
                ao = occlusion(sc, hp, n, strength, radius, all_checks) if strength > F(0.0) else F(1.0)
                u = n[1] * F(0.5) + F(0.5)
                lit = ndl * sh
                mt = sc.mat(m)
                nl = P.normalize(mt["light"])
                for a in range(3):
                    amb = ab[a] + (at[a] - ab[a]) * u
                    c = (mt["col"][a] * ((amb * ao) + (lc[a] * lit))) + (nl[a] * mt["br"])
                    if hl_row is not None and m == hl_row:
                        c = c + (hc[a] - c) * mix
                    img[y, x, a] = c
                img[y, x, 3] = F(1.0)
                cls[y, x] = AWAY if not ndl > F(0.0) else SHADOWED if sh == F(0.0) else PENUMBRA if sh < F(1.0) else LIT
                shs[y, x], aos[y, x], nodes[y, x] = sh, ao, m
    return Preview(img, cls, shs, aos, nodes)


def class_counts(pv: Preview):
    return {name: int((pv.cls == c).sum()) for c, name in enumerate(CLASSES)}
