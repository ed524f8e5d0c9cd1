"""CPU reference of the ray queries (test infrastructure).

trace(): the contract over camref.CamScene.bounds, pyref.cast_ray and
pyref.calc_normal, combined exactly as denoiseref.guides combines them, with
the rule for a ray that starts non-finite in front.  pick(): the same steps
for a pixel's jitter-free primary ray, built as denoiseref.guides builds it.
tests/test_ray_ref.py pins both against denoiseref.guides.

Shape numbering: the reference reports the shape's row in the editor tree
(-1: none), the product the ordinal of the PT_OP_SHAPE op; the two are compared
through each number's albedo (meshref.node_albedo, Mesh.vertex_colors), as
tests/test_gpu_mesh.py does.

ray_set(): 257 rays per scene from one seeded generator.
"""
from __future__ import annotations

import numpy as np

import camref
import pyref as P
from compute_path_tracer_amd import scenes

F = np.float32
FP = F(100.0)


def _query(sc, ro, rd):
    """(t, node, n) of one ray: ro and rd lists of three float32."""
    if not all(np.isfinite(v) for v in (*ro, *rd)):
        return F(np.nan), -1, [F(0.0)] * 3  # answered by definition, not traced
    check, _ = sc.bounds(ro, rd)
    t, m = P.cast_ray(sc, ro, rd, check)
    if t > FP:  # (a NaN t is a hit, as in path_trace and the guides)
        return t, -1, [F(0.0)] * 3
    hp = [ro[k] + rd[k] * t for k in range(3)]
    return t, m, P.calc_normal(sc, hp, check)


def _answers(n):
    return np.empty(n, np.float32), np.empty(n, np.int32), np.empty((n, 3), np.float32)


def trace(rows, ro, rd):
    """(t float32 [n], node int32 [n], normal float32 [n][3]) of the rays
    (ro, rd), float32 [n][3] each; `node` in the oracle's numbering."""
    sc = camref.CamScene(rows)
    ro, rd = np.asarray(ro, np.float32).reshape(-1, 3), np.asarray(rd, np.float32).reshape(-1, 3)
    t, node, nrm = _answers(len(ro))
    with np.errstate(all="ignore"):
        for i in range(len(ro)):
            t[i], node[i], nrm[i] = _query(sc, [F(v) for v in ro[i]], [F(v) for v in rd[i]])
    return t, node, nrm


def pick(rows, w, h, aspect, fov, camera, xy):
    """trace()'s answers for the pixels xy (int [n][2] of (x, y)): each one's
    jitter-free primary ray under `camera` (a Camera struct or None), a lens
    as its pinhole."""
    sc = camref.CamScene(rows)
    cam = P.camera_fields(camera)
    if cam is not None:  # a lens as its pinhole: no lens draw, no rng at all
        cam = cam[:4] + (F(0.0), cam[5])
    aspect, fov = F(aspect), F(fov)
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    t, node, nrm = _answers(len(xy))
    with np.errstate(all="ignore"):
        for i, (x, y) in enumerate(xy):
            ux = ((F(x) / F(w)) * F(2.0) - F(1.0)) * aspect
            uy = (F(y) / F(h)) * F(2.0) - F(1.0)
            ro, rd = P.camera_ray(cam, ux, uy, fov, None)
            t[i], node[i], nrm[i] = _query(sc, ro, rd)
    return t, node, nrm


# ---- the rays of the GPU tests -----------------------------------------------------
def _boxes(rows):
    """(bmin, bmax) float32 [3] of every shape with an AABB, in the f32 steps of aabb.glsl from_pos_size."""
    sc = P.Scene(rows)
    out = []
    for c, u, _ in sc.bounds_list:
        if not rows[c]["aabb"]:
            continue
        s, us = sc.slot[c], sc.slot[u]
        ctr = [sc.d(us["pos"][k]) + sc.d(s["pos"][k]) for k in range(3)]
        sz = [sc.d(j) for j in s["size"]]
        kind = rows[c]["kind"]
        so = [sz[0] + sz[1], sz[1], sz[0] + sz[1]] if kind == 3 else sz if kind == 2 else [sz[0]] * 3
        s2 = sc.d(us["scale"]) * sc.d(s["scale"])
        hs = [(so[k] * s2) * sc.d(s["ex"]) for k in range(3)]
        out.append((np.array([ctr[k] - hs[k] for k in range(3)], F), np.array([ctr[k] + hs[k] for k in range(3)], F)))
    return out


def _centres(rows):
    """Each shape's position summed up its parents' (scales and rotations left out: near its centre is enough)."""
    out = []
    for r in rows:
        if r["kind"] == 0:
            continue
        c, p = np.array(r["position"], np.float64), r["parent"]
        while p >= 0:
            c, p = c + np.array(rows[p]["position"], np.float64), rows[p]["parent"]
        out.append(np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0))
    return out


def ray_set(name, seed=31):
    """(ro, rd), float32 [257][3] each, for the scene `name` (a scenes.SCENES
    key), the same for the same (name, seed):
      36   the fixed camera's primary rays through a 6 x 6 grid of screen points;
      121  origins uniform in [-0.8, 0.8]^3 with unit random directions;
      30   24 directions with one component exactly 0 and the six axis
           directions (the slab test divides by them);
      21   10 directions of length 0.5, 10 of length 2 and one zero direction;
      16   origins at a shape's centre (negative distances);
      30   origins with one coordinate equal to a box face of a shape with an
           AABB (bmin - o = 0); random rays where the scene has no box;
      1    an origin at 1e20, past the slab test's reciprocal guard of 2^59;
      2    one ray with a NaN component, one with an inf component."""
    rows = scenes.SCENES[name]().rows()
    rng = np.random.default_rng(seed)

    def unit(n):
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def inside(n):
        return rng.uniform(-0.8, 0.8, (n, 3))

    ro, rd = [], []
    g = (np.arange(6) + 0.5) / 6.0 * 2.0 - 1.0  # 6 x 6 screen points, aspect 1, fov 1
    for uy in g:
        for ux in g:
            v = np.array([ux, uy, 1.0])
            ro.append([0.0, 0.0, -3.0])
            rd.append(v / np.linalg.norm(v))
    ro += list(inside(121))
    rd += list(unit(121))
    d = unit(24)
    d[np.arange(24), np.arange(24) % 3] = 0.0
    ro += list(inside(24))
    rd += list(d)
    ro += list(inside(6))
    rd += [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    ro += list(inside(21))
    rd += list(unit(10) * 0.5) + list(unit(10) * 2.0) + [[0.0, 0.0, 0.0]]
    centres = _centres(rows) or [np.zeros(3)]
    ro += [centres[i % len(centres)] for i in range(16)]
    rd += list(unit(16))
    boxes = _boxes(rows)
    o, d = inside(30), unit(30)
    for i in range(30 if boxes else 0):
        bmin, bmax = boxes[i % len(boxes)]
        axis, face = i % 3, (bmin, bmax)[(i // 3) % 2]
        if np.isfinite(face[axis]) and abs(face[axis]) < 1e6:  # (farbox's distant box: keep the origin near the scene)
            o[i, axis] = face[axis]
    ro += list(o)
    rd += list(d)
    ro.append([1e20, 0.1, -0.2])
    rd.append([-1.0, 0.0, 0.0])
    ro += [[0.1, np.nan, 0.2], [0.3, 0.2, -2.0]]
    rd += [[0.0, 0.0, 1.0], [0.0, np.inf, 1.0]]
    ro, rd = np.ascontiguousarray(ro, np.float32), np.ascontiguousarray(rd, np.float32)
    assert ro.shape == rd.shape == (257, 3)
    return ro, rd
