"""CPU reference for the sky (test infrastructure).

pt_set_sky lights the rays that leave the scene; the C
oracle, like the reference shader, adds nothing for them.  So a render with
a sky is made here: pyref.path_trace restated with the miss term, over the
oracle's C map() and bounds() (camref.CamScene) and camref's primary rays, so
a render can take a camera and a sky together.  With sky=None the result
equals O.OracleScene.render bit for bit (tests/test_sky_ref.py), which pins
this helper.
"""
from __future__ import annotations

import numpy as np

import camref
import pyref as P

F = np.float32


def sky_fields(sky):
    """A Sky (ctypes) or None -> (bottom, top, sun_dir, sun_color, sun_cos) in float32, or None."""
    if sky is None:
        return None
    return ([F(v) for v in sky.bottom], [F(v) for v in sky.top], [F(v) for v in sky.sun_dir],
            [F(v) for v in sky.sun_color], F(sky.sun_cos))


def sky_radiance(sky, rd):
    """(g, in_sun): the sky's radiance along rd, in the f32 steps of DESIGN.md 3.25."""
    bottom, top, sun_dir, sun_color, sun_cos = sky
    t = rd[1] * F(0.5) + F(0.5)
    g = [bottom[k] + (top[k] - bottom[k]) * t for k in range(3)]
    s = (rd[0] * sun_dir[0] + rd[1] * sun_dir[1]) + rd[2] * sun_dir[2]
    in_sun = bool(s >= sun_cos)
    if in_sun:
        g = [g[k] + sun_color[k] for k in range(3)]
    return g, in_sun


def path_trace(sc, ro, rd, rng, bounces, debug, sky, counts):
    """pyref.path_trace; a segment that misses adds sky_radiance(rd) * thr
    (debug 0 only) before the path ends.  counts: {"miss", "sun"} tallies."""
    ret = [F(0)] * 3
    thr = [F(1)] * 3
    i = 0
    while i <= bounces:
        check, _ = sc.bounds(ro, rd)
        t, m = P.cast_ray(sc, ro, rd, check)
        if t > F(100.0):
            counts["miss"] += 1
            if sky is not None and debug == 0:
                g, in_sun = sky_radiance(sky, rd)
                counts["sun"] += int(in_sun)
                ret = [ret[k] + g[k] * thr[k] for k in range(3)]
            break
        hp = [ro[k] + rd[k] * t for k in range(3)]
        n = P.calc_normal(sc, hp, check)
        ro = [hp[k] + n[k] * F(0.03) for k in range(3)]
        mt = sc.mat(m)
        do_spec = rng.f01() < mt["spec"]
        prob = P.gmax(mt["spec"] if do_spec else F(1.0) - mt["spec"], F(0.0001))
        z = rng.f01() * F(2.0) - F(1.0)
        a = rng.f01() * P.PI2
        r = F(np.sqrt(F(1.0) - z * z))
        sa, ca = P.sincos(a)
        diffuse = P.normalize([n[0] + r * ca, n[1] + r * sa, n[2] + z])
        if do_spec:
            kk = F(2.0) * P.dot(n, rd)
            sr = [rd[k] - kk * n[k] for k in range(3)]
            al = mt["rough"] * mt["rough"]
            rd = P.normalize([sr[k] * (F(1.0) - al) + diffuse[k] * al for k in range(3)])
        else:
            rd = diffuse
        nl = P.normalize(mt["light"])
        fs = F(1.0) if do_spec else F(0.0)
        for k in range(3):
            ret[k] = ret[k] + (nl[k] * mt["br"]) * thr[k]
            thr[k] = thr[k] * (mt["col"][k] * (F(1.0) - fs) + mt["sc"][k] * fs)
            thr[k] = thr[k] / prob
        p = P.gmax(thr[0], P.gmax(thr[1], thr[2]))
        if rng.f01() > p:
            break
        ip = F(1.0) / p
        thr = [thr[k] * ip for k in range(3)]
        i += 1
    if debug == 3:
        v = F(i) / F(bounces)
        return [v, v, v]
    return ret


def render(rows, w, h, frame, last_clear, aspect, bounces, spp, debug=0, fov=1.0, camera=None, sky=None, counts=None):
    """camref.render with a sky: `sky` a Sky struct (None: the reference's
    void).  counts, when given, receives the samples whose path ended in a
    miss ("miss") and those of them inside the sun's disc ("sun")."""
    if debug in (1, 2):  # these views never path trace
        return camref.render(rows, w, h, frame, last_clear, aspect, bounces, spp, debug=debug, fov=fov, camera=camera)
    sc = camref.CamScene(rows)
    cam = camref.camera_fields(camera)
    sk = sky_fields(sky)
    tally = {"miss": 0, "sun": 0}
    img = np.zeros((h, w, 4), np.float32)
    fov, aspect = F(fov), F(aspect)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                for j in range(spp):
                    ro, rd, rng = camref._primary(cam, x, y, frame + j, w, h, aspect, fov)
                    col = path_trace(sc, ro, rd, rng, bounces, debug, sk, tally)
                    px = img[y, x]
                    if debug != 0:
                        px[:3] = col
                    else:
                        wgt = F(1.0) / F(last_clear + j + 1)
                        for k in range(3):
                            px[k] = F(px[k]) * (F(1.0) - wgt) + F(col[k]) * wgt
                    px[3] = F(1.0)
    if counts is not None:
        counts.update(tally)
    return img
