"""CPU reference of the denoiser (test infrastructure).

guides(): the first-hit guide images, built as pyref builds its debug views
-- pyref.camera_ray with the aperture set to 0 over the jitter-free screen
point, camref.CamScene.bounds, pyref.cast_ray / calc_normal.

atrous(): the edge-stopping a-trous wavelet in numpy float32, whole-image
elementwise operations per tap in the contract's loop order (dy outer, dx
inner).  Each numpy operation is one IEEE f32 rounding, so it restates the
contract exactly; tests/test_denoise_ref.py pins it.
"""
from __future__ import annotations

import numpy as np

import camref
import pyref as P

F = np.float32
H = (F(0.375), F(0.25), F(0.0625))  # the B3 kernel {3/8, 1/4, 1/16} by |d|


def guides(rows, w, h, aspect, fov=1.0, camera=None):
    """(g0, g1), float32 (h, w, 4) each: g0 = (n, t), g1 = (albedo, 1) on a hit,
    g0 = (0, 0, 0, t), g1 = 0 on a miss.  `camera`: a Camera struct or None."""
    sc = camref.CamScene(rows)
    cam = P.camera_fields(camera)
    if cam is not None:  # a lens as its pinhole: no lens draw, no rng at all
        cam = cam[:4] + (F(0.0), cam[5])
    aspect, fov = F(aspect), F(fov)
    g0 = np.zeros((h, w, 4), np.float32)
    g1 = np.zeros((h, w, 4), np.float32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                ux = ((F(x) / F(w)) * F(2.0) - F(1.0)) * aspect
                uy = (F(y) / F(h)) * F(2.0) - F(1.0)
                ro, rd = P.camera_ray(cam, ux, uy, fov, None)
                check, _ = sc.bounds(ro, rd)
                t, m = P.cast_ray(sc, ro, rd, check)
                g0[y, x, 3] = t
                if t > F(100.0):  # (a NaN t is a hit, as in path_trace)
                    continue
                hp = [ro[k] + rd[k] * t for k in range(3)]
                g0[y, x, :3] = P.calc_normal(sc, hp, check)
                g1[y, x, :3] = sc.mat(m)["col"]
                g1[y, x, 3] = F(1.0)
    return g0, g1


def constants(iterations, sigma_color, sigma_depth, sigma_albedo):
    """(kc[i], kz[i], ka) in f32: the scaled sigma, its square, one division of 1; 0 for a term that is off."""

    def inv_sq(sigma, scale):
        sigma = F(sigma)
        if sigma == F(0.0):
            return F(0.0)
        v = sigma * F(scale)
        with np.errstate(all="ignore"):
            return F(1.0) / (v * v)

    kc = [inv_sq(sigma_color, 2.0 ** -i) for i in range(iterations)]
    kz = [inv_sq(sigma_depth, 2.0 ** i) for i in range(iterations)]
    return kc, kz, inv_sq(sigma_albedo, 1.0)


def _sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def _shift(h, w, ox, oy):
    """(p, q) slices with q = p + (ox, oy) inside an (h, w) image, or None when no p has its q inside."""
    x0, x1, y0, y1 = max(0, -ox), min(w, w - ox), max(0, -oy), min(h, h - oy)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def iteration(c, g0, g1, step, kc, kz, ka, npow, v=None):
    """One pass at `step` over colour c (h, w, 4) with guides g0, g1.  kc: the
    colour constant, one f32 or one per pixel (h, w).  v: a variance plane
    (h, w) filtered beside the colour with the squared weights (momentref);
    then (colour, variance) is returned."""
    h, w = c.shape[:2]
    fin = np.isfinite(c[..., :3]).all(-1)
    hit = g1[..., 3]
    kc = np.broadcast_to(np.asarray(kc, np.float32), (h, w))
    sw = np.zeros((h, w), np.float32)
    sc = np.zeros((h, w, 3), np.float32)
    sv = np.zeros((h, w), np.float32)
    one = F(1.0)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            pq = _shift(h, w, step * dx, step * dy)
            if pq is None:
                continue  # q is outside the image for every p
            p, q = pq
            cq, cp = c[q][..., :3], c[p][..., :3]
            ok = fin[q].copy()
            wgt = np.full(ok.shape, H[abs(dy)] * H[abs(dx)], np.float32)
            if dx != 0 or dy != 0:
                ok &= hit[q] == hit[p]
                den = one + _sq3(cq - cp) * kc[p]
                den_h = den * (one + _sq3(g1[q][..., :3] - g1[p][..., :3]) * ka)
                dz = g0[q][..., 3] - g0[p][..., 3]
                den_h = den_h * (one + (dz * dz) * kz)
                np_, nq = g0[p], g0[q]
                nd = np.fmax((np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2], F(0.0))
                for _ in range(npow):
                    nd = nd * nd
                hit_p = hit[p] != F(0.0)
                wgt = np.where(hit_p, wgt * nd, wgt)
                den = np.where(hit_p, den_h, den)
                wgt = wgt / den
                ok &= wgt > F(0.0)  # (false for NaN)
            sw[p] = np.where(ok, sw[p] + wgt, sw[p])
            sc[p] = np.where(ok[..., None], sc[p] + wgt[..., None] * cq, sc[p])
            if v is not None:
                sv[p] = np.where(ok, sv[p] + (wgt * wgt) * v[q], sv[p])
    out = c.copy()
    out[..., :3] = np.where(fin[..., None], sc / sw[..., None], c[..., :3])
    if v is None:
        return out
    return out, np.where(fin, sv / (sw * sw), v).astype(np.float32)


def atrous(img, g0, g1, iterations=5, sigma_color=2.0, sigma_depth=0.05, sigma_albedo=0.1, normal_power_log2=5):
    """The filtered image (linear, alpha kept); the input is left as it is."""
    c = np.array(img, np.float32)
    g0, g1 = np.asarray(g0, np.float32), np.asarray(g1, np.float32)
    assert c.ndim == 3 and c.shape[2] == 4 and g0.shape == c.shape and g1.shape == c.shape
    kc, kz, ka = constants(iterations, sigma_color, sigma_depth, sigma_albedo)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            c = iteration(c, g0, g1, 1 << i, kc[i], kz[i], ka, normal_power_log2)
    return c
