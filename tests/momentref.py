"""CPU reference of the second moments, the variance of the mean and the
variance-guided filter (test infrastructure).

A frame's colour is the existing renderer called with last_clear = 0 and
spp = 1 for that frame: the mix's weight is then 1 and the image is the frame
itself (up to the sign of a zero, which neither A nor c * c keeps).
frames_fold() mixes such colours into the accumulation image A and the moment
image M in numpy float32, one IEEE rounding per operation, in frame order.
guided() is denoiseref's a-trous loop with the per-pixel colour constant and
the variance plane beside the colour, in the contract's order.
tests/test_moment_ref.py pins all of it.
"""
from __future__ import annotations

import functools

import numpy as np

import camref
import denoiseref as D
from oracle import oracle as O

F = np.float32
H3 = (F(0.5), F(0.25))  # the 3x3 smoothing of the variance plane, per axis by |d|
EPS = F(1e-10)


def oracle_frames(rows, w, h, aspect, bounces, n, frame0=1, fov=1.0):
    """The colours of frames frame0 .. frame0 + n - 1 from the C oracle (fixed camera, no sky): a list of (h, w, 4)."""
    osc = O.OracleScene(rows)
    st = O.Settings(0, bounces, 1.0, fov, 0)
    return [osc.render(w, h, O.Constants(0.0, frame0 + j, aspect, 0), st, 1) for j in range(n)]


def camref_frames(rows, w, h, aspect, bounces, n, frame0=1, fov=1.0, camera=None, sky=None):
    """The same through camref.render: a posed camera and / or a sky."""
    return [camref.render(rows, w, h, frame0 + j, 0, aspect, bounces, 1, 0, fov, camera, sky) for j in range(n)]


@functools.lru_cache(maxsize=None)
def folded(name, w, h, n, bounces):
    """(A, M, V) of frames 1..n of a SCENES name on a cleared image (fixed
    camera, no sky), computed once and shared between the tests, read-only."""
    from compute_path_tracer_amd import scenes

    aspect = float(F(w) / F(h))
    A, M = frames_fold(oracle_frames(scenes.SCENES[name]().rows(), w, h, aspect, bounces, n))
    V = variance(A, M, n)
    for a in (A, M, V):
        a.setflags(write=False)
    return A, M, V


def frames_fold(frame_colours, last_clear=0, A=None, M=None):
    """(A, M) after mixing the frames' colours, in order, into the images:
    frame j with w = 1 / float(last_clear + j + 1) and omw = 1 - w,
      A.k = A.k * omw + c.k * w,  M.k = M.k * omw + (c.k * c.k) * w,  alpha 1.
    A, M: the images to go on from (default: cleared)."""
    first = np.asarray(frame_colours[0], np.float32)
    A = np.zeros_like(first) if A is None else np.array(A, np.float32)
    M = np.zeros_like(first) if M is None else np.array(M, np.float32)
    with np.errstate(all="ignore"):
        for j, c in enumerate(frame_colours):
            c = np.asarray(c, np.float32)[..., :3]
            w = F(1.0) / F(last_clear + j + 1)
            omw = F(1.0) - w
            A[..., :3] = A[..., :3] * omw + c * w
            M[..., :3] = M[..., :3] * omw + (c * c) * w
            A[..., 3] = M[..., 3] = F(1.0)
    return A, M


def variance(A, M, n):
    """V = (v.r + v.g) + v.b, v.k = max(M.k - A.k * A.k, 0) / float(n - 1); the max drops a NaN (0)."""
    A, M = np.asarray(A, np.float32), np.asarray(M, np.float32)
    assert n >= 2
    with np.errstate(all="ignore"):
        v = np.fmax(M[..., :3] - A[..., :3] * A[..., :3], F(0.0)) / F(n - 1)
        return (v[..., 0] + v[..., 1]) + v[..., 2]


def _shift(h, w, ox, oy):
    """(p, q) slices with q = p + (ox, oy) inside an (h, w) image, or None when no p has its q inside."""
    x0, x1, y0, y1 = max(0, -ox), min(w, w - ox), max(0, -oy), min(h, h - oy)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def smooth3(v):
    """g: the variance plane over each pixel's 3x3 neighbourhood, dy outer, dx
    inner, taps outside the image or not finite left out; +inf where none is left."""
    h, w = v.shape
    fin = np.isfinite(v)
    sg = np.zeros((h, w), np.float32)
    sw3 = np.zeros((h, w), np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            pq = _shift(h, w, dx, dy)
            if pq is None:
                continue
            p, q = pq
            w3 = H3[abs(dy)] * H3[abs(dx)]
            ok = fin[q]
            sw3[p] = np.where(ok, sw3[p] + w3, sw3[p])
            sg[p] = np.where(ok, sg[p] + w3 * v[q], sg[p])
    with np.errstate(all="ignore"):
        return np.where(sw3 > F(0.0), sg / sw3, F(np.inf)).astype(np.float32)


def noise(A, V, percentile=95.0, owned=None):
    """PathTracer.noise(): the percentile, over the owned and finite texels, of sqrt(V) / (mean of r, g, b + 0.01)."""
    with np.errstate(all="ignore"):
        rel = np.sqrt(np.asarray(V, np.float32)) / (np.asarray(A, np.float32)[..., :3].mean(-1) + F(0.01))
    keep = np.isfinite(rel) if owned is None else owned & np.isfinite(rel)
    return float(np.percentile(rel[keep], percentile)) if keep.any() else 0.0


def iteration(c, v, g0, g1, step, sv2, kz, ka, npow):
    """One pass at `step` over colour c (h, w, 4) and variance v (h, w): (colour, variance)."""
    h, w = c.shape[:2]
    fin = np.isfinite(c[..., :3]).all(-1)
    hit = g1[..., 3]
    kc_all = F(1.0) / (sv2 * smooth3(v) + EPS)
    sw = np.zeros((h, w), np.float32)
    sc = np.zeros((h, w, 3), np.float32)
    sv = np.zeros((h, w), np.float32)
    one = F(1.0)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            pq = _shift(h, w, step * dx, step * dy)
            if pq is None:
                continue
            p, q = pq
            cq, cp = c[q][..., :3], c[p][..., :3]
            ok = fin[q].copy()
            wgt = np.full(ok.shape, D.H[abs(dy)] * D.H[abs(dx)], np.float32)
            if dx != 0 or dy != 0:
                ok &= hit[q] == hit[p]
                den = one + D._sq3(cq - cp) * kc_all[p]
                den_h = den * (one + D._sq3(g1[q][..., :3] - g1[p][..., :3]) * ka)
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
            sv[p] = np.where(ok, sv[p] + (wgt * wgt) * v[q], sv[p])
    out = c.copy()
    out[..., :3] = np.where(fin[..., None], sc / sw[..., None], c[..., :3])
    return out, np.where(fin, sv / (sw * sw), v).astype(np.float32)


def guided(img, V, g0, g1, iterations=5, sigma_variance=2.0, sigma_depth=0.05, sigma_albedo=0.1, normal_power_log2=5,
           with_variance=False):
    """The filtered image (linear, alpha kept); with_variance: (image, the filtered variance plane)."""
    c = np.array(img, np.float32)
    v = np.array(V, np.float32)
    g0, g1 = np.asarray(g0, np.float32), np.asarray(g1, np.float32)
    assert c.ndim == 3 and c.shape[2] == 4 and g0.shape == c.shape and g1.shape == c.shape and v.shape == c.shape[:2]
    _kc, kz, ka = D.constants(iterations, 0.0, sigma_depth, sigma_albedo)
    sv2 = F(sigma_variance) * F(sigma_variance)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            c, v = iteration(c, v, g0, g1, 1 << i, sv2, kz[i], ka, normal_power_log2)
    return (c, v) if with_variance else c
