"""CPU reference of the second moments, the variance of the mean and the
variance-guided filter (test infrastructure).

A frame's colour is the existing renderer called with last_clear = 0 and
spp = 1 for that frame: the mix's weight is then 1 and the image is the frame
itself (up to the sign of a zero, which neither A nor c * c keeps).
frames_fold() mixes such colours into the accumulation image A and the moment
image M in numpy float32, one IEEE rounding per operation, in frame order.
guided() is denoiseref's a-trous pass (denoiseref.iteration) with the
per-pixel colour constant and the variance plane beside the colour, in the
contract's order.
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


def smooth3(v):
    """g: the variance plane over each pixel's 3x3 neighbourhood, dy outer, dx
    inner, taps outside the image or not finite left out; +inf where none is left."""
    h, w = v.shape
    fin = np.isfinite(v)
    sg = np.zeros((h, w), np.float32)
    sw3 = np.zeros((h, w), np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            pq = D._shift(h, w, dx, dy)
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
            kc = F(1.0) / (sv2 * smooth3(v) + EPS)  # the colour constant of each pixel
            c, v = D.iteration(c, g0, g1, 1 << i, kc, kz[i], ka, normal_power_log2, v)
    return (c, v) if with_variance else c
