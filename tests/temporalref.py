"""CPU reference of the temporal accumulation (test
infrastructure).

accumulate() restates pt_temporal_accumulate in numpy float32, whole-image
elementwise operations in the contract's order (taps j outer, i inner), one
IEEE f32 rounding per operation.  The rays of both views are pyref.camera_ray
over the jitter-free screen point with the aperture set to 0, as
denoiseref.guides forms them, so a view's hit points are the guide kernel's
bit for bit.  It also counts the pixels that ended in each branch and the
taps each skip rule removed.  history_variance() and denoise_history() are
momentref's variance and guided filter over the history's own planes.
tests/test_temporal_ref.py pins all of it.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import momentref as MR
import pyref as P
from compute_path_tracer_amd import _native as N

F = np.float32

# the view a set of guides was rendered with: a Camera struct or None (the fixed camera), aspect, fov
View = collections.namedtuple("View", "camera aspect fov")
# what has been accumulated, seen from `view`: colour and moments (h, w, 4), count (h, w), the guide planes
History = collections.namedtuple("History", "colour moments count g0 g1 view")

# where a pixel ends: no history at all (the first accumulate, or a degenerate previous basis); a miss; a hit whose
# colour, moments or depth is not finite; behind the previous eye; outside the previous image; inside with no tap
# left (or a cap of 0); history taken -- "partial" counts those of "taken" with fewer than four taps
BRANCHES = ("no_history", "miss", "not_finite", "behind", "outside", "no_valid_tap", "taken", "partial")
# the taps each skip rule removed, in the order the rules are applied
RULES = ("off_image", "prev_miss", "bad_history", "depth", "normal", "albedo", "weight")


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _finite_rgb(c):
    return np.isfinite(c[..., :3]).all(-1)


@functools.lru_cache(maxsize=32)
def _rays(cam_bytes, w, h, aspect, fov):
    cam = None if cam_bytes is None else P.camera_fields(N.Camera.from_buffer_copy(cam_bytes))
    if cam is not None:  # a lens as its pinhole
        cam = cam[:4] + (F(0.0), cam[5])
    aspect, fov = F(aspect), F(fov)
    ro, rd = np.empty((h, w, 3), np.float32), np.empty((h, w, 3), np.float32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                ux = ((F(x) / F(w)) * F(2.0) - F(1.0)) * aspect
                uy = (F(y) / F(h)) * F(2.0) - F(1.0)
                ro[y, x], rd[y, x] = P.camera_ray(cam, ux, uy, fov, None)
    ro.setflags(write=False)
    rd.setflags(write=False)
    return ro, rd


def rays(view, w, h):
    """(ro, rd), float32 (h, w, 3) each: the guide kernel's ray of every pixel under `view` (shared, read-only)."""
    key = None if view.camera is None else bytes(view.camera)
    return _rays(key, w, h, float(F(view.aspect)), float(F(view.fov)))


def hit_points(view, g0):
    """X.k = ro.k + rd.k * t per pixel: the guide kernel's hit points."""
    h, w = g0.shape[:2]
    ro, rd = rays(view, w, h)
    with np.errstate(all="ignore"):
        return ro + rd * g0[..., 3:4]


def reciprocal_basis(camera):
    """(origin, ir, iu, if) of a Camera struct or None (the fixed camera), float32 (3,) each: cross products over
    the determinant in double, each component rounded once.  None when the determinant is zero or not finite."""
    if camera is None:
        o, r, u, f = (0.0, 0.0, -3.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    else:
        o, r, u, f = ([np.float64(v) for v in a] for a in (camera.origin, camera.right, camera.up, camera.forward))

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    with np.errstate(all="ignore"):
        r, u, f = ([np.float64(v) for v in a] for a in (r, u, f))
        uf, fr, ru = cross(u, f), cross(f, r), cross(r, u)
        det = (r[0] * uf[0] + r[1] * uf[1]) + r[2] * uf[2]
        if not np.isfinite(det) or det == 0.0:
            return None
        return (np.array(o, np.float32),) + tuple(np.array([F(v / det) for v in c], np.float32) for c in (uf, fr, ru))


def accumulate(A, M, g0, g1, n_cur, view, hist, max_history, depth_tolerance=0.05, normal_cos=0.9,
               albedo_tolerance=0.1):
    """(History, counts): the current view -- image A and moments M of n_cur
    frames, guides g0 / g1 rendered under `view` -- merged into `hist` (a
    History, or None: none yet).  counts: pixels per BRANCHES name, taps
    removed per RULES name."""
    A, M, g0, g1 = (np.asarray(a, np.float32) for a in (A, M, g0, g1))
    h, w = A.shape[:2]
    assert A.shape == (h, w, 4) and M.shape == A.shape and g0.shape == A.shape and g1.shape == A.shape and n_cur >= 2
    nc = F(n_cur)
    counts = dict.fromkeys(BRANCHES + RULES, 0)
    Hc, Hm, Hn = A.copy(), M.copy(), np.full((h, w), nc, np.float32)
    basis = reciprocal_basis(hist.view.camera) if hist is not None else None
    if basis is None:
        counts["no_history"] = h * w
        return History(Hc, Hm, Hn, g0.copy(), g1.copy(), view), counts
    po, ir, iu, ifw = basis
    one, half = F(1.0), F(0.5)
    fw, fh = F(w), F(h)
    pa, pf = F(hist.view.aspect), F(hist.view.fov)
    at2 = F(albedo_tolerance) * F(albedo_tolerance)
    with np.errstate(all="ignore"):
        hit = g1[..., 3] != F(0.0)
        live = hit & _finite_rgb(A) & _finite_rgb(M) & np.isfinite(g0[..., 3])
        X = hit_points(view, g0)
        d = X - po
        a, b, c = _dot(d, ir), _dot(d, iu), _dot(d, ifw)
        front = live & (c > F(0.0))
        fx = ((((a / c) * pf) / pa) + one) * half * fw
        fy = (((b / c) * pf) + one) * half * fh
        inside = front & (fx > F(-1.0)) & (fx < fw) & (fy > F(-1.0)) & (fy < fh)  # (false for NaN)
        flx, fly = np.floor(np.where(inside, fx, F(0.0))), np.floor(np.where(inside, fy, F(0.0)))
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        tx, ty = fx - flx, fy - fly
        tol = F(depth_tolerance) * np.sqrt(_dot(d, d))
        Xp = hit_points(hist.view, hist.g0)
        sw, sn = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        sh, sm = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
        taps = np.zeros((h, w), np.int64)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                ok = inside.copy()

                def rule(name, keep):
                    nonlocal ok
                    counts[name] += int((ok & ~keep).sum())
                    ok = ok & keep

                rule("off_image", (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h))
                q = (np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1))
                hq, mq, nq, pg0, pg1 = hist.colour[q], hist.moments[q], hist.count[q], hist.g0[q], hist.g1[q]
                rule("prev_miss", pg1[..., 3] != F(0.0))
                rule("bad_history", (nq > F(0.0)) & _finite_rgb(hq) & _finite_rgb(mq))
                rule("depth", np.abs(_dot(Xp[q] - X, g0)) <= tol)  # distance to p's tangent plane
                rule("normal", _dot(g0, pg0) >= F(normal_cos))
                e = pg1[..., :3] - g1[..., :3]
                rule("albedo", (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2] <= at2)
                wgt = (tx if i else one - tx) * (ty if j else one - ty)
                rule("weight", wgt > F(0.0))
                sw = np.where(ok, sw + wgt, sw)
                sh = np.where(ok[..., None], sh + wgt[..., None] * hq[..., :3], sh)
                sm = np.where(ok[..., None], sm + wgt[..., None] * mq[..., :3], sm)
                sn = np.where(ok, sn + wgt * nq, sn)
                taps += ok
        hn = np.fmin(sn / sw, F(max_history))
        take = inside & (sw > F(0.0)) & (hn > F(0.0))
        n = hn + nc
        wgt = nc / n
        omw = one - wgt
        t3, w3, o3 = take[..., None], wgt[..., None], omw[..., None]
        Hc[..., :3] = np.where(t3, (sh / sw[..., None]) * o3 + A[..., :3] * w3, A[..., :3])
        Hm[..., :3] = np.where(t3, (sm / sw[..., None]) * o3 + M[..., :3] * w3, M[..., :3])
        Hn = np.where(take, n, nc).astype(np.float32)
    for name, mask in (("miss", ~hit), ("not_finite", hit & ~live), ("behind", live & ~front), ("outside", front & ~inside),
                       ("no_valid_tap", inside & ~take), ("taken", take), ("partial", take & (taps < 4))):
        counts[name] = int(mask.sum())
    return History(Hc, Hm, Hn, g0.copy(), g1.copy(), view), counts


def history_variance(hist):
    """V = (v.r + v.g) + v.b, v.k = max(HM.k - H.k * H.k, 0) / (HN - 1); the max drops a NaN (0)."""
    H, HM = hist.colour, hist.moments
    with np.errstate(all="ignore"):
        v = np.fmax(HM[..., :3] - H[..., :3] * H[..., :3], F(0.0)) / (hist.count - F(1.0))[..., None]
        return ((v[..., 0] + v[..., 1]) + v[..., 2]).astype(np.float32)


def denoise_history(hist, **params):
    """momentref.guided over the history: its colour, its variance plane, its own guides."""
    return MR.guided(hist.colour, history_variance(hist), hist.g0, hist.g1, **params)
