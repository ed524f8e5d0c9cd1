"""CPU reference of the radiance queries (test infrastructure).

radiance(): the contract over camref.CamScene (pyref's scene with the oracle's
map() and bounds()), pyref.path_trace and pyref.Rng, folded by
momentref.frames_fold -- the image's own mix, a ray in a texel's place.  Its
own arithmetic is the seed (seed_of) and the hemisphere draw
(hemisphere_direction), nothing else.  tests/test_radiance_ref.py pins both.
"""
from __future__ import annotations

import numpy as np

import camref
import momentref
import pyref as P

F = np.float32
U32 = 0xFFFFFFFF
RAY, HEMISPHERE = 0, 1
MODES = {"ray": RAY, "hemisphere": HEMISPHERE}


def seed_of(i, seed, k) -> int:
    """The rng state of ray i's sample k under the caller's `seed`: gen_rng's
    form with i, seed and k in the places of a, b and frame."""
    return ((i * 1973 + (seed & U32) * 9277 + (k & U32) * 26699) & U32) | 1


def hemisphere_direction(n, rng):
    """The first direction of a hemisphere sample about `n` (three float32):
    the path's diffuse draw, its order and f32 steps (pyref.path_trace)."""
    z = rng.f01() * F(2.0) - F(1.0)
    a = rng.f01() * P.PI2
    r = F(np.sqrt(F(1.0) - z * z))
    sa, ca = P.sincos(a)
    return P.normalize([n[0] + r * ca, n[1] + r * sa, n[2] + z])


def sample_colours(rows, ro, rd, spp, sample0=0, seed=0, bounces=4, mode=RAY, sky=None):
    """The colours of samples sample0 .. sample0 + spp - 1 of every ray,
    float32 [n][spp][3]; a ray with a non-finite component is not traced (NaN
    rows).  sky: a Sky struct or None.  mode: RAY / HEMISPHERE or their names."""
    sc = camref.CamScene(rows)
    sk = P.sky_fields(sky)
    mode = MODES.get(mode, mode)
    ro, rd = np.asarray(ro, np.float32).reshape(-1, 3), np.asarray(rd, np.float32).reshape(-1, 3)
    out = np.full((len(ro), spp, 3), np.nan, np.float32)
    with np.errstate(all="ignore"):
        for i in range(len(ro)):
            o, d = [F(v) for v in ro[i]], [F(v) for v in rd[i]]
            if not all(np.isfinite(v) for v in (*o, *d)):
                continue
            for s in range(spp):
                rng = P.Rng(seed_of(i, seed, sample0 + s))
                first = hemisphere_direction(d, rng) if mode == HEMISPHERE else d
                out[i, s] = P.path_trace(sc, list(o), list(first), rng, bounces, 0, sk)
    return out


def fold(colours, sample0=0, previous=None):
    """(mean, moment), float32 [n][3] each, after mixing colours [n][spp][3] in
    sample order into `previous` (a (mean, moment) pair; None: cleared), sample
    sample0 + s with last_clear = sample0 + s.  A NaN row of colours gives NaN."""
    colours = np.asarray(colours, np.float32)
    n = len(colours)
    A = M = None
    if previous is not None:
        A, M = (np.concatenate([np.asarray(a, np.float32).reshape(n, 3), np.ones((n, 1), np.float32)], -1) for a in previous)
    frames = [np.concatenate([colours[:, s], np.ones((n, 1), np.float32)], -1) for s in range(colours.shape[1])]
    A, M = momentref.frames_fold(frames, sample0, A, M)
    return np.ascontiguousarray(A[:, :3]), np.ascontiguousarray(M[:, :3])


def radiance(rows, ro, rd, spp, sample0=0, seed=0, bounces=4, mode=RAY, sky=None, previous=None):
    """pt_trace_radiance's (mean, moment) for the rays (ro, rd), float32 [n][3]
    each.  previous: the (mean, moment) of the first sample0 samples (needed
    when sample0 > 0).  A non-finite ray answers NaN whatever `previous` holds."""
    assert (sample0 == 0) == (previous is None)
    colours = sample_colours(rows, ro, rd, spp, sample0, seed, bounces, mode, sky)
    mean, moment = fold(colours, sample0, previous)
    dead = np.isnan(colours).all((1, 2)) & ~np.isfinite(np.concatenate([np.asarray(ro, F).reshape(-1, 3),
                                                                       np.asarray(rd, F).reshape(-1, 3)], -1)).all(-1)
    mean[dead] = moment[dead] = np.nan
    return mean, moment
