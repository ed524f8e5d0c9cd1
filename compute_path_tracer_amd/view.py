"""The view's host arithmetic: the ``pt_camera`` of a look-at pose, the
``pt_sky`` of a gradient and a sun, and the preview's default key light, in
float32 steps.  No context, no library."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _native as N

F = np.float32


def _vec(v, name):
    a = np.asarray(v, dtype=np.float32)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be three finite numbers, got {v!r}")
    return a


def _colour(v, name):
    a = _vec(v, name)
    if (a < 0).any():
        raise ValueError(f"{name} must not be negative, got {v!r}")
    return a


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=F)


def _length(a):
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def look_at_camera(eye, target, up=(0.0, 1.0, 0.0), aperture: float = 0.0, focus: Optional[float] = None) -> N.Camera:
    """The ``pt_camera`` at ``eye`` looking at ``target``, in float32 steps:
    forward = normalize(target - eye), right = normalize(cross(up, forward)),
    the camera's up = cross(forward, right) (oriented as the reference's +x
    right / +y up / +z forward view); ``focus`` defaults to |target - eye|.
    ``look_at_camera((0, 0, -3), (0, 0, 0))`` is the reference's camera.  Host
    arithmetic only (no context)."""
    e, t, u = _vec(eye, "eye"), _vec(target, "target"), _vec(up, "up")
    d = t - e
    dist = _length(d)
    if not dist > 0:
        raise ValueError("eye and target coincide")
    fwd = d / dist
    r = _cross(u, fwd)
    rl = _length(r)
    if not rl > F(1e-6) * _length(u):
        raise ValueError(f"up {up!r} is parallel to the view direction")
    right = r / rl
    cup = _cross(fwd, right)
    cam = N.Camera(aperture=float(aperture), focus=float(dist if focus is None else focus))
    for k in range(3):
        cam.origin[k], cam.right[k], cam.up[k], cam.forward[k] = e[k], right[k], cup[k], fwd[k]
    return cam


class PreviewLight(NamedTuple):
    """``preview_light``'s default key light: ``direction`` (towards the light,
    unit), ``color``, and the ambient gradient's ``ambient_bottom`` (a normal
    pointing straight down) and ``ambient_top`` (straight up), float32 [3] each."""

    direction: np.ndarray
    color: np.ndarray
    ambient_bottom: np.ndarray
    ambient_top: np.ndarray


def preview_light(camera: Optional[N.Camera] = None, sky: Optional[N.Sky] = None) -> PreviewLight:
    """The default light of ``PathTracer.preview`` under ``camera`` (None: the
    reference's fixed one) and ``sky`` (None: none set), in float32 steps.
    With a sky whose sun shines (a sun_color above 0) the direction is its
    normalised sun_dir; otherwise a headlight off the camera's shoulder,
    normalize(-forward + 0.5 up + 0.3 right).  The colour is (0.9, 0.9, 0.9).
    The ambient gradient is the sky's bottom / top scaled by 0.35, or
    (0.10, 0.10, 0.12) / (0.30, 0.32, 0.36) without a sky.  Host arithmetic
    only (no context)."""
    if sky is not None and any(float(v) > 0.0 for v in sky.sun_color):
        d = np.array(list(sky.sun_dir), F)
    else:
        if camera is None:
            r, u, f = np.array([1, 0, 0], F), np.array([0, 1, 0], F), np.array([0, 0, 1], F)
        else:
            r, u, f = (np.array(list(a), F) for a in (camera.right, camera.up, camera.forward))
        d = (-f + F(0.5) * u) + F(0.3) * r
    dl = _length(d)
    if not (dl > 0 and np.isfinite(dl)):
        raise ValueError("the light direction is zero or not finite")
    d = (d / dl).astype(F)
    if sky is not None:
        bottom, top = np.array(list(sky.bottom), F) * F(0.35), np.array(list(sky.top), F) * F(0.35)
    else:
        bottom, top = np.array([0.10, 0.10, 0.12], F), np.array([0.30, 0.32, 0.36], F)
    return PreviewLight(d, np.array([0.9, 0.9, 0.9], F), bottom.astype(F), top.astype(F))


def sky_light(bottom, top=None, sun_direction=None, sun_color=(0.0, 0.0, 0.0), sun_angle: float = 0.0) -> N.Sky:
    """The ``pt_sky`` with radiance ``bottom`` looking straight down and
    ``top`` straight up (default: ``bottom``, a uniform ambient light), and a
    sun of radiance ``sun_color`` within ``sun_angle`` degrees of
    ``sun_direction`` (towards the sun; normalised here in float32 steps, and
    (0, 1, 0) without one): sun_cos = float32(cos(radians(sun_angle))).  Host
    arithmetic only (no context)."""
    b = _colour(bottom, "bottom")
    t = b if top is None else _colour(top, "top")
    sc = _colour(sun_color, "sun_color")
    d = _vec((0.0, 1.0, 0.0) if sun_direction is None else sun_direction, "sun_direction")
    dl = _length(d)
    if not dl > 0:
        raise ValueError("sun_direction is zero")
    d = d / dl
    if not 0.0 <= float(sun_angle) <= 180.0:
        raise ValueError(f"sun_angle must lie in [0, 180] degrees, got {sun_angle!r}")
    sky = N.Sky(sun_cos=float(F(np.cos(np.radians(float(sun_angle))))))
    for k in range(3):
        sky.bottom[k], sky.top[k], sky.sun_dir[k], sky.sun_color[k] = b[k], t[k], d[k], sc[k]
    return sky
