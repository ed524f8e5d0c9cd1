/*
 * abi_camera_layout.c -- compile-time layout of pt_camera (include/pt_abi.h):
 * 14 floats, 56 bytes, the field offsets the ctypes mirror (_native.Camera)
 * and the #[repr(C)] block of INTEGRATION.md 2 rely on.  Compiled, not run
 * (tests/test_abi_camera.py: gcc -std=c11 -Wall -Wextra -Werror -pedantic).
 */
#include <stddef.h>

#include "pt_abi.h"

_Static_assert(sizeof(pt_camera) == 56, "pt_camera is 14 floats");
_Static_assert(offsetof(pt_camera, origin) == 0, "origin");
_Static_assert(offsetof(pt_camera, right) == 12, "right");
_Static_assert(offsetof(pt_camera, up) == 24, "up");
_Static_assert(offsetof(pt_camera, forward) == 36, "forward");
_Static_assert(offsetof(pt_camera, aperture) == 48, "aperture");
_Static_assert(offsetof(pt_camera, focus) == 52, "focus");
_Static_assert(sizeof(((pt_camera *)0)->origin) == 12 && sizeof(((pt_camera *)0)->forward) == 12, "vec3 fields");
_Static_assert(PT_ABI_VERSION == 1, "additive change: the version stays");

/* the entry points' signatures, as a C caller declares pointers to them */
int (*const set_camera_fn)(pt_ctx *, const pt_camera *) = pt_set_camera;
int (*const get_camera_fn)(const pt_ctx *, pt_camera *, int *) = pt_get_camera;
