/*
 * abi_sky_layout.c -- compile-time layout of pt_sky (include/pt_abi.h): 13
 * floats, 52 bytes, the field offsets the ctypes mirror (_native.Sky) and the
 * #[repr(C)] block of INTEGRATION.md 2 rely on.  Compiled, not run
 * (tests/test_abi_sky.py: gcc -std=c11 -Wall -Wextra -Werror -pedantic).
 */
#include <stddef.h>

#include "pt_abi.h"

_Static_assert(sizeof(pt_sky) == 52, "pt_sky is 13 floats");
_Static_assert(offsetof(pt_sky, bottom) == 0, "bottom");
_Static_assert(offsetof(pt_sky, top) == 12, "top");
_Static_assert(offsetof(pt_sky, sun_dir) == 24, "sun_dir");
_Static_assert(offsetof(pt_sky, sun_color) == 36, "sun_color");
_Static_assert(offsetof(pt_sky, sun_cos) == 48, "sun_cos");
_Static_assert(sizeof(((pt_sky *)0)->bottom) == 12 && sizeof(((pt_sky *)0)->sun_color) == 12, "vec3 fields");
_Static_assert(PT_ABI_VERSION == 1, "additive change: the version stays");

/* the entry points' signatures, as a C caller declares pointers to them */
int (*const set_sky_fn)(pt_ctx *, const pt_sky *) = pt_set_sky;
int (*const get_sky_fn)(const pt_ctx *, pt_sky *, int *) = pt_get_sky;
