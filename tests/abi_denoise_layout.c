/*
 * abi_denoise_layout.c -- compile-time layout of pt_denoise_params
 * (include/pt_abi.h): 20 bytes, the field offsets the ctypes mirror
 * (_native.DenoiseParams) and the #[repr(C)] block of INTEGRATION.md 2 rely
 * on.  Compiled, not run (tests/test_abi_denoise.py: gcc -std=c11 -Wall
 * -Wextra -Werror -pedantic).
 */
#include <stddef.h>

#include "pt_abi.h"

_Static_assert(sizeof(pt_denoise_params) == 20, "pt_denoise_params is 2 u32 + 3 floats");
_Static_assert(offsetof(pt_denoise_params, iterations) == 0, "iterations");
_Static_assert(offsetof(pt_denoise_params, normal_power_log2) == 4, "normal_power_log2");
_Static_assert(offsetof(pt_denoise_params, sigma_color) == 8, "sigma_color");
_Static_assert(offsetof(pt_denoise_params, sigma_depth) == 12, "sigma_depth");
_Static_assert(offsetof(pt_denoise_params, sigma_albedo) == 16, "sigma_albedo");
_Static_assert(PT_DISPLAY_RGBA32F == 0 && PT_DISPLAY_SRGB8 == 1 && PT_DENOISE_LINEAR == 2, "output formats");
_Static_assert(PT_DENOISE_MAX_ITERATIONS == 8, "iterations 1..8");
_Static_assert(PT_ABI_VERSION == 1, "additive change: the version stays");

/* the entry points' signatures, as a C caller declares pointers to them */
int (*const render_guides_fn)(pt_ctx *, const pt_constants *, const pt_settings *) = pt_render_guides;
int (*const read_guides_fn)(pt_ctx *, float *, float *, size_t) = pt_read_guides;
int (*const denoise_fn)(pt_ctx *, const pt_denoise_params *, int, void *, size_t) = pt_denoise;
