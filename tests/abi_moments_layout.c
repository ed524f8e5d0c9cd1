/*
 * abi_moments_layout.c -- compile-time layout of pt_guided_params
 * (include/pt_abi.h): 20 bytes, the field offsets the ctypes mirror
 * (_native.GuidedParams) and the #[repr(C)] block of INTEGRATION.md 2 rely
 * on, and the signatures of the second-moment entry points.  Compiled, not
 * run (tests/test_abi_moments.py: gcc -std=c11 -Wall -Wextra -Werror
 * -pedantic).
 */
#include <stddef.h>

#include "pt_abi.h"

_Static_assert(sizeof(pt_guided_params) == 20, "pt_guided_params is 2 u32 + 3 floats");
_Static_assert(offsetof(pt_guided_params, iterations) == 0, "iterations");
_Static_assert(offsetof(pt_guided_params, normal_power_log2) == 4, "normal_power_log2");
_Static_assert(offsetof(pt_guided_params, sigma_variance) == 8, "sigma_variance");
_Static_assert(offsetof(pt_guided_params, sigma_depth) == 12, "sigma_depth");
_Static_assert(offsetof(pt_guided_params, sigma_albedo) == 16, "sigma_albedo");
_Static_assert(sizeof(pt_guided_params) == sizeof(pt_denoise_params), "the two filters' blocks have one size");
_Static_assert(PT_DISPLAY_RGBA32F == 0 && PT_DISPLAY_SRGB8 == 1 && PT_DENOISE_LINEAR == 2, "output formats");
_Static_assert(PT_DENOISE_MAX_ITERATIONS == 8, "iterations 1..8");
_Static_assert(PT_ERR_UNSUPPORTED == -3 && PT_ERR_STATE == -4 && PT_ERR_SIZE == -6, "the refusals' codes");
_Static_assert(PT_ABI_VERSION == 1, "additive change: the version stays");

/* the struct has a tag as well: a C caller may name it either way */
static const struct pt_guided_params defaults = {5, 5, 2.0f, 0.05f, 0.1f};
const pt_guided_params *const guided_defaults = &defaults;

/* the entry points' signatures, as a C caller declares pointers to them */
int (*const read_moments_fn)(pt_ctx *, float *, size_t) = pt_read_moments;
int (*const write_moments_fn)(pt_ctx *, const float *, size_t, uint32_t) = pt_write_moments;
int (*const read_variance_fn)(pt_ctx *, float *, size_t) = pt_read_variance;
int (*const denoise_guided_fn)(pt_ctx *, const pt_guided_params *, int, void *, size_t) = pt_denoise_guided;
