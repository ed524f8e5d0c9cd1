/*
 * abi_temporal_layout.c -- compile-time layout of pt_temporal_params
 * (include/pt_abi.h): 16 bytes, the field offsets the ctypes mirror
 * (_native.TemporalParams) and the #[repr(C)] block of INTEGRATION.md 2 rely
 * on, and the signatures of the temporal entry points.  Compiled, not run
 * (tests/test_abi_temporal.py: gcc -std=c11 -Wall -Wextra -Werror -pedantic).
 */
#include <stddef.h>

#include "pt_abi.h"

_Static_assert(sizeof(pt_temporal_params) == 16, "pt_temporal_params is 4 floats");
_Static_assert(offsetof(pt_temporal_params, max_history) == 0, "max_history");
_Static_assert(offsetof(pt_temporal_params, depth_tolerance) == 4, "depth_tolerance");
_Static_assert(offsetof(pt_temporal_params, normal_cos) == 8, "normal_cos");
_Static_assert(offsetof(pt_temporal_params, albedo_tolerance) == 12, "albedo_tolerance");
_Static_assert(PT_ERR_INVALID == -1 && PT_ERR_UNSUPPORTED == -3 && PT_ERR_STATE == -4 && PT_ERR_SIZE == -6,
               "the refusals' codes");
_Static_assert(PT_ABI_VERSION == 1, "additive change: the version stays");

/* the struct has a tag as well: a C caller may name it either way */
static const struct pt_temporal_params defaults = {16.0f, 0.05f, 0.9f, 0.1f};
const pt_temporal_params *const temporal_defaults = &defaults;

/* the entry points' signatures, as a C caller declares pointers to them */
int (*const temporal_accumulate_fn)(pt_ctx *, const pt_temporal_params *) = pt_temporal_accumulate;
int (*const temporal_reset_fn)(pt_ctx *) = pt_temporal_reset;
int (*const read_history_fn)(pt_ctx *, float *, float *, float *, size_t) = pt_read_history;
int (*const denoise_history_fn)(pt_ctx *, const pt_guided_params *, int, void *, size_t) = pt_denoise_history;
