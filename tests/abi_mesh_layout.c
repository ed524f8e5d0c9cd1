/*
 * abi_mesh_layout.c -- compile-time layout of pt_mesh_desc and pt_mesh_info
 * (include/pt_abi.h): 36 and 48 bytes, the field offsets the ctypes mirrors
 * (_native.MeshDesc, _native.MeshInfo) and the #[repr(C)] blocks of
 * INTEGRATION.md 2 rely on.  Compiled, not run (tests/test_abi_mesh.py: gcc
 * -std=c11 -Wall -Wextra -Werror -pedantic).
 */
#include <stddef.h>

#include "pt_abi.h"

_Static_assert(sizeof(pt_mesh_desc) == 36, "pt_mesh_desc is 4 floats + 3 u32 + a float + a u32");
_Static_assert(offsetof(pt_mesh_desc, origin) == 0, "origin");
_Static_assert(offsetof(pt_mesh_desc, cell) == 12, "cell");
_Static_assert(offsetof(pt_mesh_desc, cells) == 16, "cells");
_Static_assert(offsetof(pt_mesh_desc, iso) == 28, "iso");
_Static_assert(offsetof(pt_mesh_desc, project) == 32, "project");

_Static_assert(sizeof(pt_mesh_info) == 48, "pt_mesh_info is 8 u32 + 2 u64");
_Static_assert(offsetof(pt_mesh_info, n_vertices) == 0, "n_vertices");
_Static_assert(offsetof(pt_mesh_info, n_triangles) == 4, "n_triangles");
_Static_assert(offsetof(pt_mesh_info, clipped_edges) == 8, "clipped_edges");
_Static_assert(offsetof(pt_mesh_info, void_cells) == 12, "void_cells");
_Static_assert(offsetof(pt_mesh_info, dropped_quads) == 16, "dropped_quads");
_Static_assert(offsetof(pt_mesh_info, bricks) == 20, "bricks");
_Static_assert(offsetof(pt_mesh_info, bricks_evaluated) == 24, "bricks_evaluated");
_Static_assert(offsetof(pt_mesh_info, reserved) == 28, "reserved");
_Static_assert(offsetof(pt_mesh_info, corner_evals) == 32, "corner_evals");
_Static_assert(offsetof(pt_mesh_info, device_bytes) == 40, "device_bytes");

_Static_assert(PT_MESH_BRICK == 8 && PT_MESH_MAX_CELLS == 1024 && PT_MESH_MAX_PROJECT == 8, "limits");
_Static_assert(PT_ABI_VERSION == 1, "additive change: the version stays");

/* the entry points' signatures, as a C caller declares pointers to them */
int (*const sample_field_fn)(pt_ctx *, const float *, uint32_t, float *, int32_t *) = pt_sample_field;
int (*const mesh_extract_fn)(pt_ctx *, const pt_mesh_desc *, pt_mesh_info *) = pt_mesh_extract;
int (*const mesh_read_fn)(pt_ctx *, float *, float *, int32_t *, uint32_t *, size_t, size_t) = pt_mesh_read;
