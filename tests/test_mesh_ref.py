"""The surface-nets contract of meshref.py on analytic scenes,
without a GPU: what the algorithm itself must deliver -- closed manifold
meshes wound outward, of the right genus and volume, vertices on the surface
after projection -- and its counts on a cut box, a void scene and an empty
one.  test_gpu_mesh.py then holds the kernels to meshref bit for bit."""
import functools
import math

import numpy as np
import pytest

import meshref as M
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.sdf_editor import SDFEditor, Shape, Shapes, Union
from oracle import oracle as O

ORIGIN, CELL, CELLS = (-2.0, -2.0, -2.0), 1.0 / 16.0, (64, 64, 64)  # box [-2, 2]^3


def torus_scene():
    t = Shape(Shapes.TORUS)
    for p, v in zip(t.current_shape.params, (1.0, 0.35)):
        p.set(v)
    u = Union()
    u.children_shapes.append(t)
    return SDFEditor([u])


SCENES = {"sphere": scenes.c1_default, "torus": torus_scene}
# (Euler characteristic, volume, relative volume bound)
WANT = {"sphere": (2, 4.0 * math.pi / 3.0, 0.01), "torus": (0, 2.0 * math.pi ** 2 * 1.0 * 0.35 ** 2, 0.02)}


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    return O.OracleScene(SCENES[name]().rows())


@functools.lru_cache(maxsize=None)
def mesh(name, project):
    return M.extract(oracle_scene(name), ORIGIN, CELL, CELLS, 0.0, project)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_closed_manifold_outward_with_the_right_genus_and_volume(name):
    m = mesh(name, 0)
    nv = len(m["positions"])
    euler, volume, bound = WANT[name]
    assert m["info"]["clipped_edges"] == m["info"]["void_cells"] == m["info"]["dropped_quads"] == 0
    assert m["info"]["n_triangles"] == len(m["triangles"]) and m["triangles"].max() < nv
    assert M.is_closed_manifold(m["triangles"], nv)
    assert M.euler_characteristic(m["triangles"], nv) == euler
    got = M.signed_volume(m["positions"], m["triangles"])
    print(f"{name}: {nv} vertices, {len(m['triangles'])} triangles, volume {got:.5f} ({(got / volume - 1) * 100:+.2f} %)")
    assert abs(got / volume - 1.0) < bound  # (positive: wound outward)
    if name == "sphere":  # the figures of the numpy prototype this contract was drafted from
        assert (nv, len(m["triangles"])) == (4760, 9516)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_projection_puts_vertices_on_the_surface(name):
    sc = oracle_scene(name)
    before = np.abs(M.field(sc, mesh(name, 0)["positions"])[0])
    m = mesh(name, 2)
    after = np.abs(M.field(sc, m["positions"])[0])
    print(f"{name}: |map(v)| median {np.median(before):.3g} at project 0, max {after.max():.3g} at project 2")
    assert after.max() < np.median(before)
    # the same topology, and normals that are the field's gradient: unit length, pointing outward
    assert np.array_equal(m["triangles"], mesh(name, 0)["triangles"])
    assert np.allclose(np.linalg.norm(m["normals"], axis=1), 1.0, atol=1e-5)
    if name == "sphere":
        assert (np.einsum("ij,ij->i", m["normals"], m["positions"]) > 0.99).all()


def test_a_box_that_cuts_the_sphere_counts_its_clipped_edges():
    m = M.extract(oracle_scene("sphere"), (0.0, -2.0, -2.0), 1.0 / 8.0, (16, 32, 32), 0.0, 0)
    nv = len(m["positions"])
    assert m["info"]["clipped_edges"] > 0 and nv > 0
    assert not M.is_closed_manifold(m["triangles"], nv)  # a boundary exists
    e = M.directed_edges(m["triangles"])
    code, rev = e[:, 0] * nv + e[:, 1], e[:, 1] * nv + e[:, 0]
    assert len(np.setdiff1d(code, rev)) > 0
    assert (m["positions"][:, 0] >= 0.0).all()


def test_the_nan_position_scene_has_no_void_cell_and_only_valid_indices():
    """scenes.nan_cube: the cube's coordinates are NaN, but sdCube's min / max
    drop NaNs, so its distance is 0 everywhere (the scene's own docstring) and
    map() = min(octahedron, 0) is finite at every corner: this scene has no
    void cell (measured: 0 of 4096), only the octahedron's surface.  The scenes
    whose map() really is non-finite follow."""
    ed = scenes.SCENES["nan-position"]()
    m = M.extract(O.OracleScene(ed.rows()), (-2.0, -2.0, -2.0), 0.25, (16, 16, 16), 0.0, 1)
    assert m["info"]["void_cells"] == 0 and m["info"]["n_vertices"] > 0
    assert m["triangles"].max() < len(m["positions"])
    assert np.isfinite(m["positions"]).all()


def test_a_nan_field_is_all_void():
    """A sphere at a NaN position in the last header union: opUnion keeps the
    NaN, every corner is NaN (outside), every cell void, nothing is emitted."""
    m = M.extract(O.OracleScene(M.nan_sphere_scene().rows()), (-2.0, -2.0, -2.0), 0.5, (8, 8, 8), 0.0, 1)
    assert m["info"]["void_cells"] == 512
    assert m["info"]["n_vertices"] == m["info"]["n_triangles"] == m["info"]["dropped_quads"] == 0


def test_void_cells_drop_their_quads_and_every_emitted_index_is_valid():
    """A sphere of infinite radius seen from 1.8e19 away: |p|^2 overflows in
    part of the grid, where the distance is inf - inf = NaN (outside); elsewhere
    it is -inf (inside).  Every cell is void; the edges between the two regions
    change sign, emit nothing and are counted."""
    grid = M.INF_SPHERE_GRID
    m = M.extract(O.OracleScene(M.inf_sphere_scene().rows()), *grid, 0.0, 1)
    assert m["info"]["void_cells"] == 512 and m["info"]["dropped_quads"] > 0 and m["info"]["clipped_edges"] > 0
    assert m["info"]["n_vertices"] == m["info"]["n_triangles"] == 0 and len(m["triangles"]) == 0


def test_the_empty_scene_has_no_vertices():
    m = M.extract(O.OracleScene(scenes.SCENES["empty"]().rows()), (-2.0, -2.0, -2.0), 0.5, (8, 8, 8), 0.0, 2)
    assert m["info"]["n_vertices"] == m["info"]["n_triangles"] == 0
    assert m["info"]["clipped_edges"] == m["info"]["void_cells"] == 0


def test_iso_offsets_the_surface():
    """inside <=> map(p) < iso: the unit sphere at iso 0.25 is the sphere of radius 1.25."""
    m = M.extract(oracle_scene("sphere"), (-2.0, -2.0, -2.0), 0.125, (32, 32, 32), 0.25, 2)
    r = np.linalg.norm(m["positions"].astype(np.float64), axis=1)
    assert np.abs(r - 1.25).max() < 1e-5
    assert M.is_closed_manifold(m["triangles"], len(m["positions"]))
