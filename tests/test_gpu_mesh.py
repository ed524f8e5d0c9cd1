"""GPU: pt_sample_field and pt_mesh_extract against the CPU oracle and the
numpy restatement of the contract (meshref.py), bit for bit
and in order (a NaN equal only to a NaN in the same place).

Shape numbering: the product's `shape` counts PT_OP_SHAPE ops in program
order (Hit.m - 1); the oracle's pto_map returns the shape's row in the editor
tree (map_ct stores o->cs[i], unions included in the count).  The two are
compared through the material: each number's albedo."""
import ctypes
import functools

import numpy as np
import pytest

import gpuharness as G
import meshref as M
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.path_tracer import Mesh, mesh_grid
from gpuharness import EYE, TARGET
from compute_path_tracer_amd.sdf_editor import CompData, SDFEditor
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
FP, IP, UP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
EXTRA = {"nan-sphere": M.nan_sphere_scene, "inf-sphere": M.inf_sphere_scene}


def editor(name) -> SDFEditor:
    return EXTRA[name]() if name in EXTRA else scenes.SCENES[name]()


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    return O.OracleScene(editor(name).rows())


@functools.lru_cache(maxsize=None)
def reference(name, grid, iso, project):
    """meshref's mesh, computed once and shared (read-only)."""
    return M.extract(oracle_scene(name), *grid, iso, project)


def _tracer_of(ed, **options):
    """A 16 x 16 context on the interpreter kernels unless `options` say otherwise."""
    return G.tracer(ed, 16, 16, 2, extra=dict({"jit": 0}, **options))


def tracer(name, **options):
    ed = editor(name)
    return _tracer_of(ed, **options), ed


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(G.same_or_nan(a, b).all())


def assert_matches(mesh: Mesh, ref, rows, prog, data=None, what=""):
    counted = ("n_vertices", "n_triangles", "clipped_edges", "void_cells", "dropped_quads", "bricks", "reserved")
    assert {k: mesh.info[k] for k in counted} == {k: ref["info"][k] for k in counted}, what
    assert same_bits(mesh.positions, ref["positions"]), f"{what}: positions"
    assert same_bits(mesh.normals, ref["normals"]), f"{what}: normals"
    assert np.array_equal(mesh.triangles, ref["triangles"]), f"{what}: triangles"
    assert np.array_equal(mesh.vertex_colors(prog, data), M.node_albedo(rows, ref["node"])), f"{what}: shapes"


def identical(a: Mesh, b: Mesh):
    return (a.positions.tobytes() == b.positions.tobytes() and a.normals.tobytes() == b.normals.tobytes() and
            a.shapes.tobytes() == b.shapes.tobytes() and a.triangles.tobytes() == b.triangles.tobytes())


# ---- field sampling --------------------------------------------------------------
def sample_points(n):
    """n points: the edge cases first, then a box around the scenes.  The far
    points stop at 1e30: next to f32's largest value a rotation's sum itself
    overflows, and the reference's full matrices then turn the inf into NaNs
    (0 * inf) where the kernels' skipped zero terms do not."""
    nan, inf = float("nan"), float("inf")
    special = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.5), (1e6, -2e6, 3e6), (1e20, 0.0, 0.0),
               (-1e30, 2e30, 3e30), (nan, 0.0, 0.0), (0.3, nan, 0.1), (nan, nan, nan), (inf, 0.0, 0.0),
               (0.5, -inf, 0.25), (inf, -inf, inf), (1e-30, 1e-38, -1e-45)]
    rng = np.random.default_rng(20)
    pts = np.concatenate([np.array(special, F), rng.uniform(-3.0, 3.0, (max(n, 0), 3)).astype(F)])
    return np.ascontiguousarray(pts[:n] if n != 1 else pts[13:14])


@pytest.mark.parametrize("name,jit", [("c2", 0), ("c2", 1), ("nested", 0), ("fuzz-56", 0), ("fuzz-56", 1),
                                      ("fuzz-15793", 0), ("fuzz-15793", 1)])
def test_sample_field_matches_the_oracle(gpu, name, jit):
    """0, 1 and 64 * 5 + 37 points (ragged against the 256-thread block); the
    same answers from a context with scene kernels and from one without."""
    pt, ed = tracer(name, jit=jit, jit_bake=0)
    prog, rows, sc = ed.compile(CompData()), ed.rows(), oracle_scene(name)
    for n in (0, 1, 64 * 5 + 37):
        pts = sample_points(n)
        d, shape = pt.sample_field(pts)
        want_d, want_node = M.field(sc, pts)
        assert d.shape == (n,) and shape.shape == (n,)
        assert same_bits(d, want_d), f"{name} jit {jit} n {n}: d differs at {np.nonzero(d.view(np.uint32) != want_d.view(np.uint32))[0][:5]}"
        got_albedo = Mesh(pts, pts, shape, np.zeros((0, 3))).vertex_colors(prog)
        assert np.array_equal(got_albedo, M.node_albedo(rows, want_node)), f"{name} jit {jit} n {n}: shape"
    pt.close()


def test_sample_field_outputs_are_optional(gpu):
    pt, _ = tracer("c2")
    pts = sample_points(50)
    d, s = pt.sample_field(pts)
    d2, s2 = np.empty(50, F), np.empty(50, np.int32)
    assert pt._L.pt_sample_field(pt._ctx, pts.ctypes.data_as(FP), 50, d2.ctypes.data_as(FP), None) == N.PT_OK
    assert pt._L.pt_sample_field(pt._ctx, pts.ctypes.data_as(FP), 50, None, s2.ctypes.data_as(IP)) == N.PT_OK
    assert pt._L.pt_sample_field(pt._ctx, pts.ctypes.data_as(FP), 50, None, None) == N.PT_OK
    assert d.tobytes() == d2.tobytes() and s.tobytes() == s2.tobytes()
    assert pt._L.pt_sample_field(pt._ctx, None, 5, d2.ctypes.data_as(FP), None) == N.PT_ERR_INVALID
    assert pt.get_option("sample_ms") > 0.0
    pt.close()


# ---- extraction ------------------------------------------------------------------
def grid_of(cells, lo=-2.0, hi=2.0):
    """A grid of cubic cells from `lo` whose longest axis spans about [lo, hi]; hashable."""
    cell = F((hi - lo) / max(cells))
    return ((lo, lo, lo), float(cell), tuple(cells))


GRIDS = {"c2": grid_of((19, 13, 21)), "nested": grid_of((24, 24, 24)), "fuzz-56": grid_of((24, 24, 24)),
         "fuzz-15793": grid_of((24, 24, 24))}


@pytest.mark.parametrize("iso", [0.0, 0.05])
@pytest.mark.parametrize("project", [0, 2])
@pytest.mark.parametrize("name", list(GRIDS))
def test_extract_matches_meshref_with_and_without_the_skip(gpu, name, project, iso):
    """c2 on 19 x 13 x 21 cells (ragged against the 8^3 bricks on every axis),
    the others on 24^3; mesh_skip 1 against meshref, mesh_skip 0 against that."""
    pt, ed = tracer(name)
    prog, rows, grid = ed.compile(CompData()), ed.rows(), GRIDS[name]
    meshes = {}
    for skip in (1, 0):
        pt.set_option("mesh_skip", skip)
        meshes[skip] = pt.extract_mesh(grid=grid, iso=iso, project=project)
    ref = reference(name, grid, iso, project)
    assert ref["info"]["n_vertices"] > 100
    assert_matches(meshes[1], ref, rows, prog, what=f"{name} project {project} iso {iso}")
    assert identical(meshes[0], meshes[1])
    i0, i1 = meshes[0].info, meshes[1].info
    varies = ("bricks_evaluated", "corner_evals", "device_bytes")
    assert {k: v for k, v in i0.items() if k not in varies} == {k: v for k, v in i1.items() if k not in varies}
    assert i0["bricks_evaluated"] == i0["bricks"] >= i1["bricks_evaluated"] >= 1
    # every corner of the clipped lattices, once per evaluated brick that holds it
    n = grid[2]
    per_axis = [sum(min(8, c - 8 * b) + 1 for b in range(-(-c // 8))) for c in n]
    assert i0["corner_evals"] == per_axis[0] * per_axis[1] * per_axis[2] >= i1["corner_evals"] > 0
    assert i0["device_bytes"] > 0 and pt.get_option("mesh_ms") > 0.0
    # two runs give identical bytes
    again = pt.extract_mesh(grid=grid, iso=iso, project=project)
    assert identical(again, meshes[0])
    pt.close()


def sphere_scene(radius, scale=1.0):
    ed = SDFEditor()  # one union, one unit sphere
    ed.header_unions[0].children_shapes[0].current_shape.params[0].set(radius)
    ed.header_unions[0].transform.scale.set(scale)
    return ed


def test_the_skip_really_skips(gpu):
    """A sphere of radius 0.5 in [-2, 2]^3 at cell 1/16: 512 bricks of side 0.5
    and half-diagonal 0.433.  Only the 8 bricks around the origin and the 24
    with one centre coordinate +-0.75 have their centre within 0.433 of it."""
    ed = sphere_scene(0.5)
    pt = _tracer_of(ed)
    assert np.isfinite(pt.get_option("bound_k"))
    grid = mesh_grid((-2, -2, -2), (2, 2, 2), 64)
    assert grid[2] == (64, 64, 64) and grid[1] == F(1.0 / 16.0)
    assert pt.get_option("mesh_skip") == 1.0  # the default
    on = pt.extract_mesh((-2, -2, -2), (2, 2, 2), resolution=64, project=2)
    pt.set_option("mesh_skip", 0)
    off = pt.extract_mesh((-2, -2, -2), (2, 2, 2), resolution=64, project=2)
    print(f"bricks evaluated: {on.info['bricks_evaluated']} of {on.info['bricks']} with the skip, "
          f"{off.info['bricks_evaluated']} without; {on.info['n_vertices']} vertices")
    assert on.info["bricks"] == off.info["bricks"] == 512
    assert 8 <= on.info["bricks_evaluated"] <= 64
    assert off.info["bricks_evaluated"] == 512
    assert identical(on, off) and on.info["n_vertices"] > 0
    assert M.is_closed_manifold(on.triangles, len(on.positions))
    # wound outward; a polyhedron with its vertices on the sphere and edges of h = r / 8 falls short of the
    # sphere's volume by the order of (h / r)^2 = 1.6 %
    assert M.signed_volume(on.positions, on.triangles) == pytest.approx(4.0 / 3.0 * np.pi * 0.125, rel=0.05)
    pt.close()


def test_a_scene_without_a_map_bound_evaluates_every_brick(gpu):
    """A union scale of 3 is outside [1/2, 2]: bound_k is NaN, nothing is skipped."""
    ed = sphere_scene(0.25, scale=3.0)  # radius 0.75 in world units
    pt = _tracer_of(ed)
    assert np.isnan(pt.get_option("bound_k"))
    grid = grid_of((20, 20, 20))
    mesh = pt.extract_mesh(grid=grid, project=1)
    assert mesh.info["bricks_evaluated"] == mesh.info["bricks"] == 27
    ref = M.extract(O.OracleScene(ed.rows()), *grid, 0.0, 1)
    assert ref["info"]["n_vertices"] > 100
    assert_matches(mesh, ref, ed.rows(), ed.compile(CompData()))
    pt.close()


@pytest.mark.parametrize("name", ["nan-position", "nan-sphere", "inf-sphere", "empty"])
def test_scenes_with_nan_and_void_fields(gpu, name):
    """nan-position has no non-finite corner (sdCube's min / max drop the NaN);
    nan-sphere is NaN everywhere, inf-sphere -inf or NaN: every cell void."""
    pt, ed = tracer(name)
    grid = M.INF_SPHERE_GRID if name == "inf-sphere" else grid_of((12, 9, 10))
    mesh = pt.extract_mesh(grid=grid, project=1)
    ref = reference(name, grid, 0.0, 1)
    assert_matches(mesh, ref, ed.rows(), ed.compile(CompData()), what=name)
    if name in ("nan-sphere", "inf-sphere"):
        assert mesh.info["void_cells"] == grid[2][0] * grid[2][1] * grid[2][2] and mesh.info["n_vertices"] == 0
    if name == "inf-sphere":
        assert mesh.info["dropped_quads"] > 0
    if len(mesh.triangles):
        assert mesh.triangles.max() < len(mesh.positions)
    pt.close()


def test_value_edits_and_snapshots(gpu):
    """A new extract after set_data matches meshref on the new data; the mesh
    extracted before stays readable, unchanged, until then."""
    ed = scenes.SCENES["c2"]()
    cd = CompData()
    prog = ed.compile(cd)
    pt = _tracer_of(prog)
    grid = GRIDS["c2"]
    first = pt.extract_mesh(grid=grid, project=2)
    sphere = ed.header_unions[0].children_shapes[1]
    sphere.current_shape.params[0].set(0.6)
    sphere.transform.position.set((-0.5, 0.4, 0.1))
    ed.data_update(cd)
    data = cd.data_array.as_array()
    pt.set_data(data)
    snapshot = pt.read_mesh(first.info)  # the scene edit did not invalidate it
    assert identical(snapshot, first)
    second = pt.extract_mesh(grid=grid, project=2)
    assert_matches(second, M.extract(O.OracleScene(ed.rows()), *grid, 0.0, 2), ed.rows(), prog, data, "after the edit")
    assert not identical(second, first)
    assert_matches(first, reference("c2", grid, 0.0, 2), scenes.SCENES["c2"]().rows(), prog, what="before the edit")
    pt.close()


def test_no_side_effects(gpu):
    """The image, the guides' validity, the camera, the sky and the options stay as they were."""
    pt, _ = tracer("c2", kernel="binned")
    k = G.constants(16, 16)
    pt.look_at(EYE, TARGET)
    pt.set_sky((0.9, 0.8, 0.7), (0.2, 0.4, 0.9))
    pt.dispatch(k, 2)
    before = pt.read_image()
    assert before[..., :3].mean() > 0
    pt.render_guides(k)
    state = [pt.get_option(o) for o in ("guides_valid", "kernel", "mesh_skip", "bin_lanes")]
    cam, sky = bytes(pt.get_camera()[0]), bytes(pt.get_sky()[0])
    g0 = pt.read_guides()[0]
    pt.sample_field(sample_points(100))
    pt.extract_mesh(grid=GRIDS["c2"], project=2)
    assert pt.read_image().tobytes() == before.tobytes()
    assert [pt.get_option(o) for o in ("guides_valid", "kernel", "mesh_skip", "bin_lanes")] == state and state[0] == 1.0
    assert bytes(pt.get_camera()[0]) == cam and bytes(pt.get_sky()[0]) == sky
    assert pt.read_guides()[0].tobytes() == g0.tobytes()
    # and the render goes on as if nothing had happened
    pt.clear()
    pt.dispatch(k, 2)
    assert pt.read_image().tobytes() == before.tobytes()
    pt.close()


def test_argument_and_state_errors(gpu):
    L = N.lib()
    pt = _tracer_of(None)
    desc = N.MeshDesc(cell=0.25, iso=0.0, project=1)
    for k in range(3):
        desc.origin[k], desc.cells[k] = -2.0, 16
    info = N.MeshInfo(n_vertices=77)
    pts, d = np.zeros((3, 3), F), np.full(3, 7.0, F)
    # before a program is set
    assert L.pt_sample_field(pt._ctx, pts.ctypes.data_as(FP), 3, d.ctypes.data_as(FP), None) == N.PT_ERR_STATE
    assert L.pt_mesh_extract(pt._ctx, ctypes.byref(desc), ctypes.byref(info)) == N.PT_ERR_STATE
    assert L.pt_mesh_read(pt._ctx, None, None, None, None, 0, 0) == N.PT_ERR_STATE
    assert (d == 7.0).all() and info.n_vertices == 77
    prog = scenes.SCENES["c2"]().compile(CompData())
    pt.remake_pipeline(prog)
    assert L.pt_mesh_extract(pt._ctx, ctypes.byref(desc), ctypes.byref(info)) == N.PT_ERR_STATE  # no data yet
    pt.set_data(prog.data)
    assert L.pt_mesh_read(pt._ctx, None, None, None, None, 0, 0) == N.PT_ERR_STATE  # no extract yet
    # bad descriptions: PT_ERR_INVALID, info untouched
    nan, inf = float("nan"), float("inf")
    for field, value in [("cell", 0.0), ("cell", -1.0), ("cell", nan), ("cell", inf), ("iso", nan), ("iso", -inf),
                         ("project", 9), ("origin", (nan, 0.0, 0.0)), ("origin", (0.0, inf, 0.0)),
                         ("cells", (0, 16, 16)), ("cells", (16, 1025, 16)), ("cells", (16, 16, 0xFFFFFFFF))]:
        bad = N.MeshDesc.from_buffer_copy(desc)
        if isinstance(value, tuple):
            for k in range(3):
                getattr(bad, field)[k] = value[k]
        else:
            setattr(bad, field, value)
        assert L.pt_mesh_extract(pt._ctx, ctypes.byref(bad), ctypes.byref(info)) == N.PT_ERR_INVALID, (field, value)
        assert info.n_vertices == 77
    assert L.pt_mesh_extract(pt._ctx, None, ctypes.byref(info)) == N.PT_ERR_INVALID
    assert L.pt_mesh_extract(pt._ctx, ctypes.byref(desc), None) == N.PT_ERR_INVALID
    assert L.pt_mesh_read(pt._ctx, None, None, None, None, 0, 0) == N.PT_ERR_STATE  # a refused extract leaves no mesh
    with pytest.raises(N.NativeError):
        pt.set_option("mesh_skip", 2)
    # the limits themselves are accepted: 1 and 1024 cells per axis
    for cells in [(1, 1, 1), (1024, 1, 2)]:
        ok = N.MeshDesc.from_buffer_copy(desc)
        for k in range(3):
            ok.cells[k] = cells[k]
        assert L.pt_mesh_extract(pt._ctx, ctypes.byref(ok), ctypes.byref(info)) == N.PT_OK, cells
        assert info.bricks == -(-cells[0] // 8) and info.reserved == 0
    # too-small caps: PT_ERR_SIZE, buffers untouched
    assert L.pt_mesh_extract(pt._ctx, ctypes.byref(desc), ctypes.byref(info)) == N.PT_OK
    nv, nt = info.n_vertices, info.n_triangles
    assert nv > 10 and nt > 10
    pos, nrm = np.full((nv, 3), 7.0, F), np.full((nv, 3), 8.0, F)
    shp, tri = np.full(nv, 9, np.int32), np.full((nt, 3), 5, np.uint32)
    args = (pos.ctypes.data_as(FP), nrm.ctypes.data_as(FP), shp.ctypes.data_as(IP), tri.ctypes.data_as(UP))
    assert L.pt_mesh_read(pt._ctx, *args, nv - 1, nt) == N.PT_ERR_SIZE
    assert L.pt_mesh_read(pt._ctx, *args, nv, nt - 1) == N.PT_ERR_SIZE
    assert L.pt_mesh_read(pt._ctx, None, None, args[2], None, 0, nt) == N.PT_ERR_SIZE
    assert (pos == 7.0).all() and (nrm == 8.0).all() and (shp == 9).all() and (tri == 5).all()
    # a cap only counts for an array that is asked for
    assert L.pt_mesh_read(pt._ctx, None, None, None, args[3], 0, nt) == N.PT_OK
    assert (pos == 7.0).all() and tri.max() < nv
    assert L.pt_mesh_read(pt._ctx, *args, nv, nt) == N.PT_OK
    assert np.isfinite(pos).all() and shp.min() >= -1 and shp.max() < 6
    pt.close()
