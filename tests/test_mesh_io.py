"""Mesh, mesh_grid and the OBJ / PLY writers, on the host: each file read back
by a small parser here; vertex_colors on c2's materials."""
import struct

import numpy as np
import pytest

from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.path_tracer import Mesh, mesh_grid
from compute_path_tracer_amd.sdf_editor import CompData


def tetrahedron():
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.1, 0.2, 1.0 / 3.0]], np.float32)
    nrm = np.array([[-1, -1, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.uint32)
    return Mesh(pos, nrm, np.array([0, 1, -1, 4], np.int32), tri, {"n_vertices": 4, "n_triangles": 4})


def read_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        tok = line.split()
        if not tok or tok[0].startswith("#"):
            continue
        if tok[0] == "v":
            v.append([float(x) for x in tok[1:]])
        elif tok[0] == "vn":
            vn.append([float(x) for x in tok[1:]])
        elif tok[0] == "f":
            corners = [t.split("/") for t in tok[1:]]
            assert all(len(c) == 3 and c[1] == "" and c[0] == c[2] for c in corners), line  # a//a
            f.append([int(c[0]) - 1 for c in corners])
        else:
            raise AssertionError(f"unexpected record {line!r}")
    return np.array(v, np.float32), np.array(vn, np.float32), np.array(f, np.uint32)


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, cur = {}, {}, None
    for line in lines[2:]:
        tok = line.split()
        if tok[:1] == ["element"]:
            cur = tok[1]
            counts[cur], props[cur] = int(tok[2]), []
        elif tok[:1] == ["property"]:
            props[cur].append(tok[1:])
    assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    fmt = {"float": "f", "uchar": "B"}
    vfmt = "<" + "".join(fmt[p[0]] for p in props["vertex"])
    names = [p[1] for p in props["vertex"]]
    off = end
    verts = []
    for _ in range(counts["vertex"]):
        verts.append(struct.unpack_from(vfmt, raw, off))
        off += struct.calcsize(vfmt)
    faces = []
    for _ in range(counts["face"]):
        n, a, b, c = struct.unpack_from("<Biii", raw, off)
        assert n == 3
        faces.append((a, b, c))
        off += 13
    assert off == len(raw)
    return names, np.array(verts, np.float64).reshape(-1, len(names)), np.array(faces, np.uint32).reshape(-1, 3)


def test_obj_round_trip(tmp_path):
    m = tetrahedron()
    path = tmp_path / "mesh.obj"
    m.save_obj(str(path))
    v, vn, f = read_obj(path)
    assert np.array_equal(v.view(np.uint32), m.positions.view(np.uint32))  # %.9g round-trips a float32
    assert np.array_equal(vn.view(np.uint32), m.normals.view(np.uint32))
    assert np.array_equal(f, m.triangles)


@pytest.mark.parametrize("colored", [False, True])
def test_ply_round_trip(tmp_path, colored):
    m = tetrahedron()
    colors = np.array([[0, 0, 0], [1, 0.5, 0.25], [2.0, -1.0, 0.2], [0.4, 0.8, 1.0]], np.float32) if colored else None
    path = tmp_path / "mesh.ply"
    m.save_ply(str(path), colors)
    names, v, f = read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz"] + (["red", "green", "blue"] if colored else [])
    assert np.array_equal(v[:, :3].astype(np.float32).view(np.uint32), m.positions.view(np.uint32))
    assert np.array_equal(v[:, 3:6].astype(np.float32).view(np.uint32), m.normals.view(np.uint32))
    assert np.array_equal(f, m.triangles)
    if colored:
        assert v[:, 6:].tolist() == [[0, 0, 0], [255, 128, 64], [255, 0, 51], [102, 204, 255]]
        with pytest.raises(ValueError):
            m.save_ply(str(path), colors[:3])


def test_an_empty_mesh_writes_valid_files(tmp_path):
    m = Mesh(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3)))
    m.save_obj(str(tmp_path / "e.obj"))
    m.save_ply(str(tmp_path / "e.ply"))
    assert all(len(a) == 0 for a in read_obj(tmp_path / "e.obj"))
    names, v, f = read_ply(tmp_path / "e.ply")
    assert len(v) == len(f) == 0 and len(names) == 6


def test_vertex_colors_on_c2():
    """c2's shape ops in program order: torus, sphere, torus, box, light, floor."""
    ed = scenes.SCENES["c2"]()
    prog = ed.compile(CompData())
    shape_rows = [r for r in ed.rows() if r["kind"] != N.PT_NODE_UNION]
    assert len(shape_rows) == 6
    m = Mesh(np.zeros((8, 3)), np.zeros((8, 3)), np.array([1, 0, 3, -1, 5, 2, 4, 1], np.int32), np.zeros((0, 3)))
    got = m.vertex_colors(prog)
    want = np.array([shape_rows[s]["material"][:3] if s >= 0 else [0, 0, 0] for s in m.shapes], np.float32)
    assert np.array_equal(got, want)
    assert got[0].tolist() == np.array([0.9, 0.25, 0.2], np.float32).tolist()  # the sphere
    # explicit data: an edited albedo shows
    data = prog.data.copy()
    sphere_op = [prog.ops[i] for i in range(prog.n_ops) if prog.ops[i].opcode == N.PT_OP_SHAPE][1]
    data[sphere_op.material[1]] = 0.75
    assert m.vertex_colors(prog, data)[0].tolist() == np.array([0.9, 0.75, 0.2], np.float32).tolist()
    with pytest.raises(ValueError):
        Mesh(np.zeros((1, 3)), np.zeros((1, 3)), np.array([6]), np.zeros((0, 3))).vertex_colors(prog)


def test_mesh_grid():
    origin, cell, cells = mesh_grid((-2, -2, -2), (2, 2, 2), 64)
    assert origin.dtype == np.float32 and origin.tolist() == [-2.0, -2.0, -2.0]
    assert cell == np.float32(1.0 / 16.0) and cells == (64, 64, 64)
    # cubic cells: the longest axis gets `resolution`, the others as many as cover them
    origin, cell, cells = mesh_grid((0, 0, 0), (1.0, 0.5, 0.26), 10)
    assert cell == np.float32(np.float32(1.0) / np.float32(10)) and cells == (10, 5, 3)
    assert mesh_grid((0, 0, 0), (8, 1e-3, 8), 4)[2] == (4, 1, 4)
    for bad in [((0, 0, 0), (1, 0, 1), 8), ((0, 0, 0), (1, 1, float("inf")), 8), ((0, 0, 0), (1, 1, 1), 0),
                ((0, 0, 0), (1, 1, 1), 1025), ((0, 0), (1, 1), 8)]:
        with pytest.raises(ValueError):
            mesh_grid(*bad)
