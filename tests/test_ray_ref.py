"""Pins tests/rayref.py, the CPU reference of the ray queries,
without a GPU: its pixel picks against denoiseref.guides, the rule for a ray
that starts non-finite, the ray set's make-up, and SDFEditor.shape_nodes()'s
order against the compiled program's material slots."""
import numpy as np
import pytest

import denoiseref as D
import gpuharness as G
import meshref as M
import rayref as R
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.sdf_editor import CompData, Shape

W, H = 12, 8


@pytest.mark.parametrize("view", ["default", "pinhole", "lens"])
def test_pick_equals_the_guides(view):
    """Every pixel at 12 x 8, fixed and posed (the lens as its pinhole):
    (n, t) is g0 bit for bit, the node's albedo g1.rgb, hit g1.a."""
    rows = scenes.c2_sphere_box_torus().rows()
    cam = G.camera(view)
    g0, g1 = D.guides(rows, W, H, G.aspect(W, H), 1.0, cam)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)  # image order
    t, node, nrm = R.pick(rows, W, H, G.aspect(W, H), 1.0, cam, xy)
    hit = ~(t > np.float32(100.0))
    assert 0.1 < hit.mean() < 0.9  # both occur
    assert G.same_or_nan(t.reshape(H, W), g0[..., 3]).all()
    assert G.same_or_nan(nrm.reshape(H, W, 3), g0[..., :3]).all()
    assert np.array_equal(M.node_albedo(rows, node).reshape(H, W, 3), g1[..., :3])
    assert np.array_equal(hit.reshape(H, W).astype(np.float32), g1[..., 3])
    assert (node[~hit] == -1).all() and (nrm[~hit] == 0).all()


def test_trace_of_the_camera_rays_equals_pick():
    """trace() on the rays pick() builds gives pick()'s answers."""
    rows = scenes.c2_sphere_box_torus().rows()
    xy = np.array([(0, 0), (5, 3), (6, 4), (11, 7)])
    want = R.pick(rows, W, H, 1.5, 1.0, None, xy)
    F = np.float32
    rd = []
    for x, y in xy:
        v = [((F(x) / F(W)) * F(2.0) - F(1.0)) * F(1.5), (F(y) / F(H)) * F(2.0) - F(1.0), F(1.0)]
        l = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        rd.append([c / l for c in v])
    got = R.trace(rows, np.tile(np.array([0, 0, -3], F), (4, 1)), np.array(rd, F))
    for a, b in zip(got, want):
        assert G.same_or_nan(a.astype(F), b.astype(F)).all()


def test_a_ray_that_starts_non_finite_is_answered_by_definition():
    rows = scenes.c2_sphere_box_torus().rows()
    nan, inf = float("nan"), float("inf")
    ro = np.array([(nan, 0, -3), (0, 0, -3), (0, inf, -3), (0, 0, -3), (0, 0, -3)], np.float32)
    rd = np.array([(0, 0, 1), (0, nan, 1), (0, 0, 1), (-inf, 0, 1), (0, 0, 1)], np.float32)
    t, node, nrm = R.trace(rows, ro, rd)
    assert np.isnan(t[:4]).all() and (node[:4] == -1).all() and (nrm[:4] == 0).all()
    assert not np.signbit(nrm[:4]).any()
    assert np.isfinite(t[4]) and t[4] < 100.0 and node[4] >= 0  # the finite ray is traced (and hits c2's centre)


@pytest.mark.parametrize("name", ["c2", "c3", "c3_noaabb", "farbox", "nan-position"])
def test_ray_set(name):
    ro, rd = R.ray_set(name)
    again = R.ray_set(name)
    assert ro.tobytes() == again[0].tobytes() and rd.tobytes() == again[1].tobytes()
    assert ro.dtype == rd.dtype == np.float32 and ro.shape == rd.shape == (257, 3)
    finite = np.isfinite(ro).all(1) & np.isfinite(rd).all(1)
    assert (~finite).sum() == 2 and np.isnan(ro[255]).any() and np.isinf(rd[256]).any()
    assert ro[254, 0] == np.float32(1e20)
    assert ((rd == 0).sum(1) == 3).sum() == 1  # one zero direction
    assert ((rd[157:181] == 0).sum(1) >= 1).all()  # one component exactly 0
    lengths = np.linalg.norm(rd[187:207].astype(np.float64), axis=1)
    assert np.allclose(lengths[:10], 0.5, atol=1e-6) and np.allclose(lengths[10:], 2.0, atol=1e-6)
    if name in ("c2", "c3"):
        boxes = R._boxes(scenes.SCENES[name]().rows())
        faces = {float(v) for b in boxes for v in (*b[0], *b[1])}
        assert sum(any(float(v) in faces for v in o) for o in ro[224:254]) == 30
    if name == "c3_noaabb":
        assert R._boxes(scenes.SCENES[name]().rows()) == []


@pytest.mark.parametrize("name", ["c3", "nested", "wide"])
def test_shape_nodes_are_in_the_order_of_the_shape_ops(name):
    """Node k's albedo equals the albedo read through SHAPE op k's material
    slots -- with every shape's albedo made its own first, so the order is
    pinned, not just the multiset."""
    ed = scenes.SCENES[name]()
    nodes = ed.shape_nodes()
    assert all(isinstance(s, Shape) for s in nodes) and len(nodes) == sum(r["kind"] != 0 for r in ed.rows())
    for k, s in enumerate(nodes):
        s.material.color.set((0.001 * (k + 1), 0.5, 1.0 - 0.001 * k))
    assert [id(s) for s in ed.shape_nodes()] == [id(s) for s in nodes]
    prog = ed.compile(CompData())
    ops = [prog.ops[i] for i in range(prog.n_ops) if prog.ops[i].opcode == N.PT_OP_SHAPE]
    assert len(ops) == len(nodes) >= 3
    for k, (op, s) in enumerate(zip(ops, nodes)):
        got = [float(prog.data[op.material[j]]) for j in range(3)]
        assert got == [float(np.float32(v)) for v in s.material.color.vals()], (name, k)
