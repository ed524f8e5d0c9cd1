"""GPU: the ray queries (pt_trace_rays / pt_pick_pixels) bit
for bit against tests/rayref.py (pinned on the CPU by test_ray_ref.py) and
against the context's own guide images.  16 x 16 contexts unless said.  Floats
are compared with same_or_nan (a NaN equal only to a NaN in the same place);
shapes through each number's albedo: the product reports the PT_OP_SHAPE
ordinal, the reference the editor tree's row (test_gpu_mesh.py)."""
import ctypes
import functools

import numpy as np
import pytest

import gpuharness as G
import meshref as M
import rayref as R
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.path_tracer import Mesh
from compute_path_tracer_amd.sdf_editor import CompData
from gpuharness import EYE, TARGET

pytestmark = pytest.mark.gpu

F = np.float32
FP, IP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
SCENES = ["c2", "c3", "cull", "nested", "tiny", "farbox", "c3_noaabb", "wide", "nan-position"]


def _tracer(scene="c2", w=16, h=16, **options):
    return G.tracer(scene, w, h, 2, extra=options)


@functools.lru_cache(maxsize=None)
def _rays(name):
    ro, rd = R.ray_set(name)
    ro.setflags(write=False)
    rd.setflags(write=False)
    return ro, rd


@functools.lru_cache(maxsize=None)
def _reference(name):
    """rayref's answers for the scene's ray set, computed once and shared (read-only)."""
    ref = R.trace(scenes.SCENES[name]().rows(), *_rays(name))
    for a in ref:
        a.setflags(write=False)
    return ref


def _albedo(prog, shape, data=None):
    """The albedo of the product's shape ordinals (black for -1)."""
    s = np.asarray(shape, np.int32).reshape(-1)
    return Mesh(np.zeros((len(s), 3)), np.zeros((len(s), 3)), s, np.zeros((0, 3))).vertex_colors(prog, data)


def _assert_hits(got, want, prog, rows, what, data=None):
    t, node, nrm = want
    for name, a, b in (("t", got.t, t), ("normal", got.normal, nrm)):
        same = G.same_or_nan(np.asarray(a, F), np.asarray(b, F))
        assert same.all(), (what, name, np.argwhere(~same)[:5].tolist())
    same = (_albedo(prog, got.shape, data) == M.node_albedo(rows, node)).all(-1)
    assert same.all(), (what, "shape", np.nonzero(~same)[0][:5].tolist())
    assert np.array_equal(got.hit, ~(t > F(100.0))), (what, "hit")


@pytest.mark.parametrize("jit", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_caller_rays_match_the_reference(gpu, name, jit):
    ed = scenes.SCENES[name]()
    prog, rows = ed.compile(CompData()), ed.rows()
    ro, rd = _rays(name)
    want = _reference(name)
    hit = ~(want[0] > F(100.0))
    print(f"{name}: {int(hit.sum())} of {len(hit)} rays hit, {int(np.isnan(want[0]).sum())} NaN t")
    # both occur (nan-position: by the reference no ray of the set misses; 252 of its normals are NaN)
    assert hit.any() and ((~hit).any() or name == "nan-position")
    pt = _tracer(prog, jit=jit, jit_bake=0)
    got = pt.trace_rays(ro, rd)
    assert got.t.shape == (257,) and got.normal.shape == (257, 3) and got.point.shape == (257, 3)
    _assert_hits(got, want, prog, rows, f"{name} jit {jit}")
    # the non-finite rays: answered by definition
    assert np.isnan(got.t[255:]).all() and (got.shape[255:] == -1).all() and (got.normal[255:] == 0).all()
    assert (got.shape[~got.hit] == -1).all() and (got.normal[~got.hit] == 0).all()
    assert np.isnan(got.point[~got.hit]).all()
    with np.errstate(all="ignore"):
        assert G.same_or_nan(got.point[hit], (ro + rd * got.t[:, None])[hit]).all()
    assert pt.get_option("rays_ms") > 0.0
    pt.close()


def test_ragged_sizes_give_the_prefix(gpu):
    ro, rd = _rays("c2")
    pt = _tracer("c2")
    full = pt.trace_rays(ro, rd)
    for n in (1, 63, 64, 65, 257):
        got = pt.trace_rays(ro[:n], rd[:n])
        for a, b in ((got.t, full.t), (got.normal, full.normal)):
            assert G.same_or_nan(a, b[:n]).all(), n
        assert np.array_equal(got.shape, full.shape[:n]), n
    # the arrays are shaped like the input's leading dimensions; no rays is a no-op
    got = pt.trace_rays(ro[:6].reshape(2, 3, 3), rd[:6].reshape(2, 3, 3))
    assert got.t.shape == got.hit.shape == got.shape.shape == (2, 3) and got.normal.shape == got.point.shape == (2, 3, 3)
    assert G.same_or_nan(got.t.reshape(-1), full.t[:6]).all()
    assert pt.trace_rays(np.zeros((0, 3)), np.zeros((0, 3))).t.shape == (0,)
    assert pt._L.pt_trace_rays(pt._ctx, None, None, 0, None, None, None) == N.PT_OK
    pt.close()


def test_null_outputs(gpu):
    """A call with any two outputs NULL returns the third unchanged."""
    ro, rd = (np.ascontiguousarray(a[:100]) for a in _rays("c2"))
    pt = _tracer("c2")
    full = pt.trace_rays(ro, rd)
    img = pt.id_image()
    k = G.constants(16, 16)
    t, s, nrm = np.empty(100, F), np.empty(100, np.int32), np.empty((100, 3), F)
    L, o, d = pt._L, ro.ctypes.data_as(FP), rd.ctypes.data_as(FP)
    assert L.pt_trace_rays(pt._ctx, o, d, 100, t.ctypes.data_as(FP), None, None) == N.PT_OK
    assert L.pt_trace_rays(pt._ctx, o, d, 100, None, s.ctypes.data_as(IP), None) == N.PT_OK
    assert L.pt_trace_rays(pt._ctx, o, d, 100, None, None, nrm.ctypes.data_as(FP)) == N.PT_OK
    assert L.pt_trace_rays(pt._ctx, o, d, 100, None, None, None) == N.PT_OK
    assert G.same_or_nan(t, full.t).all() and np.array_equal(s, full.shape) and G.same_or_nan(nrm, full.normal).all()
    t, s, nrm = np.empty(256, F), np.empty(256, np.int32), np.empty((256, 3), F)
    pick = lambda *out: L.pt_pick_pixels(pt._ctx, ctypes.byref(k), ctypes.byref(pt.settings), None, 256, *out)  # noqa: E731
    assert pick(t.ctypes.data_as(FP), None, None) == N.PT_OK
    assert pick(None, s.ctypes.data_as(IP), None) == N.PT_OK
    assert pick(None, None, nrm.ctypes.data_as(FP)) == N.PT_OK
    assert G.same_or_nan(t, img.t.reshape(-1)).all() and np.array_equal(s, img.shape.reshape(-1))
    assert G.same_or_nan(nrm, img.normal.reshape(-1, 3)).all()
    pt.close()


@pytest.mark.parametrize("size", [(16, 16), (13, 7)], ids=["16x16", "13x7"])
@pytest.mark.parametrize("view", ["default", "pinhole", "lens"])
def test_id_image_equals_the_guides(gpu, view, size):
    """g0 is (normal, t) bit for bit, g1.rgb the albedo of shape, g1.a is hit;
    a lens equals its pinhole."""
    w, h = size
    ed = scenes.SCENES["c3"]()
    prog = ed.compile(CompData())
    pt = _tracer(prog, w, h)
    if view != "default":
        pt.look_at(EYE, TARGET, **G.LOOK[view])
    got = pt.id_image()
    assert pt.get_option("guides_valid") == 0.0 and pt.get_option("pick_ms") > 0.0
    pt.render_guides()
    g0, g1 = pt.read_guides()
    assert got.t.shape == got.shape.shape == (h, w) and got.normal.shape == (h, w, 3)
    assert G.same_or_nan(got.t, g0[..., 3]).all() and G.same_or_nan(got.normal, g0[..., :3]).all()
    assert np.array_equal(_albedo(prog, got.shape).reshape(h, w, 3), g1[..., :3])
    assert np.array_equal(got.hit.astype(F), g1[..., 3])
    assert got.hit.any() and len(np.unique(got.shape[got.hit])) >= 2
    if view == "lens":
        pt.look_at(EYE, TARGET)
        pin = pt.id_image()
        assert G.same_or_nan(pin.t, got.t).all() and np.array_equal(pin.shape, got.shape)
    pt.close()


def test_pixel_lists(gpu):
    """A shuffled subset of the pixels equals the same pixels of id_image(), on a ragged image."""
    w, h = 13, 7
    pt = _tracer("c3", w, h)
    pt.look_at(EYE, TARGET)
    img = pt.id_image()
    rng = np.random.default_rng(5)
    idx = rng.permutation(w * h)[:70]  # more than one wave, ragged
    xy = np.stack([idx % w, idx // w], -1).astype(np.int32)
    got = pt.pick_pixels(xy)
    assert got.t.shape == (70,)
    assert G.same_or_nan(got.t, img.t[xy[:, 1], xy[:, 0]]).all()
    assert G.same_or_nan(got.normal, img.normal[xy[:, 1], xy[:, 0]]).all()
    assert np.array_equal(got.shape, img.shape[xy[:, 1], xy[:, 0]])
    assert G.same_or_nan(got.point, img.point[xy[:, 1], xy[:, 0]]).all()
    # a pixel may be listed twice, and a list keeps its leading dimensions
    twice = pt.pick_pixels(np.array([[(3, 2), (3, 2)], [(0, 0), (12, 6)]]))
    assert twice.t.shape == (2, 2) and G.same_or_nan(twice.t[0, 0:1], twice.t[0, 1:2]).all()
    assert G.same_or_nan(twice.t[1], np.array([img.t[0, 0], img.t[6, 12]])).all()
    pt.close()


def test_pick_against_the_reference(gpu):
    """pt_pick_pixels against rayref.pick directly (posed camera, 13 x 7)."""
    w, h = 13, 7
    ed = scenes.SCENES["c2"]()
    prog, rows = ed.compile(CompData()), ed.rows()
    pt = _tracer(prog, w, h)
    pt.look_at(EYE, TARGET)
    xy = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2)
    want = R.pick(rows, w, h, G.aspect(w, h), 1.0, G.camera("pinhole"), xy)
    _assert_hits(pt.pick_pixels(xy), want, prog, rows, "pick")
    pt.close()


def test_editor_pick(gpu):
    """pick(x, y, editor) returns the node whose albedo the guide shows; None on a miss."""
    ed = scenes.SCENES["c3"]()
    pt = _tracer(ed)
    pt.render_guides()
    g0, g1 = pt.read_guides()
    nodes = ed.shape_nodes()
    seen = set()
    for y in range(0, 16, 3):
        for x in range(0, 16, 3):
            p = pt.pick(x, y, ed)
            assert p.hit == bool(g1[y, x, 3]) and G.same_or_nan(F(p.t), g0[y, x, 3])
            assert G.same_or_nan(np.asarray(p.normal, F), g0[y, x, :3]).all()
            if p.hit and p.shape >= 0:
                assert p.node is nodes[p.shape]
                assert [F(v) for v in p.node.material.color.vals()] == g1[y, x, :3].tolist()
                seen.add(p.shape)
            else:
                assert p.node is None
            assert pt.pick(x, y).node is None  # without an editor
    assert len(seen) >= 2
    pt.close()
    # a miss: the empty corner of the posed view
    pt = _tracer("c2")
    pt.look_at(EYE, TARGET)
    img = pt.id_image()
    assert (~img.hit).any()
    y, x = (int(v) for v in np.argwhere(~img.hit)[0])
    p = pt.pick(x, y, scenes.SCENES["c2"]())
    assert not p.hit and p.node is None and p.shape == -1 and np.isnan(p.point).all() and p.t > 100.0
    pt.close()


def test_after_a_value_edit(gpu):
    """After set_data moves a shape the answers follow the reference for the edited rows."""
    ed = scenes.SCENES["c2"]()
    cd = CompData()
    prog = ed.compile(cd)
    pt = _tracer(prog)
    ro, rd = _rays("c2")
    before = pt.trace_rays(ro, rd)
    sphere = ed.header_unions[0].children_shapes[1]
    sphere.current_shape.params[0].set(0.6)
    sphere.transform.position.set((-0.5, 0.4, 0.1))
    ed.data_update(cd)
    data = cd.data_array.as_array()
    pt.set_data(data)
    got = pt.trace_rays(ro, rd)
    _assert_hits(got, R.trace(ed.rows(), ro, rd), prog, ed.rows(), "after the edit", data)
    assert not G.same_or_nan(got.t, before.t).all()
    pt.close()


def test_no_side_effects(gpu):
    """render -> query -> render leaves the bits of render -> render; the guides'
    validity, the guides, the moments and the history stay as they were."""
    ro, rd = _rays("c2")
    a, b = (_tracer("c2", kernel="binned", moments=1) for _ in range(2))  # b never queries
    k = G.constants(16, 16, 1, 0)
    for pt in (a, b):
        pt.look_at(EYE, TARGET)
        pt.set_sky((0.9, 0.8, 0.7), (0.2, 0.4, 0.9))
        pt.set_tiles(0, 1)
        pt.dispatch(k, 2)
    assert a.get_option("guides_valid") == 0.0
    a.trace_rays(ro, rd)
    a.id_image(k)
    assert a.get_option("guides_valid") == 0.0  # a query renders no guides
    for pt in (a, b):
        pt.render_guides(k)
        pt.accumulate_history()
    state = lambda pt: [pt.get_option(o) for o in ("guides_valid", "moments_valid", "moment_frames", "history_valid",  # noqa: E731
                                                   "history_views", "kernel")]
    snap = lambda pt: b"".join(x.tobytes() for x in (pt.read_image(), *pt.read_guides(), pt.read_moments(),  # noqa: E731
                                                     *pt.read_history()))
    st, sn = state(a), snap(a)
    assert st[:5] == [1.0, 1.0, 2.0, 1.0, 1.0]
    cam, sky = bytes(a.get_camera()[0]), bytes(a.get_sky()[0])
    a.trace_rays(ro, rd)
    a.id_image(k)
    a.pick_pixels([(3, 4), (15, 15)], k)
    a.pick(8, 8)
    assert state(a) == st and snap(a) == sn == snap(b)
    assert bytes(a.get_camera()[0]) == cam and bytes(a.get_sky()[0]) == sky
    # ... whatever pt_set_tiles says: a query answers for every pixel
    a.set_tiles(1, 3)
    full = a.id_image(k)
    a.set_tiles(0, 1)
    assert G.same_or_nan(full.t, a.id_image(k).t).all()
    for pt in (a, b):
        pt.clear()
        pt.dispatch(k, 2)
    a.trace_rays(ro, rd)
    for pt in (a, b):
        pt.dispatch(G.constants(16, 16, 3, 2), 2)
    assert a.read_image().tobytes() == b.read_image().tobytes()
    assert a.read_moments().tobytes() == b.read_moments().tobytes()
    assert a.read_image()[..., :3].mean() > 0
    a.close()
    b.close()


def test_refusals_on_a_live_context(gpu):
    L = N.lib()
    k, s = G.constants(16, 16), N.Settings(0, 2, 1.0, 1.0, 0)
    kp, sp = ctypes.byref(k), ctypes.byref(s)
    rays = np.zeros((4, 3), F)
    rays[:, 2] = 1.0
    t, shape, nrm = np.full(4, 5.0, F), np.full(4, 7, np.int32), np.full((4, 3), 9.0, F)
    out = (t.ctypes.data_as(FP), shape.ctypes.data_as(IP), nrm.ctypes.data_as(FP))
    rp = rays.ctypes.data_as(FP)
    xy = np.array([(0, 0), (3, 3), (15, 15), (1, 2)], np.int32)
    xp = xy.ctypes.data_as(IP)
    untouched = lambda: (t == 5.0).all() and (shape == 7).all() and (nrm == 9.0).all()  # noqa: E731
    # no program, then no data
    pt = _tracer(None)
    assert L.pt_trace_rays(pt._ctx, rp, rp, 4, *out) == N.PT_ERR_STATE
    assert L.pt_pick_pixels(pt._ctx, kp, sp, xp, 4, *out) == N.PT_ERR_STATE
    assert L.pt_pick_pixels(pt._ctx, kp, sp, None, 256, None, None, None) == N.PT_ERR_STATE
    prog = scenes.SCENES["c2"]().compile(CompData())
    pt.remake_pipeline(prog)
    assert L.pt_trace_rays(pt._ctx, rp, rp, 4, *out) == N.PT_ERR_STATE
    pt.set_data(prog.data)
    assert untouched()
    # too many: refused on the count alone, before any access (the buffers hold 4)
    assert L.pt_trace_rays(pt._ctx, rp, rp, N.PT_RAYS_MAX + 1, *out) == N.PT_ERR_INVALID
    assert L.pt_pick_pixels(pt._ctx, kp, sp, xp, N.PT_RAYS_MAX + 1, *out) == N.PT_ERR_INVALID
    assert L.pt_pick_pixels(pt._ctx, kp, sp, None, N.PT_RAYS_MAX + 1, *out) == N.PT_ERR_INVALID
    assert L.pt_trace_rays(pt._ctx, rp, rp, 0xFFFFFFFF, *out) == N.PT_ERR_INVALID
    # missing inputs
    assert L.pt_trace_rays(pt._ctx, None, rp, 4, *out) == N.PT_ERR_INVALID
    assert L.pt_trace_rays(pt._ctx, rp, None, 4, *out) == N.PT_ERR_INVALID
    assert L.pt_pick_pixels(pt._ctx, None, sp, xp, 4, *out) == N.PT_ERR_INVALID
    assert L.pt_pick_pixels(pt._ctx, kp, None, xp, 4, *out) == N.PT_ERR_INVALID
    # every pixel means n = w * h
    for n in (4, 255, 257):
        assert L.pt_pick_pixels(pt._ctx, kp, sp, None, n, None, None, None) == N.PT_ERR_INVALID, n
    # a pixel outside the image: nothing is written, wherever it stands in the list
    for bad in ((16, 0), (-1, 0), (0, 16), (0, -1), (2 ** 31 - 1, 0)):
        for at in (0, 3):
            lst = xy.copy()
            lst[at] = bad
            assert L.pt_pick_pixels(pt._ctx, kp, sp, lst.ctypes.data_as(IP), 4, *out) == N.PT_ERR_INVALID, (bad, at)
            assert untouched()
    assert b"outside" in L.pt_last_error(pt._ctx)
    # and the next valid calls still work
    assert L.pt_pick_pixels(pt._ctx, kp, sp, xp, 4, *out) == N.PT_OK and not untouched()
    assert L.pt_pick_pixels(pt._ctx, kp, sp, None, 0, None, None, None) == N.PT_OK  # n = 0: a no-op
    assert L.pt_trace_rays(pt._ctx, rp, rp, 4, *out) == N.PT_OK
    pt.close()
