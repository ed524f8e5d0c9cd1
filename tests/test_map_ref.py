"""The point probes without a GPU: the probe modules' source is
the scene kernels' source up to the kernel list, it compiles, and every input
family of mapref.py yields what it claims -- checked with the oracle alone,
so test_gpu_map.py compares the kernels at the points it means to."""
import ctypes
import re

import numpy as np
import pytest

import mapref as M
from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData

F = np.float32
PROGRAMS = [(name, None) for name in sorted(scenes.SCENES)] + [(None, seed) for seed in scenes.FUZZ_SEEDS]


def _program(name, seed):
    return (scenes.SCENES[name]() if name else scenes.fuzz_scene(seed)).compile(CompData())


def test_the_source_prefix_covers_67_programs():
    assert len(PROGRAMS) == 67


@pytest.mark.parametrize("name,seed", PROGRAMS, ids=[n or f"seed-{s}" for n, s in PROGRAMS])
def test_probe_source_is_the_scene_source_up_to_the_kernel_list(name, seed):
    prog = _program(name, seed)
    for baked in (0, 1):
        src, probe = N.scene_kernel_source(prog, baked=baked), N.probe_kernel_source(prog, baked=baked)
        cut = src.index('extern "C" __global__')
        assert src[:cut].endswith("amdgpu_waves_per_eu(7)))\n")  # (the wave macros' last line)
        assert probe[:cut] == src[:cut]
        tail = probe[cut:]
        assert tail.startswith('#include "pt_map_probe.h"\n')
        kernels = re.findall(r'extern "C" __global__ __launch_bounds__\(64\) void (\w+)\(PtProbe P\)', tail)
        assert kernels == [k + s for k in ("pt_probe_map_jit", "pt_probe_map_b0_jit", "pt_probe_map_b1_jit",
                                           "pt_probe_taps_jit", "pt_probe_bounds_jit") for s in ("", "_stats")]
        assert "pt_bin_" not in tail and "pt_wave_jit" not in tail  # no scene kernel in a probe module


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_probe_source_compiles(name):
    """hipRTC cross-compiles without a device (as test_cull.py relies on): every probe kernel, both builds."""
    p = scenes.SCENES[name]().compile(CompData())
    for baked in (0, 1):
        log, size = ctypes.create_string_buffer(1 << 18), ctypes.c_size_t()
        rc = N.lib().pt_probe_jit_compile(p.ops, p.n_ops, p.aabbs, p.n_aabb, N.fptr(p.data), len(p.data), baked, log,
                                          len(log), ctypes.byref(size))
        assert rc == N.PT_OK, log.value.decode(errors="replace")[-3000:]
        assert size.value > 4096
        names = re.findall(r"Function Name: (\w+)", log.value.decode(errors="replace"))
        assert len(names) == 10 and all(n.startswith("pt_probe_") for n in names)


def test_probe_entry_points_refuse_a_null_context():
    L = N.lib()
    pts = np.zeros((4, 3), F)
    assert L.pt_probe_map(None, 0, 0, 4, N.fptr(pts), None, None, None, 0, None, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_taps(None, 1, 4, N.fptr(pts), None, None, None, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_bounds(None, 1, 0, None, None, 0, None, None, None) == N.PT_ERR_INVALID
    n = ctypes.c_size_t()
    assert L.pt_probe_kernel_source(None, 0, None, 0, None, 0, 0, None, 0, None) == N.PT_ERR_INVALID
    p = scenes.SCENES["c1"]().compile(CompData())
    args = (p.ops, p.n_ops, p.aabbs, p.n_aabb, N.fptr(p.data), len(p.data), 0)
    assert L.pt_probe_kernel_source(*args, None, 0, ctypes.byref(n)) == N.PT_OK
    buf = ctypes.create_string_buffer(n.value)
    assert L.pt_probe_kernel_source(*args, buf, n.value - 1, ctypes.byref(n)) == N.PT_ERR_SIZE


# ---- the families yield what they claim ----------------------------------------------
@pytest.mark.parametrize("name", ["c2", "c3", "cull", "tiny", "wide"])
def test_logged_masks_equal_bounds(name):
    sc = M.scene(name)
    ro, rd, mask = sc.segments[:3]
    assert len(ro) > 300
    assert np.array_equal(sc.bounds(ro[:300], rd[:300]), mask[:300])


def test_bound_k_restated():
    """mapref's pt_bound_k: c2's chain by hand, and NaN for a scale outside [1/2, 2].  c2 has unit scales
    and header unions at the origin; its floor, at (0, -2, 1) with half-extents (6, 0.5, 6), reaches
    furthest: |pos|_1 + |b| = 3 + sqrt(72.25) = 11.5 (every term exact in float32), against 5.6 for the
    light, 2.25 for the cube, 2.0 for the sphere and 1.57 for the tori."""
    assert M.scene("c2").bound_k == F(11.5 * (1.0 + 2.0 ** -20))
    assert np.isnan(M.scene("tiny").bound_k)  # (union scale 1e-3)


@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_boxes_are_the_programs_and_the_oracles(name):
    """mapref's boxes, one per entry of the program's box list: the oracle's bounds() sets the box's check[]
    entry for a ray through its centre, and clears it for the same ray moved sideways past the box (where
    no other box shares the entry); the rays aimed at corners and edges come from the whole list."""
    sc = M.scene(name)
    lo, hi = sc.boxes
    assert len(lo) == sc.prog.n_aabb == len(sc.backs)
    pinned = 0
    for b, back in enumerate(sc.backs):
        if not (np.isfinite(lo[b]).all() and np.isfinite(hi[b]).all() and (hi[b] > lo[b]).all() and
                np.abs(np.concatenate([lo[b], hi[b]])).max() < 1e6):
            continue
        centre, diag = (lo[b].astype(np.float64) + hi[b]) / 2, float(np.linalg.norm(hi[b].astype(np.float64) - lo[b]))
        o = centre + np.array([0.3, 0.2, -1.0]) * (2.0 * diag + 1.0)
        d = centre - o
        side = np.cross(d, [0.0, 1.0, 0.0])
        side *= 3.0 * diag / np.linalg.norm(side)
        m = sc.bounds([o, o + side], [d, d])
        bit = (m[:, back >> 6] >> np.uint64(back & 63)) & np.uint64(1)
        assert bit[0] == 1, (name, b, lo[b], hi[b])
        if sc.backs.count(back) == 1:
            assert bit[1] == 0, (name, b, lo[b], hi[b])
        pinned += 1
    assert pinned >= min(1, len(lo)) or name in ("inf-sphere",)  # (its one box is infinite)
    if name == "boxed72":  # corner and edge rays reach boxes whose bits sit in mask words 2-3
        ro, rd, fam, _ = M.ray_inputs(name)
        want = sc.bounds(ro[fam == 1], rd[fam == 1])
        assert want[:, 1].any() and want[:, 0].any()


@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_eligible_unions_are_the_generated_maps(name):
    """mapref's reading of 3.12 (`eligible`) against the generated JitMap itself: the unions that carry a
    cull target are the eligible ones whose parent has combined something before them (a fresh parent's
    union gets no tests), and every live bit belongs to a shape of a top-level eligible union, with that
    shape's own check[] entry."""
    sc = M.scene(name)
    g, rows = sc.generated, sc.rows
    with_target = {sc.row_of_op[i] for i in g["cull_unions"] + g["cull_off"]}
    eligible = {s["union"] for s in sc.shapes if s["eligible"]}
    fresh = {u for u in eligible if not any(r["parent"] == rows[u]["parent"] for r in rows[:u])}
    assert with_target == eligible - fresh, (name, with_target, eligible, fresh)
    by_check = {}
    for s in sc.shapes:
        by_check.setdefault(s["check"], []).append(s)
    assert len({bit for bit, _ in g["live"]}) == len(g["live"]) <= 64
    for bit, k in g["live"]:
        assert any(s["eligible"] and rows[s["union"]]["parent"] < 0 for s in by_check[k]), (name, bit, k)
    top = sum(1 for s in sc.shapes if s["eligible"] and rows[s["union"]]["parent"] < 0)
    assert len(g["live"]) <= top


@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_cube_features_have_the_claimed_number_of_positive_q(name):
    sc = M.scene(name)
    pts, which, what = M.cube_points(sc, 3)
    want = {"face": 1, "edge": 2, "corner": 3, "inside": 0}
    for p, k, feature in zip(pts, which, what):
        s = sc.shapes[k]
        q = np.abs(M.to_local(s, p.astype(np.float64))[0]) - np.array(s["size"])
        # what the float32 rounding of the world point can move a local coordinate by: a few of its ulps,
        # in the shape's units
        tol = 8.0 * 2.0 ** -24 * max(1e-3, float(np.abs(p).max())) / s["world"]
        if feature == "surface":
            assert abs(q.max()) < tol, (name, s["row"], q)
        elif np.abs(q).min() > tol:  # (the rounding cannot flip these)
            assert int((q > 0).sum()) == want[feature], (name, s["row"], feature, q)


@pytest.mark.parametrize("name", ["c2", "boxed72"])  # (every shape behind a box: one bit isolates a shape)
def test_surface_points_lie_on_their_shape(name):
    """The oracle alone: with only the shape's own check[] bit set, map() within 1e-4 (in the shape's world
    scale) of zero on the shape's surface points and -R * s at a sphere's local origin -- which also pins
    mapref's transform chain to the oracle's."""
    sc = M.scene(name)
    rng = np.random.default_rng(2)
    checked = 0
    for s in sc.shapes:
        boxless = [t for t in sc.shapes if t["check"] < 0]
        if s["check"] < 0 or boxless or not np.isfinite(s["world"]):
            continue
        v = rng.normal(size=(6, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        world = M.to_world(s, M.surface_points(s, v)).astype(F)
        mask = np.zeros((len(world), 2), np.uint64)
        mask[:, s["check"] >> 6] = np.uint64(1 << (s["check"] & 63))
        d = sc.map(world, mask)[0]
        tol = 1e-4 * max(1.0, s["world"]) + 4e-6 * float(np.abs(world).max())
        assert (np.abs(d) < tol).all(), (name, s["row"], d)
        if s["kind"] == N.PT_NODE_SPHERE:
            d0 = sc.map(M.to_world(s, np.zeros((1, 3))).astype(F), mask[:1])[0][0]
            assert abs(d0 + s["size"][0] * s["world"]) < tol, (name, s["row"], d0)
        checked += 1
    assert checked >= 3


@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_hits_and_bounds(name):
    sc, H = M.scene(name), M.hit_inputs(name)
    if name in ("nan-sphere", "inf-sphere", "tiny"):  # map() is NaN / -inf, or the specks are never hit: no hit to tap
        assert len(H["hits"]) == 0 or name == "tiny"
    if not len(H["hits"]):
        return
    f = sc.map(H["hits"], H["masks"])[0]
    assert (np.abs(f[~H["displaced"]]) < 1e-4).all()
    assert (np.abs(f[H["displaced"]]) < 1e-4 + 2e-4 * np.sqrt(3) * 1.001).all()
    b, d6 = H["bounds"], H["d6"]
    finite = np.isfinite(d6).all(1)
    assert (b["tightest"][finite][:, None] >= d6[finite]).all()
    assert np.isinf(b["tightest"][~finite]).all() and np.isinf(b["pipeline"][~finite]).all()
    # a condition on the inputs (3.13's contract): the pipeline's bound is an upper bound on every tap value
    rule_on = finite & ~np.isnan(b["pipeline"])
    assert np.isnan(sc.bound_k) or rule_on.sum() == finite.sum()
    bad = np.nonzero(rule_on & ~(b["pipeline"] >= b["tightest"]))[0]
    assert not len(bad), (name, H["hits"][bad[:3]], b["pipeline"][bad[:3]], b["tightest"][bad[:3]])
    assert np.array_equal(H["taps"].reshape(-1, 3)[::6, 1:], H["hits"][:, 1:])  # tap 0 moves x only


@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_orders_are_permutations_and_ragged(name):
    pts, masks, pf, mf = M.map_inputs(name)
    n = len(pts)
    assert n % 64 == 37 and n > 64 * 8
    order = M.interleave(n)
    assert np.array_equal(np.sort(order), np.arange(n))
    # interleaved: the waves mix point families and mask families; grouped: most waves hold one of each
    mixed = sum(len(set(pf[order[w:w + 64]])) > 1 and len(set(mf[order[w:w + 64]])) > 1 for w in range(0, n - 63, 64))
    pure = sum(len(set(pf[w:w + 64])) == 1 and len(set(mf[w:w + 64])) == 1 for w in range(0, n - 63, 64))
    assert mixed == n // 64 and pure >= 5
    ro, rd, fam, _ = M.ray_inputs(name)
    assert len(ro) % 64 == 37 and len(M.skip_rays(name)[0]) % 64 == 37


@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_census(name):
    """Per scene: every mask family and every point family the scene can have, the single bits covering
    every check[] entry, both fast_cube kinds where the scene has them, points inside and outside 2 R of
    every shape of a union whose cull rule is on in the generated JitMap, and every ray family the scene's
    boxes allow."""
    sc = M.scene(name)
    pts, masks, pf, mf = M.map_inputs(name)
    cubes = [s for s in sc.shapes if s["kind"] == N.PT_NODE_CUBE and min(s["size"]) > 0 and np.isfinite(s["size"]).all()]
    families = {"specials", "box", "path", "around"}  # (a path has its ray's origin at least)
    if cubes:
        families.add("cube")
    assert {M.POINT_FAMILIES[i] for i in set(pf)} == families
    assert set(mf) == set(range(len(M.MASK_FAMILIES)))
    valid_lo = (1 << min(sc.n_check, 64)) - 1
    ones, zeros = masks[mf == 0], masks[mf == 1]
    assert (ones[:, 0] == np.uint64(valid_lo)).all() and not zeros.any()
    logged = {tuple(m) for m in sc.segments[2].tolist()}
    assert {tuple(m) for m in masks[mf == 2].tolist()} <= logged
    assert len(logged) >= min(3, 1 + sc.prog.n_aabb)  # (without a box every ray has the one mask)
    assert len({tuple(m) for m in masks[mf == 3].tolist()}) > min(50, 2 ** sc.n_check // 2)
    single = masks[mf == 4]
    bits = [bin(int(a)).count("1") + bin(int(b)).count("1") for a, b in single.tolist()]
    assert set(bits) == {1}
    assert {int(a).bit_length() - 1 if a else 64 + int(b).bit_length() - 1 for a, b in single.tolist()} == \
        set(range(sc.n_check))
    if sc.n_check > 64:
        assert masks[:, 1].any()
    cpts, which, what = M.cube_points(sc, 3)
    kinds = {sc.shapes[k]["fast_cube"] for k in which}
    assert kinds == {s["fast_cube"] for s in cubes}
    if name in ("c3", "cull"):
        assert kinds == {True, False}
    assert {"face", "edge", "corner", "inside", "surface"} <= set(what) or not cubes
    apts, awhich, ratio = M.around_points(sc, 2)
    culling = {sc.row_of_op[i] for i in sc.generated["cull_unions"]}
    assert culling or name in ("fuzz-15793", "chain8", "nan-sphere", "inf-sphere")  # (no target, or its rule off by values)
    for k, s in enumerate(sc.shapes):
        if s["union"] in culling:
            assert np.isfinite(s["R"]) and s["R"] >= 0
            r = ratio[awhich == k]
            assert (r < 2.0).any() and (r > 2.0).any() and r.max() > 32.0, (name, k)
    lo, hi = sc.boxes
    aimable = (np.isfinite(lo).all(1) & np.isfinite(hi).all(1) & (np.abs(lo) < 1e6).all(1) & (np.abs(hi) < 1e6).all(1)).any()
    assert set(M.ray_inputs(name)[2]) == ({0, 1, 2, 3} if aimable else {0, 3})
