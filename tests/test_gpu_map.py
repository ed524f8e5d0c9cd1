"""GPU: the scene kernels' map() variants and bounds() point by point against
the CPU oracle, bit for bit, no tolerance and no excluded
input.  The probes (pt_probe_map / pt_probe_taps / pt_probe_bounds) run the
interpreter ahead of time and the scene's own generated JitMap, JitMapB0,
JitMapB1 and bounds() -- values from the node table and baked -- on the
inputs of mapref.py; a failure names the point, the family, the mask and the
variant.  test_map_ref.py checks, without a GPU, that the inputs are what
they claim."""
import numpy as np
import pytest

import fuzzref
import gpuharness as G
import mapref as M
from compute_path_tracer_amd import _native as N, scenes
from compute_path_tracer_amd.sdf_editor import CompData

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = ("interp", "table", "baked")
GENERATED = ("table", "baked")
# every scene once per kind (DESIGN.md 3.29 lists what each scene brings and what its probe modules cost)
CASES = [(s, k) for s in M.GPU_SCENES for k in KINDS]


@pytest.fixture(scope="module")
def contexts(gpu):
    """One context per (scene, kind), kept for the module and closed at its end.  The contexts run no
    scene kernel (jit 0): a probe module is compiled from the tables a context holds, whatever it renders with."""
    held = {}

    def get(scene, kind):
        if (scene, kind) not in held:
            held[scene, kind] = G.tracer(M.scene(scene).prog, 16, 16, 2, extra={"jit": 0})
        return held[scene, kind]

    yield get
    for pt in held.values():
        pt.close()


def differing(got, want):
    return np.nonzero(~G.same_or_nan(np.asarray(got, F), np.asarray(want, F)))[0]


def describe_point(name, i, pts, masks, pf, mf):
    return (f"{name}: input {i} point {pts[i].tolist()} ({M.POINT_FAMILIES[pf[i]]}) mask "
            f"{int(masks[i, 0]):#x}:{int(masks[i, 1]):#x} ({M.MASK_FAMILIES[mf[i]]})")


def assert_map(name, what, sc, got_d, got_shape, want_d, want_node, pts, masks, pf, mf):
    bad = differing(got_d, want_d)
    assert not len(bad), (f"{what}: {len(bad)} of {len(pts)} distances differ; first "
                          f"{describe_point(name, bad[0], pts, masks, pf, mf)}: got {got_d[bad[0]]!r} want {want_d[bad[0]]!r}")
    ga, wa = M.albedo_of_shapes(sc, got_shape), M.albedo_of_nodes(sc, want_node)
    bad = np.nonzero((ga != wa).any(1))[0]
    assert not len(bad), (f"{what}: {len(bad)} shapes differ; first {describe_point(name, bad[0], pts, masks, pf, mf)}: "
                          f"got shape {got_shape[bad[0]]} want node {want_node[bad[0]]}")


# ---- JitMap -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", CASES)
def test_map_matches_the_oracle(contexts, name, kind):
    """Every point family under every mask family, wave-homogeneous (grouped) and with every wave mixed
    (interleaved), with and without the wave's check[] union, n = 64 k + 37, 1 and 0."""
    pt, sc = contexts(name, kind), M.scene(name)
    pts, masks, pf, mf = M.map_inputs(name)
    want_d, want_node = M.map_expected(name)
    order = M.interleave(len(pts))
    per_input = {}
    for union_mode in (0, 1):
        for label, idx in (("grouped", np.arange(len(pts))), ("interleaved", order)):
            d, shape, _ = pt.probe_map(kind, pts[idx], check=masks[idx], union_mode=union_mode)
            what = f"{name} {kind} JitMap union_mode {union_mode} {label}"
            assert_map(name, what, sc, d, shape, want_d[idx], want_node[idx], pts[idx], masks[idx], pf[idx], mf[idx])
            back = np.empty_like(d)
            back[idx] = d
            per_input[union_mode, label] = back
    first = per_input[0, "grouped"]
    assert all(G.same_or_nan(first, v).all() for v in per_input.values())  # the orders agree per input
    # a NULL check[] is every bit set; one point; none
    ones = mf == 0
    d, shape, _ = pt.probe_map(kind, pts[ones])
    assert not len(differing(d, want_d[ones])), f"{name} {kind}: NULL check[]"
    d, shape, _ = pt.probe_map(kind, pts[13:14], check=masks[13:14], union_mode=1)
    assert not len(differing(d, want_d[13:14])), f"{name} {kind}: n = 1"
    d, shape, live = pt.probe_map(kind, pts[:0], check=masks[:0])
    assert d.shape == (0,) and shape.shape == (0,) and live.shape == (0,)


# ---- the shade pass's taps ------------------------------------------------------------------
TAP_CASES = [(s, k) for s in M.GPU_SCENES if s not in ("nan-sphere", "inf-sphere") for k in KINDS]


@pytest.mark.parametrize("name,kind", TAP_CASES)
def test_taps_match_the_oracle(contexts, name, kind):
    """The six taps of every hit under the four bounds: +inf, NaN (rule off), the pipeline's own tap_bound
    and the tightest (the maximum of the oracle's six tap values); d6 and shapes equal the oracle's at the
    six tap points; and JitMapB1 handed JitMapB0's live mask through pt_probe_map returns them too.  The
    live mask after the first tap names only shapes whose check[] bit the lane has; under +inf and NaN,
    where no bound excludes a shape, it names every one of them, and JitMapB0 alone returns the same mask.
    The interpreter's taps are six plain evaluations and leave live alone."""
    pt, sc, H = contexts(name, kind), M.scene(name), M.hit_inputs(name)
    n = len(H["hits"])
    assert n >= 16
    admitted = sc.expected_live(H["masks"]) if kind in GENERATED else np.zeros(n, np.uint64)
    if not np.isnan(sc.bound_k):
        assert F(pt.get_option("bound_k")) == sc.bound_k  # the pipeline bound is the pipeline's
    else:
        assert np.isnan(pt.get_option("bound_k"))
    want_albedo = M.albedo_of_nodes(sc, H["node6"].reshape(-1))
    order = M.interleave(n, seed=11)
    for family in M.BOUND_FAMILIES:
        bnd = H["bounds"][family]
        for label, idx in (("grouped", np.arange(n)), ("interleaved", order)):
            d6, shape6, live = pt.probe_taps(kind, H["hits"][idx], check=H["masks"][idx], bnd=bnd[idx])
            bad = differing(d6.reshape(-1), H["d6"][idx].reshape(-1))
            assert not len(bad), (f"{name} {kind} taps, bound {family} {label}: {len(bad)} tap values differ; first hit "
                                  f"{H['hits'][idx][bad[0] // 6].tolist()} tap {bad[0] % 6} bound {bnd[idx][bad[0] // 6]!r} "
                                  f"mask {int(H['masks'][idx][bad[0] // 6, 0]):#x}: got {d6.reshape(-1)[bad[0]]!r} want "
                                  f"{H['d6'][idx].reshape(-1)[bad[0]]!r}")
            got_albedo = M.albedo_of_shapes(sc, shape6.reshape(-1))
            assert np.array_equal(got_albedo.reshape(n, 6, 3), want_albedo.reshape(n, 6, 3)[idx]), \
                f"{name} {kind} taps, bound {family} {label}: shapes"
            stray = np.nonzero(live & ~admitted[idx])[0]
            assert not len(stray), (f"{name} {kind} taps, bound {family} {label}: live {int(live[stray[0]]):#x} names a shape "
                                    f"outside check[] {int(H['masks'][idx][stray[0], 0]):#x} (admitted "
                                    f"{int(admitted[idx][stray[0]]):#x}) at hit {H['hits'][idx][stray[0]].tolist()}")
            if family in ("inf", "nan"):
                assert np.array_equal(live, admitted[idx]), f"{name} {kind} taps, bound {family} {label}: live"
            back = np.empty_like(live)
            back[idx] = live
            taps_live = back  # (per hit, whichever order ran last: both were checked)
        # B0 at the first tap point, then B1 with its live mask at the other five
        taps = H["taps"]
        d0, s0, live0 = pt.probe_map(kind, taps[:, 0], check=H["masks"], bnd=bnd, variant="b0")
        assert not len(differing(d0, H["d6"][:, 0])), f"{name} {kind} JitMapB0, bound {family}"
        assert not (live0 & ~admitted).any(), f"{name} {kind} JitMapB0, bound {family}: live outside check[]"
        if family in ("inf", "nan"):  # (a finite bound is widened about the hit in the taps, about the tap point here)
            assert np.array_equal(live0, taps_live), f"{name} {kind} JitMapB0's live is not the taps', bound {family}"
        for k in range(1, 6):
            dk, sk, _ = pt.probe_map(kind, taps[:, k], check=H["masks"], bnd=bnd, live_in=live0, variant="b1")
            bad = differing(dk, H["d6"][:, k])
            assert not len(bad), (f"{name} {kind} JitMapB1 tap {k}, bound {family}: {len(bad)} differ; first hit "
                                  f"{H['hits'][bad[0]].tolist()} live {int(live0[bad[0]]):#x}: got {dk[bad[0]]!r} want "
                                  f"{H['d6'][bad[0], k]!r}")
            assert np.array_equal(M.albedo_of_shapes(sc, sk), M.albedo_of_nodes(sc, H["node6"][:, k]))
    # one hit; none
    d6, shape6, live = pt.probe_taps(kind, H["hits"][5:6], check=H["masks"][5:6], bnd=H["bounds"]["tightest"][5:6])
    assert not len(differing(d6.reshape(-1), H["d6"][5])), f"{name} {kind} taps: n = 1"
    d6, shape6, live = pt.probe_taps(kind, H["hits"][:0], check=H["masks"][:0])
    assert d6.shape == (0, 6) and shape6.shape == (0, 6) and live.shape == (0,)


# ---- bounds() -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", CASES)
def test_bounds_match_the_oracle(contexts, name, kind):
    """Every ray family, grouped and interleaved (waves that mix guarded and unguarded lanes), and the
    first pass's wave-level box skip: the mask is still the oracle's, and a skip bit is set only for a
    box every ray of its wave misses."""
    pt, sc = contexts(name, kind), M.scene(name)
    ro, rd, fam, names = M.ray_inputs(name)
    want = sc.bounds(ro, rd)
    for label, idx in (("grouped", np.arange(len(ro))), ("interleaved", M.interleave(len(ro), seed=13))):
        mask, _ = pt.probe_bounds(kind, ro[idx], rd[idx])
        bad = np.nonzero((mask != want[idx]).any(1))[0]
        assert not len(bad), (f"{name} {kind} bounds() {label}: {len(bad)} of {len(ro)} masks differ; first ray "
                              f"{ro[idx][bad[0]].tolist()} -> {rd[idx][bad[0]].tolist()} ({names[fam[idx][bad[0]]]}): got "
                              f"{[hex(int(v)) for v in mask[bad[0]]]} want {[hex(int(v)) for v in want[idx][bad[0]]]}")
    sro, srd = M.skip_rays(name)
    swant = sc.bounds(sro, srd)
    mask, skip = pt.probe_bounds(kind, sro, srd, skip_mode=1)
    bad = np.nonzero((mask != swant).any(1))[0]
    assert not len(bad), f"{name} {kind} bounds() after the box skip: first ray {sro[bad[0]].tolist()} -> {srd[bad[0]].tolist()}"
    assert skip[-1] == 0  # the ragged wave skips nothing
    backs = [a["back"] for a in sc.prog.aabb_dicts()]
    for w, word in enumerate(skip.tolist()):
        for k in range(min(64, len(backs))):
            if (word >> k) & 1 and backs.count(backs[k]) == 1:
                hit = (swant[64 * w:64 * w + 64, backs[k] >> 6] >> np.uint64(backs[k] & 63)) & np.uint64(1)
                assert not hit.any(), f"{name} {kind}: wave {w} skips box {k}, which {int(hit.sum())} of its rays hit"
    m1, _ = pt.probe_bounds(kind, ro[:1], rd[:1])
    assert np.array_equal(m1, want[:1])
    m0, s0 = pt.probe_bounds(kind, ro[:0], rd[:0])
    assert m0.shape == (0, 2) and s0.shape == (0,)


# ---- value edits without a recompile (C3) -----------------------------------------------------
EDIT_LABELS = ("position x to 1e20", "position y to NaN", "cube size y to -0.1", "sphere radius to -0.2")


def test_value_edits_reuse_the_table_module_and_match_the_oracle(gpu):
    """fuzzref.EDITS on C3 -- a position to 1e20, one to NaN, a cube size to -0.1 (its union's rule goes
    off), a radius to -0.2 -- and each inverse: after pt_set_data the table kind answers as the oracle
    with no new compile, the baked kind after its rebuild."""
    ed = scenes.SCENES["c3"]()
    comp = CompData()
    prog = ed.compile(comp)
    pt = G.tracer(prog, 16, 16, 2, extra={"jit": 0})
    pts, masks, pf, mf = M.map_inputs("c3")
    keep = np.arange(0, len(pts), 3)  # (a third of the inputs per step: twelve steps)
    pts, masks, pf, mf = pts[keep], masks[keep], pf[keep], mf[keep]
    ro, rd, _, _ = M.ray_inputs("c3")
    pt.probe_map("table", pts, check=masks, union_mode=1)
    pt.probe_bounds("table", ro, rd)
    compiles = pt.get_option("probe_compiles")
    assert compiles == 2 and pt.get_option("probe_seconds") > 0.0
    wanted = [e for e in fuzzref.EDITS if any(lbl in e[0] for lbl in EDIT_LABELS)]
    assert len(wanted) == 4
    steps = fuzzref.edit_steps(wanted)
    assert len(steps) == 8
    baked_seen = set()
    for label, run, changes_source, _, _ in steps:
        assert not changes_source
        run(ed)
        ed.data_update(comp)
        data = comp.data_array.as_array()
        pt.set_data(data)
        sc = M.Scene(ed)  # the oracle of the edited tree
        want_d, want_node = sc.map(pts, masks)
        wantb = sc.bounds(ro, rd)
        for kind in ("table", "baked"):
            d, shape, _ = pt.probe_map(kind, pts, check=masks, union_mode=1)
            assert_map("c3", f"c3 {kind} after '{label}'", sc, d, shape, want_d, want_node, pts, masks, pf, mf)
            mask, _ = pt.probe_bounds(kind, ro, rd)
            assert np.array_equal(mask, wantb), f"c3 {kind} bounds() after '{label}'"
        if data.tobytes() not in baked_seen:  # the baked kind's two modules, once per distinct set of values
            baked_seen.add(data.tobytes())
            compiles += 2
        assert pt.get_option("probe_compiles") == compiles, label  # the table modules served every step
    pt.close()


# ---- census: the inputs reach what they are meant to reach ------------------------------------
@pytest.mark.parametrize("name", M.GPU_SCENES)
def test_census_of_the_launch_counters(contexts, name):
    """Conditions on the inputs, from the instrumented builds of the same code (whose values equal the
    oracle's too), on every scene, each where the scene's own generated code has the feature: JitMap with
    a cull target whose rule is on drops shapes and evaluates others; the taps under a finite bound drop
    shapes, and live is neither all set nor all clear across hits, where JitMapB0 records live bits; a
    wave returns a non-zero skip word where primary_box_skip serves the scene; a bounds() wave reaches the
    exact fallback on the corner and edge rays where the scene has a box to aim at."""
    pt, sc = contexts(name, "table"), M.scene(name)
    pts, masks, pf, mf = M.map_inputs(name)
    want_d, _ = M.map_expected(name)
    d, _, _, st = pt.probe_map("table", pts, check=masks, union_mode=1, counters=True)
    assert not len(differing(d, want_d))
    print(name, "JitMap", {k: st[k] for k in ("culled", "wave_evals", "wave_shapes", "wave_maps")})
    assert st["wave_maps"] == (len(pts) + 63) // 64
    if sc.generated["cull_unions"]:
        assert st["culled"] > 0 and st["wave_evals"] > 0 and st["wave_shapes"] > st["wave_evals"], st
    H = M.hit_inputs(name)
    if len(H["hits"]):
        family = "pipeline" if not np.isnan(sc.bound_k) else "tightest"
        d6, _, live, stt = pt.probe_taps("table", H["hits"], check=H["masks"], bnd=H["bounds"][family], counters=True)
        assert not len(differing(d6.reshape(-1), H["d6"].reshape(-1)))
        admitted = sc.expected_live(H["masks"])
        print(name, "taps", {k: stt[k] for k in ("culled", "wave_evals", "normal_maps")}, "live bits",
              len(sc.generated["live"]), "distinct", len(set(live.tolist())), "all admitted", int((live == admitted).sum()),
              "none", int((live == 0).sum()), "of", len(live))
        assert stt["normal_maps"] >= 6 * len(H["hits"]), stt
        if sc.generated["live"]:  # (JitMapB0 has bound-rule tests)
            assert stt["culled"] > 0, stt
            assert not (live & ~admitted).any()
            assert (live != admitted).any() and (live != 0).any() and len(set(live.tolist())) > 1
    ro, rd, fam, _ = M.ray_inputs(name)
    corner = fam == 1
    if corner.any():
        mask, _, stb = pt.probe_bounds("table", ro[corner], rd[corner], counters=True)
        assert np.array_equal(mask, sc.bounds(ro[corner], rd[corner]))
        print(name, "bounds", {k: stb[k] for k in ("bounds_waves", "bounds_exact", "segments", "aabb_tests")})
        assert stb["segments"] == int(corner.sum()) and stb["aabb_tests"] == int(corner.sum()) * sc.prog.n_aabb
        if pt.get_option("fast_bounds"):  # (farbox: every wave takes the IEEE loop, none the slab tests)
            assert stb["bounds_waves"] > 0 and stb["bounds_exact"] > 0, stb
    sro, srd = M.skip_rays(name)
    _, skip = pt.probe_bounds("table", sro, srd, skip_mode=1)
    print(name, "skip words", [hex(int(w)) for w in skip])
    if pt.get_option("fast_bounds") and 0 < sc.prog.n_aabb <= 64:
        assert skip.any(), f"{name}: no wave skipped a box"
    else:  # (primary_box_skip serves scenes of 1 to 64 boxes that pass the slab tests' guards)
        assert not skip.any()


# ---- the entry points' refusals ---------------------------------------------------------------
def test_probe_refusals(gpu):
    import ctypes

    pts = np.zeros((3, 3), F)
    mask = np.zeros((3, 4), np.uint32)
    empty = G.tracer(None, 16, 16, 2)
    L, c = empty._L, empty._ctx
    assert L.pt_probe_map(c, 0, 0, 3, N.fptr(pts), None, None, None, 0, None, None, None, None) == N.PT_ERR_STATE
    assert L.pt_probe_taps(c, 1, 3, N.fptr(pts), None, None, None, None, None, None) == N.PT_ERR_STATE
    assert L.pt_probe_bounds(c, 2, 3, N.fptr(pts), N.fptr(pts), 0, N.ptr(mask, ctypes.c_uint32), None, None) == N.PT_ERR_STATE
    empty.close()
    pt = G.tracer("c2", 16, 16, 2, extra={"jit": 0})
    L, c = pt._L, pt._ctx
    assert L.pt_probe_map(c, 0, 0, 3, None, None, None, None, 0, None, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_map(c, 3, 0, 3, N.fptr(pts), None, None, None, 0, None, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_map(c, 0, 3, 3, N.fptr(pts), None, None, None, 0, None, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_map(c, 0, 0, 3, N.fptr(pts), None, None, None, 2, None, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_taps(c, 1, 3, None, None, None, None, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_bounds(c, 1, 3, N.fptr(pts), None, 0, N.ptr(mask, ctypes.c_uint32), None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_bounds(c, 1, 3, N.fptr(pts), N.fptr(pts), 0, None, None, None) == N.PT_ERR_INVALID
    assert L.pt_probe_map(c, 0, 0, 0, None, None, None, None, 0, None, None, None, None) == N.PT_OK
    assert L.pt_probe_map(c, 1, 0, 3, N.fptr(pts), None, None, None, 0, None, None, None, None) == N.PT_OK  # no output asked
    assert pt.get_option("probe_compiles") == 1
    pt.close()
