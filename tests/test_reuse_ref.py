"""The walks of reuseref.py, host side: before a GPU sees them, every
transition a walk claims is in its steps (computed from the step data, not
the labels), every expected image is lit and differs from the one before, the
oracle's continuation of its own image is consistent, and each seeded order
is a permutation that keeps the groups whole.  No GPU."""
import collections

import numpy as np
import pytest

import gpuharness as G
import reuseref as R

CASES = [(name, v) for name in ("PIPELINE", "GENERIC") for v in R.VARIANTS[name]]
ORDERS = [None, *R.SEEDS]


def test_scene_classes():
    """How each scene of the walks is binned, from its n_check against PT_BIN_BITS and 64."""
    assert R.BIN_BITS == R.header_bin_bits()
    n = {s: R.n_check(s) for s in ("c1", "c2", "c3", "c3_noaabb", "cull", "wide")}
    assert n["c1"] <= n["c2"] <= R.BIN_BITS  # the set is the bin index
    assert R.BIN_BITS < n["c3"] == n["c3_noaabb"] <= 64 and R.program("c3").n_aabb == 24  # the table of sets
    assert R.program("c3_noaabb").n_aabb == 0  # no box: every mask empty
    assert n["cull"] == 64  # the last size the table takes
    assert 64 < n["wide"] <= 128  # hash bins, the wide masks
    assert [R.scene_class(s) for s in ("c1", "c2", "c3", "c3_noaabb", "cull", "wide")] == \
        ["index", "index", "table", "table", "table", "wide"]
    assert R.BYTES_PER_SAMPLE == 168 and R.BYTES_WIDE == 24


def test_walk_sizes():
    for name, variant in CASES:
        steps = R.walk(name, None, variant)
        assert len(steps) <= 44, (name, variant, len(steps))
        assert all(s.w * s.h <= 72 * 40 or (s.w, s.h) == (64, 48) for s in steps)
        assert all(1 <= s.spp <= 5 for s in steps)
        assert all(s.variant == variant for s in steps)
        labels = [s.label for s in steps]
        assert len(set(labels)) == len(labels)
        # the cleared steps' images are all determined differently, so in any order neighbours differ
        keys = [R.render_key(s) for s in steps if s.clear]
        assert len(set(keys)) == len(keys), [k for k, c in collections.Counter(keys).items() if c > 1]
    assert len(R.walk("PIPELINE", None, "binned_tier")) == R.TIER_STEPS
    # the tier's five steps cut no group and are the end of the scene-kernel walk
    assert R.walk("PIPELINE", None, "binned_tier")[0].group is None
    assert [s.label for s in R.walk("PIPELINE", None, "binned_tier")] == \
        [s.label for s in R.walk("PIPELINE", None, "binned_jit")][-R.TIER_STEPS:]
    # the scene-kernel variants keep to the scenes whose kernels the build ships
    from compute_path_tracer_amd import build
    for v in R.SCENEK + ("jit",):
        name = "GENERIC" if v == "jit" else "PIPELINE"
        assert {s.scene for s in R.walk(name, None, v)} <= {"c1", "c2", "c3"} <= set(build.JIT_CACHE_SCENES)


@pytest.mark.parametrize("name,variant", CASES)
def test_transitions_present(name, variant):
    steps = R.walk(name, None, variant)
    got = R.transitions(steps, variant)
    claims = set(R.TIER_CLAIMS if variant == "binned_tier" else R.CLAIMS[name])
    assert claims <= got, sorted(claims - got)
    assert claims <= {s.label[0] for s in steps}  # (and the labels say so)
    if variant in ("binned", "simple"):
        assert R.has_moments_group(steps)
    if variant == "binned_tier":
        assert any(R.scene_class(a.scene) == "index" and R.scene_class(b.scene) == "table"
                   for a, b in zip(steps, steps[1:]))


def test_pipeline_model_along_the_walk():
    """What the binned steps ask of the buffers, from the model alone."""
    steps = R.walk("PIPELINE", None, "binned")
    m = R.BinModel()
    last, saw_wide, back_from_wide, grew_passes = 0, False, False, False
    for prev, s in zip([None] + steps, steps):
        if not R.binned(s):
            continue
        p = R.plan(s)
        # the issue's launch count: every chunk of these steps uses the same lanes
        assert p.trace_launches == p.lanes_used * (s.bounces + 1) * p.chunks, s.label
        passes_before = m.passes
        if m.launch(s) and passes_before and p.passes > passes_before and s.bounces == 32:
            grew_passes = True
        assert m.bin_bytes >= last
        last = m.bin_bytes
        if prev is not None and R.scene_class(prev.scene) == "wide" and R.scene_class(s.scene) != "wide":
            back_from_wide = back_from_wide or m.wide
        saw_wide = saw_wide or m.wide
        if s.label.startswith("d: bin_samples 64"):
            assert p.chunks == s.spp and s.samples < p.n_pix
        if s.label.startswith("d: bin_samples 1 << 20"):
            assert p.chunks == 1
        if s.label.startswith("c: 4 lanes"):
            assert p.lanes_used == s.spp == 2 < s.lanes
    assert saw_wide and back_from_wide and grew_passes
    assert m.cap == 72 * 40 * 3 and m.n_lanes == 3


@pytest.mark.parametrize("name,variant", [("PIPELINE", "binned"), ("PIPELINE", "binned_jit"), ("GENERIC", "simple")])
def test_expected_images(name, variant):
    """Lit (the no-tile step is all zero bits; a debug view differs from the
    same step at debug 0), and at least 4 pixels away from the step before, in
    every order."""
    import dataclasses

    for seed in ORDERS:
        steps = R.walk(name, seed, variant)
        images = R.expected_images(steps)
        for k, (s, img) in enumerate(zip(steps, images)):
            assert img.shape == (s.h, s.w, 4)
            if R.n_tiles(s) == 0:
                assert not G.bits(img).any(), s.label
            elif s.debug:
                plain = R.expected(dataclasses.replace(s, debug=0))
                assert G.pixels_changed(img, plain) >= 4, s.label
            else:
                assert img[..., :3].mean() > 0, s.label
            if k and images[k - 1].shape == img.shape:
                assert G.pixels_changed(img, images[k - 1]) >= 4, (steps[k - 1].label, s.label)


def test_oracle_continuation_is_consistent():
    """2 + 3 + 2 spp continued equals 7 spp at once, bit for bit; the tiles of three ranks sum to the full image."""
    S = R.Step
    a = R.expected(S("2", bounces=4))
    b = R.expected(S("+3", bounces=4, spp=3, clear=False), a)
    c = R.expected(S("+2", bounces=4, clear=False), b)
    assert R.frames_done(c) == 7
    whole = G.oracle_image("c3", 40, 24, 7, 4)
    assert G.first_difference(c, whole) is None
    assert G.pixels_changed(a, b) >= 4 and G.pixels_changed(b, c) >= 4
    full = R.expected(S("full"))
    parts = [R.expected(S("part", tiles=(r, 3))) for r in range(3)]
    owned = [(G.bits(p) != 0).any(-1) for p in parts]
    assert (np.sum(owned, axis=0) <= 1).all()  # no texel twice
    assert G.first_difference(parts[0] + parts[1] + parts[2], full) is None
    # the walks' accumulating group, part by part, is the oracle going on from its own image
    steps = [s for s in R.walk("PIPELINE", None, "binned") if s.group == "acc"]
    images = R.expected_images(steps)
    total = sum(s.spp for s in steps)
    assert G.first_difference(images[-1], G.oracle_image("c3", steps[0].w, steps[0].h, total, steps[0].bounces)) is None


@pytest.mark.parametrize("name,variant", CASES)
def test_permutations(name, variant):
    scripted = R.walk(name, None, variant)
    orders = [[s.label for s in scripted]]
    for seed in R.SEEDS:
        steps = R.walk(name, seed, variant)
        assert collections.Counter(steps) == collections.Counter(scripted)
        assert steps == R.walk(name, seed, variant)  # the seed fixes the order
        # groups intact: the same units, each in its scripted order
        key = lambda u: tuple(s.label for s in u)  # noqa: E731
        assert sorted(map(key, R.units(steps))) == sorted(map(key, R.units(scripted)))
        for u in R.units(steps):
            assert u[0].clear and all(not s.clear for s in u[1:])
        orders.append([s.label for s in steps])
    assert len({tuple(o) for o in orders}) == 3, "the two seeds and the scripted order must differ"
