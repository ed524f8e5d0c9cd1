"""Random editor trees (scenes.fuzz_scene) and the live-edit sequence on C3,
host side: what the GPU tests of test_gpu_fuzz.py render must be well formed,
lit, varied, and understood by compiler, oracle and pyref alike.  No GPU."""
import math
import re

import numpy as np
import pytest

import fuzzref as R
import pyref
from compute_path_tracer_amd import _native as N, build, scenes
from compute_path_tracer_amd.sdf_editor import CompData
from test_scene_compiler import compiler_matches_oracle

MIXED = [(s, "mixed") for s in scenes.FUZZ_SEEDS]
JIT = list(scenes.FUZZ_JIT_SEEDS)


def test_seed_lists():
    assert len(set(scenes.FUZZ_SEEDS)) == len(scenes.FUZZ_SEEDS) >= 48
    assert [p for _, p in JIT] == ["mixed"] * 5 + ["deep"]
    for seed, profile in JIT:
        ed = scenes.SCENES[f"fuzz-{seed}"]()
        assert _values(ed) == _values(scenes.fuzz_scene(seed, profile))
        # small enough to compile quickly: 12 program ops, or the deep chain's 8 x (BEGIN, shape, END)
        assert ed.compile(CompData()).n_ops <= (12 if profile == "mixed" else 3 * scenes.FUZZ_DEEP_LEVELS)
        assert f"fuzz-{seed}" in build.JIT_CACHE_SCENES  # build() ships its kernels
    with pytest.raises(ValueError):
        scenes.fuzz_scene(0, "no such profile")


def _values(ed):
    return [{k: v for k, v in r.items() if k != "keys"} for r in ed.rows()]


def test_generator_is_deterministic():
    for seed, profile in MIXED[:8] + JIT:
        assert _values(scenes.fuzz_scene(seed, profile)) == _values(scenes.fuzz_scene(seed, profile))
    assert _values(scenes.fuzz_scene(1)) != _values(scenes.fuzz_scene(2))


def test_deep_profile_is_one_chain_of_eight():
    rows = scenes.fuzz_scene(2, "deep").rows()
    unions = [i for i, r in enumerate(rows) if r["kind"] == N.PT_NODE_UNION]
    assert len(unions) == scenes.FUZZ_DEEP_LEVELS == 8 and len(rows) == 16
    assert [rows[i]["parent"] for i in unions] == [-1] + unions[:-1]  # each inside the one before
    assert sorted(r["parent"] for r in rows if r["kind"] != N.PT_NODE_UNION) == unions  # a shape at every level
    ops = scenes.fuzz_scene(2, "deep").compile(CompData()).op_dicts()
    depth = best = 0
    for o in ops:
        depth += {N.PT_OP_UNION_BEGIN: 1, N.PT_OP_UNION_END: -1}.get(o["opcode"], 0)
        best = max(best, depth)
    assert best == 8


def test_product_compiler_matches_oracle_on_random_trees():
    for seed, profile in [(s, "mixed") for s in range(200)] + MIXED + JIT + [(s, "deep") for s in range(8)]:
        try:
            compiler_matches_oracle(scenes.fuzz_scene(seed, profile))
        except AssertionError as e:
            raise AssertionError(f"seed {seed} ({profile}): {e}") from e


# the five small mixed scenes and the deep chain
PYREF_SEEDS = JIT


def test_pyref_seeds_cover_what_they_should():
    have = set().union(*(R.features(scenes.fuzz_scene(s, p)) for s, p in PYREF_SEEDS))
    assert {"nesting depth >= 3", "header Subtraction", "union scale not 1"} <= have
    assert any(f.startswith("torus as") for f in have)


@pytest.mark.parametrize("seed,profile", PYREF_SEEDS)
def test_oracle_matches_pyref(seed, profile):
    """The C oracle against the exact-arithmetic Python restatement, bit for bit."""
    w, h, spp, bounces = 5, 4, 1, 3
    ed = scenes.fuzz_scene(seed, profile)
    want = pyref.render(ed.rows(), w, h, 1, 1, R.aspect(w, h), bounces, spp)
    got = R.oracle_image(ed, w, h, spp, bounces)
    assert R.first_difference(got, want) is None, R.first_difference(got, want)


@pytest.mark.parametrize("name", ["nan-position", "nan-rotation", "nan-union-rotation"])
def test_nan_transform_scenes_in_both_references(name):
    """A NaN position, rotation about x, or union rotation about z: the oracle and pyref agree bit for
    bit (full rotation matrices, 0 * NaN = NaN), the cube's distance is 0
    everywhere, and so every ray ends on the cube at once."""
    w, h, spp, bounces = 5, 4, 1, 3
    ed = scenes.SCENES[name]()
    want = pyref.render(ed.rows(), w, h, 1, 1, R.aspect(w, h), bounces, spp)
    got = R.oracle_image(ed, w, h, spp, bounces)
    assert R.first_difference(got, want) is None, R.first_difference(got, want)
    sc = pyref.Scene(ed.rows())
    with np.errstate(all="ignore"):
        d, m = sc.map([np.float32(0.3), np.float32(-0.2), np.float32(1.0)], [True] * sc.n_check)
    assert d == 0.0 and ed.rows()[m]["kind"] == N.PT_NODE_CUBE
    # so at 0 bounces every texel is the cube's emission, the octahedron in front of it included
    flat = R.oracle_image(ed, R.W, R.H, 1, 0)
    assert (flat[..., :3] > 0).all() and len(np.unique(flat.reshape(-1, 4), axis=0)) == 1


@pytest.mark.parametrize("corpus", [MIXED, JIT], ids=["FUZZ_SEEDS", "FUZZ_JIT_SEEDS"])
def test_census(corpus):
    """Every feature fuzz_scene's docstring promises occurs in each seed list
    (so a later change to the generator cannot silently shrink the corpus),
    and every scene has an emitter."""
    count = {}
    for seed, profile in corpus:
        f = R.features(scenes.fuzz_scene(seed, profile))
        assert "emitter" in f, seed
        for k in f:
            count[k] = count.get(k, 0) + 1
    print({k: count.get(k, 0) for k in sorted(R.WANTED)})
    assert not R.WANTED - set(count), sorted(R.WANTED - set(count))


def test_every_seed_renders_a_lit_image():
    """At the GPU tests' size the oracle image has a positive mean and at
    least 10 % of its pixels are not black."""
    dark = []
    for seed, profile in MIXED + JIT:
        rgb = R.fuzz_oracle(seed, profile)[..., :3]
        share = float((rgb != 0).any(-1).mean())
        if not (rgb.mean() > 0 and share >= 0.10):
            dark.append((seed, profile, float(rgb.mean()), share))
    assert not dark, dark


def test_both_sources_generate_for_every_seed():
    """test_jit_source.py's checks on every random scene: both sources
    generate, the same text for the same scene, each of the 14 kernels defined once."""
    for seed, profile in MIXED + JIT:
        for baked in (0, 1):
            src = N.scene_kernel_source(scenes.fuzz_scene(seed, profile).compile(CompData()), baked=baked)
            assert src == N.scene_kernel_source(scenes.fuzz_scene(seed, profile).compile(CompData()), baked=baked), seed
            names = re.findall(r'^extern "C" __global__ [^\n{]*?\bvoid (\w+)\(', src, re.M)
            assert len(names) == 14 and len(set(names)) == 14, (seed, names)
            for name in names:
                assert len(re.findall(r"\b%s\b" % name, src)) == 1, (seed, name)


def _steps():
    return (R.edit_steps(R.EDITS + R.EDITS_SCALE), R.edit_steps(R.EDITS + R.EDITS_SCALE + R.EDITS_INTERPRETER),
            R.edit_steps(R.EDITS + R.EDITS_SCALE + R.EDITS_SOURCE))


@pytest.mark.parametrize("steps", _steps(), ids=["all", "interpreter", "scene-kernel"])
def test_edit_sequence_cost_and_visibility(steps):
    """The live-edit sequence of test_gpu_fuzz.py on C3: a value edit leaves
    the table scene-kernel source as it was (the shipped C3 kernel keeps
    serving, no compile), the steps meant to change it do; every step changes
    at least 4 pixels of the oracle's image, and an inverse restores the
    earlier image bit for bit."""
    ed = scenes.c3_graph32()
    cd = CompData()
    prog = ed.compile(cd)
    src = N.scene_kernel_source(prog, baked=0)
    images = [R.oracle_image(ed, R.EW, R.EH, R.ESPP, R.EBOUNCES)]
    assert math.isfinite(R.union_pads(prog)[1])  # objects-a's cull rule is on
    assert R.baked_fast_bounds(prog)
    for label, run, changes_source, restores, (fast_bounds, _) in steps:
        run(ed)
        ed.data_update(cd)
        data = cd.data_array.as_array()
        assert np.array_equal(data.view(np.uint32), ed.compile(CompData()).data.view(np.uint32)), label
        # the box coordinates against bounds()' reciprocal guard, as the step's label says
        assert R.baked_fast_bounds(prog, data) == fast_bounds, label
        new = N.scene_kernel_source(prog, data=data, baked=0)
        assert (new != src) == changes_source, label
        src = new
        images.append(R.oracle_image(ed, R.EW, R.EH, R.ESPP, R.EBOUNCES))
        assert R.pixels_changed(images[-1], images[-2]) >= 4, label
        if restores:
            assert np.array_equal(images[-1].view(np.uint32), images[-3].view(np.uint32)), label
        if label.startswith("cube size y to -0.1"):
            prog_now = ed.compile(CompData())
            assert math.isnan(R.union_pads(prog_now)[1]), label  # the rule went off
        if label.startswith("the room light's light colour"):
            assert np.isnan(images[-1]).any(), label
