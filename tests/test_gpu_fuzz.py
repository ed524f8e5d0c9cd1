"""GPU: random editor trees (scenes.fuzz_scene), programs at pt_set_program's
limits and live edits on one long-lived context, through the kernel variants,
bit for bit against the CPU oracle (a NaN equal only to a NaN in the same
place).  test_scene_fuzz.py checks, without a GPU, that the corpus is lit and
varied and that the edit sequence is visible at every step."""
import time

import numpy as np
import pytest

import camref
import fuzzref as R
import gpuharness as G
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.sdf_editor import CompData
from gpuharness import INTERPRETERS, KERNELS, SCENE_KERNELS

pytestmark = pytest.mark.gpu

# test_work_counters_match_oracle's keys, and the torus the random scenes add
COUNTERS = ("samples", "segments", "march_steps", "normal_maps", "shaded", "aabb_tests", "xform_union", "xform_shape",
            "sdf_sphere", "sdf_cube", "sdf_torus", "sdf_octahedron", "comb_union", "comb_sub", "comb_assign", "rr_break")


def _image(pt, w, h, spp):
    pt.dispatch(G.constants(w, h), spp)
    return pt.read_image()


@pytest.mark.parametrize("kernel", INTERPRETERS)
def test_corpus_on_interpreter_kernels(gpu, kernel):
    """Every FUZZ_SEEDS scene, 24x16, 2 spp, 4 bounces; on every fourth seed
    the work counters of the same context against the oracle's."""
    for k, seed in enumerate(scenes.FUZZ_SEEDS):
        ed = scenes.fuzz_scene(seed)
        pt = G.tracer(ed.compile(CompData()), R.W, R.H, R.BOUNCES, kernel)
        img = _image(pt, R.W, R.H, R.SPP)
        diff = R.first_difference(img, R.fuzz_oracle(seed))
        assert diff is None, f"seed {seed} on {kernel}: {diff}"
        if k % 4 == 0:
            got = pt.stats(G.constants(R.W, R.H), R.SPP)
            _, want = R.oracle_image(ed, R.W, R.H, R.SPP, R.BOUNCES, counters=True)
            bad = {c: (got[c], want[c]) for c in COUNTERS if got[c] != want[c]}
            assert not bad, f"seed {seed} on {kernel}: counters (got, oracle) {bad}"
        pt.close()


@pytest.mark.parametrize("kernel", SCENE_KERNELS)
@pytest.mark.parametrize("seed,profile", scenes.FUZZ_JIT_SEEDS)
def test_small_scenes_on_scene_kernels(gpu, seed, profile, kernel):
    """Every FUZZ_JIT_SEEDS scene on its own generated kernels (shipped in
    lib/jitcache by build(); compiled here on a miss), the binned ones with
    one and two pipelines; the deep chain also at 0 bounces."""
    prog = scenes.SCENES[f"fuzz-{seed}"]().compile(CompData())
    for bounces in (R.BOUNCES, 0) if profile == "deep" else (R.BOUNCES,):
        want = R.fuzz_oracle(seed, profile, R.W, R.H, R.SPP, bounces)
        for lanes in (1, 2) if kernel.startswith("binned") else (None,):
            pt = G.tracer(prog, R.W, R.H, bounces, kernel, extra={"bin_lanes": lanes} if lanes else None)
            diff = R.first_difference(_image(pt, R.W, R.H, R.SPP), want)
            pt.close()
            assert diff is None, f"fuzz-{seed} on {kernel}, bin_lanes {lanes}, {bounces} bounces: {diff}"


ALL = INTERPRETERS + SCENE_KERNELS


@pytest.mark.parametrize("kernel", ALL)
@pytest.mark.parametrize("name", ["nan-position", "nan-rotation", "nan-union-rotation"])
def test_nan_in_a_transform(gpu, name, kernel):
    """scenes.nan_cube: a NaN position, a NaN rotation about x, or a NaN
    rotation about z of the union above a cube with no rotation, makes every
    coordinate of the cube NaN in the reference (full rotation matrices); the
    kernels skip the matrices' zero terms and must get there all the same."""
    ed = scenes.SCENES[name]()
    want = R.oracle_image(ed, R.W, R.H, R.SPP, R.BOUNCES)
    assert want[..., :3].mean() > 0
    pt = G.tracer(ed.compile(CompData()), R.W, R.H, R.BOUNCES, kernel)
    diff = R.first_difference(_image(pt, R.W, R.H, R.SPP), want)
    pt.close()
    assert diff is None, f"{name} on {kernel}: {diff}"


_sky_refs = {}


@pytest.mark.parametrize("kernel", ["binned", "binned_tier"])
@pytest.mark.parametrize("seed", [154, 15793])
def test_posed_camera_and_sky(gpu, seed, kernel):
    """The camera and sky tests' lens camera and sky."""
    w, h, spp, bounces = 12, 8, 1, 3
    ed = scenes.SCENES[f"fuzz-{seed}"]()
    if seed not in _sky_refs:
        _sky_refs[seed] = camref.render(ed.rows(), w, h, 1, 1, G.aspect(w, h), bounces, spp, camera=G.camera("lens"),
                                        sky=G.sky())
    pt = G.tracer(ed.compile(CompData()), w, h, bounces, kernel)
    pt.look_at(G.EYE, G.TARGET, **G.LOOK["lens"])
    pt.set_sky(**G.SKY)
    diff = R.first_difference(_image(pt, w, h, spp), _sky_refs[seed])
    pt.close()
    assert diff is None, f"fuzz-{seed} on {kernel}: {diff}"


def _refused_then_serves(kernel, bad, good, w, h, spp, bounces):
    """pt_set_program refuses `bad` on the host (PT_ERR_UNSUPPORTED, nothing
    launched); the same context then takes `good` and renders it exactly."""
    pt = G.tracer(None, w, h, bounces, kernel)
    with pytest.raises(N.NativeError) as e:
        pt.remake_pipeline(bad.compile(CompData()))
    assert e.value.code == N.PT_ERR_UNSUPPORTED
    prog = good.compile(CompData())
    pt.remake_pipeline(prog)
    pt.set_data(prog.data)
    diff = R.first_difference(_image(pt, w, h, spp), R.oracle_image(good, w, h, spp, bounces))
    pt.close()
    assert diff is None, diff


@pytest.mark.parametrize("kernel", ["binned", "simple"])
def test_check_limit(gpu, kernel):
    """128 check[] entries (PT_MAX_CHECK) render; 129 are refused."""
    w, h, spp, bounces = 16, 8, 1, 3
    full = R.boxed_scene(128)
    prog = full.compile(CompData())
    assert prog.n_check == prog.n_aabb == 128
    want = R.oracle_image(full, w, h, spp, bounces)
    assert want[..., :3].mean() > 0
    pt = G.tracer(prog, w, h, bounces, kernel)
    diff = R.first_difference(_image(pt, w, h, spp), want)
    pt.close()
    assert diff is None, diff
    over = R.boxed_scene(129)
    assert over.compile(CompData()).n_check == 129
    _refused_then_serves(kernel, over, full, w, h, spp, bounces)


@pytest.mark.parametrize("kernel", ["binned", "simple"])
def test_depth_limit(gpu, kernel):
    """Unions nested 8 deep (PT_MAX_DEPTH) render; 9 deep are refused."""
    seed, profile = scenes.FUZZ_JIT_SEEDS[-1]
    assert profile == "deep"
    deep = scenes.fuzz_scene(seed, profile)
    pt = G.tracer(deep.compile(CompData()), R.W, R.H, R.BOUNCES, kernel)
    diff = R.first_difference(_image(pt, R.W, R.H, R.SPP), R.fuzz_oracle(seed, profile))
    pt.close()
    assert diff is None, diff
    eight = R.chain_scene(8)
    assert R.oracle_image(eight, 16, 8, 1, 3)[..., :3].mean() > 0
    _refused_then_serves(kernel, R.chain_scene(9), eight, 16, 8, 1, 3)


def _derived(pt):
    """(fast_bounds, bound_k is finite): what pt_set_data derived from the values."""
    return pt.get_option("fast_bounds") == 1.0, bool(np.isfinite(pt.get_option("bound_k")))


EDIT_KERNELS = ["simple", "wave", "binned", "jit", "binned_jit", "binned_jit_trace_taps"]


@pytest.mark.parametrize("kernel", EDIT_KERNELS)
def test_live_edits_on_one_context(gpu, kernel):
    """One C3 context through the whole edit sequence of fuzzref.EDITS
    (data_update, set_data, clear, dispatch at 32x20, 2 spp, 4 bounces), each
    image against a fresh oracle of the edited tree, and the derived state
    (fast_bounds, bound_k) against what the step is named for.  C3 has no
    shape with a scale other than 1, so on every kernel one leaves 1 first (a
    new source: one compile per process on the scene kernels, timed), then
    goes to 1e-7 and back.  The interpreter kernels also take a union's scale
    to 1e-7; binned_jit ends with the two edits that change its source."""
    edits = R.EDITS + R.EDITS_SCALE + (R.EDITS_INTERPRETER if kernel in INTERPRETERS else []) + \
        (R.EDITS_SOURCE if kernel == "binned_jit" else [])
    w, h, spp, bounces = R.EW, R.EH, R.ESPP, R.EBOUNCES
    opts = KERNELS[kernel]
    ed = scenes.c3_graph32()
    cd = CompData()
    pt = G.tracer(ed.compile(cd), w, h, bounces, kernel)
    images = [R.oracle_image(ed, w, h, spp, bounces)]
    diff = R.first_difference(_image(pt, w, h, spp), images[0])
    assert diff is None, f"before any edit: {diff}"
    assert _derived(pt) == (True, True)
    for label, run, changes_source, restores, state in R.edit_steps(edits):
        run(ed)
        ed.data_update(cd)
        t0 = time.perf_counter()
        pt.set_data(cd.data_array.as_array())
        took = time.perf_counter() - t0
        pt.clear()
        G.ready(pt, opts)
        assert _derived(pt) == state, label  # the thresholds the step is named for
        if changes_source and opts["jit"]:
            print(f"{kernel}: '{label}' changed the source: set_data took {took:.1f} s "
                  f"(jit_seconds {pt.get_option('jit_seconds'):.1f})")
        images.append(R.oracle_image(ed, w, h, spp, bounces))
        # the step is visible, from the oracle's images alone
        assert R.pixels_changed(images[-1], images[-2]) >= 4, label
        if restores:
            assert np.array_equal(images[-1].view(np.uint32), images[-3].view(np.uint32)), label
        diff = R.first_difference(_image(pt, w, h, spp), images[-1])
        assert diff is None, f"{kernel} after '{label}': {diff}"
    # what the context derived from the data, against a fresh context given the final data
    fresh = G.tracer(ed.compile(CompData()), w, h, bounces, kernel)
    assert pt.get_option("jit_active") == fresh.get_option("jit_active") == float(opts["jit"])
    assert _derived(pt) == _derived(fresh) and pt.get_option("bound_k") == fresh.get_option("bound_k")
    diff = R.first_difference(_image(fresh, w, h, spp), images[-1])
    fresh.close()
    pt.close()
    assert diff is None, f"fresh context: {diff}"
