"""GPU: one long-lived context through the walks of reuseref.py -- sizes,
bounces, lanes, chunk size, scenes, stats(), debug views, tiles, accumulation
across kernels, camera and sky, each configuration on the buffers the one
before left behind -- bit for bit against the oracle after every step, with
the binned pipeline's readings against a model of what its buffers hold.
test_reuse_ref.py shows, without a GPU, that the walks reach the transitions
they claim.  Also here, the narrow tests of what the walks found: the
check-set table's readings after a reallocation, bin_bytes after a wide scene,
and a tile with one pixel on every kernel."""
import dataclasses
import time

import pytest

import gpuharness as G
import reuseref as R

pytestmark = pytest.mark.gpu

CASES = [(name, v) for name in ("PIPELINE", "GENERIC") for v in R.VARIANTS[name]]


def _render(pt, step, carried):
    """The step's stats() run, if it has one, and its dispatch; the counters of the stats() run."""
    c = R.constants(step, R.frames_done(carried))
    counters = pt.stats(c, step.spp) if step.stats else None
    pt.dispatch(c, step.spp)
    return counters


def _check_binned_state(pt, step, model, floor, where):
    """The readings a binned step leaves, against the model of the buffers; returns bin_bytes."""
    p = R.plan(step)
    opts = G.KERNELS[step.variant]
    got = pt.get_option("bin_bytes")
    assert got == model.bin_bytes, f"{where}: bin_bytes {got}, model {model.bin_bytes} " \
                                   f"(cap {model.cap}, lanes {model.n_lanes}, wide {model.wide})"
    assert got >= floor, f"{where}: bin_bytes fell from {floor} to {got}"
    assert pt.get_option("bin_chunks") == p.chunks, where
    assert pt.get_option("trace_launches") == p.lanes_used * (step.bounces + 1) * p.chunks, where
    assert pt.get_option("shade_launches") == pt.get_option("trace_launches"), where
    assert pt.get_option("sky_launches") == (pt.get_option("trace_launches") if step.sky else 0.0), where
    # the first pass makes its own camera rays on whole tiles (scene kernels with the taps in the shade pass)
    gen_trace = 1.0 if opts["jit"] and opts.get("shade_taps", 1) and R.full_tiles(step) else 0.0
    assert pt.get_option("gen_trace") == gen_trace, where
    uses_table = step.table == 1 and R.scene_class(step.scene) == "table"
    sets = pt.get_option("bin_sets")
    # (the shade passes bin the next rays: with 0 bounces on whole tiles nothing looks a set up)
    some = step.bounces > 0 or not R.full_tiles(step)
    assert (sets > 0 if some else sets >= 0) if uses_table else (sets == -1.0), f"{where}: bin_sets {sets}"
    return got


def _run_walk(name, variant, seed):
    order = "scripted" if seed is None else f"seed {seed}"
    steps = R.walk(name, seed, variant)
    t0 = time.perf_counter()
    pt = R.open_context(steps[0])
    model, floor = R.BinModel(), 0.0
    prev = image = None
    # (a compile instead of the shipped cache, of the posed builds for instance, would show in jit_seconds)
    slowest = (pt.get_option("jit_seconds"), steps[0].label)
    for step in steps:
        where = f"{variant}, {order}: '{step.label}' after '{prev.label if prev else 'a fresh context'}'"
        if prev is not None:
            R.apply(pt, prev, step)
        carried = None if step.clear else image
        counters = _render(pt, step, carried)
        image = R.expected(step, carried)
        got = pt.read_image()
        diff = G.first_difference(got, image)
        assert diff is None, f"{where}: {diff}"
        if R.n_tiles(step) == 0:
            assert not G.bits(got).any(), where
        if counters is not None:
            want = R.expected_counters(step)
            bad = {k: (counters[k], want[k]) for k in R.COUNTERS if counters[k] != want[k]}
            assert not bad, f"{where}: counters (got, oracle) {bad}"
        if R.binned(step):
            model.launch(step)  # (a stats() run plans, and may reallocate, exactly as its dispatch does)
            floor = _check_binned_state(pt, step, model, floor, where)
            if step.stats:  # the overflow count is the stats() run's, on a table scene only
                over = pt.get_option("bin_overflow")
                table = step.table == 1 and R.scene_class(step.scene) == "table"
                assert (over >= 0.0) if table else (over == -1.0), f"{where}: bin_overflow {over}"
        elif name == "PIPELINE":
            assert pt.get_option("trace_launches") == 0.0, where
        slowest = max(slowest, (pt.get_option("jit_seconds"), step.label))
        prev = step
    walked = time.perf_counter() - t0
    # a fresh context given the final configuration: the same bits, the same number of check sets
    final = dataclasses.replace(steps[-1], label="the final configuration", clear=True, stats=False, group=None)
    R.apply(pt, prev, final)
    _render(pt, final, None)
    fresh = R.open_context(final)
    _render(fresh, final, None)
    diff = G.first_difference(fresh.read_image(), pt.read_image())
    diff_oracle = G.first_difference(pt.read_image(), R.expected(final))
    sets = (pt.get_option("bin_sets"), fresh.get_option("bin_sets")) if R.binned(final) else None
    fresh.close()
    pt.close()
    print(f"{name} on {variant}, {order}: {len(steps)} steps in {walked:.2f} s, {model.reallocs} reallocations, "
          f"{time.perf_counter() - t0:.2f} s with the fresh context; largest jit_seconds {slowest[0]:.3f} "
          f"at '{slowest[1]}'")
    assert diff_oracle is None, f"{variant}, {order}: the final configuration after '{prev.label}': {diff_oracle}"
    assert diff is None, f"{variant}, {order}: fresh context against the walked one: {diff}"
    assert sets is None or sets[0] == sets[1], f"{variant}, {order}: bin_sets (walked, fresh) {sets}"


@pytest.mark.parametrize("name,variant", CASES)
def test_walk_scripted(gpu, name, variant):
    _run_walk(name, variant, None)


@pytest.mark.parametrize("name,variant", CASES)
def test_walk_first_permutation(gpu, name, variant):
    _run_walk(name, variant, R.SEEDS[0])


@pytest.mark.parametrize("name,variant", CASES)
def test_walk_second_permutation(gpu, name, variant):
    _run_walk(name, variant, R.SEEDS[1])


def test_table_readings_after_a_reallocation(gpu):
    """bin_sets and bin_overflow read the check-set table only once a dispatch
    of the matching kind has written it: a growth of the buffers allocates a
    new table, and the overflow count then reads -1 until the next stats()."""
    pt = G.tracer("c3", 24, 16, 3, "binned")
    pt.stats(G.constants(24, 16), 2)
    assert pt.get_option("bin_overflow") >= 0.0
    assert pt.get_option("bin_sets") == -1.0  # (no timed dispatch yet)
    small = pt.get_option("bin_bytes")
    pt.update(resized=True, window=(72, 40))
    pt.dispatch(G.constants(72, 40), 2)
    assert pt.get_option("bin_bytes") > small  # a growth: everything reallocated
    assert pt.get_option("bin_overflow") == -1.0
    assert pt.get_option("bin_sets") > 0.0
    diff = G.first_difference(pt.read_image(), G.oracle_image("c3", 72, 40, 2, 3))
    assert diff is None, diff
    pt.stats(G.constants(72, 40), 2)
    assert pt.get_option("bin_overflow") >= 0.0
    assert pt.get_option("bin_sets") > 0.0
    pt.close()


@pytest.mark.parametrize("kernel", G.ALL + ["binned_jit_trace_taps"])
def test_one_pixel_tile_takes_every_frame(gpu, kernel):
    """9x9: the corner tile has one pixel inside the image.  The wave kernel's
    job pool divides by the tile's pixel count with a 32-bit multiplier, which
    a count of 1 does not have: with more than one frame it handed frames 1..
    to pixel slots that do not exist and the corner texel kept frame 0 alone
    (found by the walks' 9x17 step, on a fresh context as well)."""
    w = h = 9
    spp, bounces = 3, 3
    want = G.oracle_image("c3", w, h, spp, bounces)
    one = G.oracle_image("c3", w, h, 1, bounces)
    assert (G.bits(want[8, 8]) != G.bits(one[8, 8])).any()  # the corner texel tells three frames from one
    pt = G.tracer("c3", w, h, bounces, kernel)
    pt.dispatch(G.constants(w, h), spp)
    diff = G.first_difference(pt.read_image(), want)
    pt.close()
    assert diff is None, f"{kernel}: {diff}"


def test_bin_bytes_keeps_the_wide_buffers(gpu):
    """`wide`, then c3 on the same context: the wide buffers stay allocated,
    bin_bytes goes on counting them (it read the current scene's bytes per
    sample and fell by the wide term), a growth keeps them too, and c3 renders
    exactly beside them."""
    w, h, spp, bounces = 24, 16, 2, 3
    first = R.Step("wide", scene="wide", w=w, h=h, lanes=2, samples=1 << 20, table=1, variant="binned")
    pt = R.open_context(first)
    _render(pt, first, None)
    held = w * h * 2 * (R.BYTES_PER_SAMPLE + R.BYTES_WIDE)  # a frame per lane
    assert pt.get_option("bin_bytes") == held
    second = dataclasses.replace(first, label="c3", scene="c3")
    R.apply(pt, first, second)
    _render(pt, second, None)
    assert pt.get_option("bin_bytes") == held
    diff = G.first_difference(pt.read_image(), G.oracle_image("c3", w, h, spp, bounces))
    assert diff is None, diff
    third = dataclasses.replace(second, label="c3, 4 frames", spp=4)
    R.apply(pt, second, third)
    _render(pt, third, None)
    assert pt.get_option("bin_bytes") == 2 * held
    diff = G.first_difference(pt.read_image(), G.oracle_image("c3", w, h, 4, bounces))
    pt.close()
    assert diff is None, diff
