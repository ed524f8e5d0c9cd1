"""bench.py's algorithmic accounting, host side: the per-kernel
flop split covers the whole pipeline exactly once, and the pipeline-bytes
model adds up.  Counters from the oracle's instrumented render of a small
C3 frame (the same events the GPU's stats kernels count)."""
import numpy as np
import pytest

import bench
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.sdf_editor import CompData
from oracle import oracle as O


@pytest.fixture(scope="module")
def counters():
    ed = scenes.c3_graph32()
    prog = ed.compile(CompData())
    w, h = 48, 32
    _, ct = O.OracleScene(ed.rows()).render(w, h, O.Constants(0.0, 1, float(np.float32(w) / np.float32(h)), 1),
                                            O.Settings(0, 8, 1.0, 1.0, 0), 2, counters=True)
    return prog, ct, w * h


def _taps_share(ct: dict) -> dict:
    """A stand-in for the stats run's shade-pass tap half: every calc_normal
    map() of the oracle (the counters split it out on the GPU)."""
    taps = {k: 0 for k in ct}
    taps["normal_maps"] = ct["normal_maps"]
    return taps


@pytest.mark.parametrize("gen_trace", [True, False])
def test_flop_split_covers_the_pipeline_once(counters, gen_trace):
    prog, ct, _ = counters
    st = dict(ct, wave_maps=0, wave_shapes=0)
    taps = _taps_share(ct)
    total = bench.algorithmic_flops(st)
    trace = bench.trace_flops(st, taps, prog.n_aabb, gen_trace)
    shade = bench.shade_flops(st, taps, prog.n_aabb)
    gen = 0.0 if gen_trace else (bench.W_CAMERA + bench.W_AABB * prog.n_aabb) * st["samples"]
    fold = bench.W_ACCUM * st["samples"]
    assert trace > 0 and shade > 0
    assert trace + shade + gen + fold == pytest.approx(total, rel=0, abs=1e-3)
    # the primary rays' bounds() are never the shade pass's: one test per box
    # of each primary segment
    assert st["aabb_tests"] >= st["samples"] * prog.n_aabb
    if gen_trace:  # the first trace pass carries the camera rays and primary bounds()
        assert trace - bench.trace_flops(st, taps, prog.n_aabb, False) == pytest.approx(
            (bench.W_CAMERA + bench.W_AABB * prog.n_aabb) * st["samples"])


def test_pipeline_bytes_add_up(counters):
    _, ct, pixels = counters
    # (the oracle does not count first-segment hits; a stand-in below the samples)
    ct = dict(ct, shaded_first=ct["samples"] * 3 // 4)
    for gen_trace, gen_norec in ((True, False), (False, False), (True, True)):
        parts = bench.pipeline_bytes(ct, pixels, gen_trace=gen_trace, gen_norec=gen_norec)
        assert parts["total"] == pytest.approx(sum(v for k, v in parts.items() if k not in ("total", "trace_m", "trace_first")))
        assert parts["trace_m"] + parts["trace_first"] == pytest.approx(parts["trace"])
        assert parts["fold"] == 16.0 * ct["samples"] + 32.0 * pixels
    # no records in the first pass: 64 B per sample (trace) and per first-segment hit (shade) fewer
    rec = bench.pipeline_bytes(ct, pixels, gen_trace=True)
    norec = bench.pipeline_bytes(ct, pixels, gen_trace=True, gen_norec=True)
    assert rec["trace"] - norec["trace"] == pytest.approx(64.0 * ct["samples"])
    assert rec["shade"] - norec["shade"] == pytest.approx(64.0 * ct["shaded_first"])


def test_hw_view_and_cpu_info():
    hw = bench.hw_view({"valu_issue_frac_of_peak": 0.5, "valu_lane_utilization": 0.8, "salu_per_valu": 0.3})
    assert hw["valu_lane_slots_busy"] == pytest.approx(0.4)
    info = bench.cpu_info()
    assert info["os_cpu_count"] >= 1 and info["affinity"] >= 1 and info["model"]
    assert 1 <= bench.default_cpu_threads() <= info["affinity"]
    assert bench.default_cpu_threads() == bench.usable_cpus(info)  # every usable CPU: pthreads, not OpenMP
    assert bench.usable_cpus(dict(info, affinity=256, quota=16.0)) == 16
    assert bench.usable_cpus(dict(info, affinity=8, quota=None)) == 8


def test_resolve_world():
    """--gpus N without a launcher starts N ranks; under a launcher it must
    agree with WORLD_SIZE (a silent 1-GPU run claimed N)."""
    assert bench.resolve_world(None, {}) == (1, False)
    assert bench.resolve_world(1, {}) == (1, False)
    assert bench.resolve_world(8, {}) == (8, True)
    assert bench.resolve_world(None, {"WORLD_SIZE": "4"}) == (4, False)
    assert bench.resolve_world(4, {"WORLD_SIZE": "4"}) == (4, False)
    with pytest.raises(SystemExit):
        bench.resolve_world(8, {"WORLD_SIZE": "2"})
    with pytest.raises(SystemExit):
        bench.resolve_world(0, {})
    cmd = bench.launcher_cmd(["--gpus", "8", "--steps", "3"], 8, 29501)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd
    assert "--master-addr=127.0.0.1" in cmd and cmd[-3:] == ["--gpus", "8", "--steps", "3"][-3:]


def test_gpus_mismatch_exits_before_the_gpu():
    """A launcher's WORLD_SIZE that disagrees with --gpus ends bench.py with a
    non-zero status before it imports the library or touches a GPU."""
    import os
    import subprocess
    import sys

    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "8"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr and not any(l.startswith("{") for l in r.stdout.splitlines())


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: image.npy is the float32 image bit for bit but for its
    non-finite channels, which are 0 there and rows of nonfinite.npy (so both
    files are finite and the image can be put together again); above the
    limit a fixed sample of its texels, the same on every call, both files
    within DUMP_LIMIT."""
    import os

    img = np.random.default_rng(7).random((40, 40, 4)).astype(np.float32)
    img[3, 5] = np.nan
    img[7, 1, 2], img[7, 1, 3] = np.inf, -np.inf
    keep = img.copy()
    info = bench.dump_outputs(str(tmp_path / "a"), img)
    assert np.array_equal(img.view(np.uint32), keep.view(np.uint32))  # (the caller's image is left alone)
    got, nf = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "a" / "nonfinite.npy")
    assert got.dtype == np.float32 and nf.dtype == np.float64 and np.isfinite(got).all() and np.isfinite(nf).all()
    at = [(3 * 40 + 5) * 4 + k for k in range(4)] + [(7 * 40 + 1) * 4 + 2, (7 * 40 + 1) * 4 + 3]
    assert nf.tolist() == [[float(i), c] for i, c in zip(at, [1.0] * 4 + [2.0, 3.0])]
    assert info["nonfinite"]["count"] == 6 and info["nonfinite"]["shape"] == [6, 2]
    back = got.copy().reshape(-1)
    assert not back[nf[:, 0].astype(int)].any()
    back[nf[:, 0].astype(int)] = np.array([0, np.nan, np.inf, -np.inf], np.float32)[nf[:, 1].astype(int)]
    fin = np.isfinite(img)
    assert np.array_equal(back.reshape(img.shape)[fin].view(np.uint32), img[fin].view(np.uint32))
    assert np.array_equal(np.isnan(back.reshape(img.shape)), np.isnan(img))
    assert np.array_equal(back.reshape(img.shape)[~fin & ~np.isnan(img)], img[~fin & ~np.isnan(img)])
    assert info["image"]["sampled"] is False and info["image"]["shape"] == [40, 40, 4]
    monkeypatch.setattr(bench, "DUMP_NONFINITE", 16 * 12)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 16 * 12 + 16 * 58)
    img[:] = np.where(np.arange(40 * 40 * 4).reshape(img.shape) % 7 == 0, np.nan, img)
    info = bench.dump_outputs(str(tmp_path / "b"), img)
    bench.dump_outputs(str(tmp_path / "c"), img)
    b, c = np.load(tmp_path / "b" / "image.npy"), np.load(tmp_path / "c" / "image.npy")
    nb = np.load(tmp_path / "b" / "nonfinite.npy")
    assert b.dtype == np.float32 and b.shape == (50, 4) and np.isfinite(b).all()
    assert nb.shape == (4, 2) and info["nonfinite"]["count"] > 4 and np.array_equal(
        nb, np.load(tmp_path / "c" / "nonfinite.npy"))
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= bench.DUMP_LIMIT
    assert np.array_equal(b.view(np.uint32), c.view(np.uint32))
    assert info["image"]["sampled"] is True and info["image"]["of"] == [40, 40, 4]
    flat = {np.nan_to_num(r, nan=0.0).tobytes() for r in img.reshape(-1, 4)}
    assert all(r.tobytes() in flat for r in b)


def test_validate_needs_full():
    """--validate is one of the --full checks: a plain run refuses it before
    it imports the library or touches a GPU."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, bench.__file__, "--validate"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--full" in r.stderr


def test_executed_flops_drop_only_culled_work(counters):
    """roofline.frac's executed flops: each pass's algorithmic flops less its
    culled evaluations, each culled one still paying its test; without culls
    the two agree."""
    prog, ct, _ = counters
    st = dict(ct, wave_maps=0, wave_shapes=0)
    taps = _taps_share(ct)
    alg = (bench.trace_flops(st, taps, prog.n_aabb, True), bench.shade_flops(st, taps, prog.n_aabb))
    assert bench.executed_split(dict(st, culled=0), taps, prog.n_aabb, True) == pytest.approx(alg)
    st_c = dict(st, culled=st["xform_shape"] // 2)
    ex = bench.executed_split(st_c, taps, prog.n_aabb, True)
    assert ex[0] < alg[0] and ex[1] == pytest.approx(alg[1])
    per = bench.W_XFORM + bench.W_FINALISE + 1 - bench.W_CULL_TEST
    assert alg[0] - ex[0] >= st_c["culled"] * per  # (plus the mean SDF weight)


def _kernel_source(prog, data, baked: int) -> str:
    from compute_path_tracer_amd import _native as N

    return N.scene_kernel_source(prog, data, baked)


@pytest.mark.parametrize("scene", ["c1", "c2", "c3"])
def test_value_edit_leg_rebuilds_only_the_baked_kernel(scene):
    """bench.value_edit_leg's one-ulp edit: the table
    scene kernel's source is unchanged (no recompile: what an editing
    session renders meanwhile) and the values-baked source differs (its
    rebuild is what tier_up_s times -- a source no cache holds)."""
    from compute_path_tracer_amd import scenes
    from compute_path_tracer_amd.sdf_editor import CompData

    prog = scenes.SCENES[scene]().compile(CompData())
    for ulps in (1, 4095):
        k, edited = bench.edited_data(prog, ulps)
        assert k == bench.edit_slot(prog) and edited[k] > prog.data[k]
        assert np.count_nonzero(edited != prog.data) == 1
        assert _kernel_source(prog, prog.data, 0) == _kernel_source(prog, edited, 0)
        assert _kernel_source(prog, prog.data, 1) != _kernel_source(prog, edited, 1)
