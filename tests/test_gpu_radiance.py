"""GPU: the radiance queries (pt_trace_radiance) bit for bit
against tests/bakeref.py (pinned on the CPU by test_radiance_ref.py).  16 x 16
contexts.  Floats are compared with same_or_nan (a NaN equal only to a NaN in
the same place).  The rays are rayref.ray_set's 257 per scene, the last two
non-finite; 8 samples, 4 bounces, seed 7 unless said."""
import ctypes
import functools

import numpy as np
import pytest

import bakeref as B
import gpuharness as G
import pyref as P
import rayref as R
from compute_path_tracer_amd import _native as N
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.sdf_editor import CompData
from gpuharness import EYE, TARGET

pytestmark = pytest.mark.gpu

F = np.float32
FP = ctypes.POINTER(ctypes.c_float)
SCENES = ["c2", "c3", "tiny", "nested", "nan-position"]
MODES = ["ray", "hemisphere"]
SPP, BOUNCES, SEED = 8, 4, 7


def _sky():
    return N.Sky((0.2, 0.15, 0.1), (0.5, 0.7, 1.0), (0.0, 0.8, -0.6), (4.0, 3.5, 3.0), 0.95)


def _tracer(scene="c2", sky=True, **options):
    """A 16 x 16 context with 2 bounces in its settings, the test sky set; no scene kernels: the query has none."""
    pt = G.tracer(scene, 16, 16, 2, extra={"jit": 0, **options})
    if sky and scene is not None:
        pt.set_sky(_sky())
    return pt


@functools.lru_cache(maxsize=None)
def _rays(name):
    ro, rd = R.ray_set(name)
    ro.setflags(write=False)
    rd.setflags(write=False)
    return ro, rd


@functools.lru_cache(maxsize=None)
def _colours(name, mode, sky, n=257, spp=SPP, bounces=BOUNCES):
    """bakeref's sample colours [n][spp][3] of the scene's first n rays, computed once and shared (read-only)."""
    ro, rd = _rays(name)
    c = B.sample_colours(scenes.SCENES[name]().rows(), ro[:n], rd[:n], spp, 0, SEED, bounces, mode, _sky() if sky else None)
    c.setflags(write=False)
    return c


def _assert_same(got, want, what):
    for name, a, b in (("mean", got[0], want[0]), ("moment", got[1], want[1])):
        same = G.same_or_nan(np.asarray(a, F), np.asarray(b, F)).all(-1)
        assert same.all(), (what, name, f"{int((~same).sum())} rays differ", np.nonzero(~same)[0][:5].tolist())


@pytest.mark.parametrize("sky", [False, True], ids=["void", "sky"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_both_modes_match_the_reference(gpu, name, mode, sky):
    ro, rd = _rays(name)
    colours = _colours(name, mode, sky)
    want = B.fold(colours)
    want[0][255:] = want[1][255:] = np.nan  # (bakeref.radiance's rule for the two non-finite rays)
    finite = colours[:255]
    nonzero = int((want[0][:255] != 0).any(-1).sum())
    differ = int((G.bits(finite) != G.bits(finite[:, :1])).any((1, 2)).sum())
    print(f"{name} {mode} sky {sky}: {nonzero} of 255 rays with a non-zero mean, {differ} whose samples differ")
    if sky:  # the data is not trivial
        assert nonzero >= 85 and differ >= 26
    pt = _tracer(name, sky)
    got = pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED, mode)
    assert got.mean.shape == got.moment.shape == (257, 3) and got.samples == SPP and got.mode == mode
    _assert_same((got.mean, got.moment), want, f"{name} {mode} sky {sky}")
    assert np.isnan(got.mean[255:]).all() and np.isnan(got.moment[255:]).all()
    with np.errstate(all="ignore"):
        v = np.fmax(got.moment - got.mean * got.mean, F(0.0)) / F(SPP - 1)
        assert G.same_or_nan(got.variance, (v[:, 0] + v[:, 1]) + v[:, 2]).all()
    pt.close()


def test_ragged_ray_counts_give_the_prefix(gpu):
    ro, rd = _rays("c2")
    pt = _tracer("c2")
    for mode in MODES:
        full = pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED, mode)
        for n in (1, 63, 64, 65, 257):
            got = pt.trace_radiance(ro[:n], rd[:n], SPP, BOUNCES, SEED, mode)
            _assert_same((got.mean, got.moment), (full.mean[:n], full.moment[:n]), f"{mode} n {n}")
    # leading dimensions are kept; no rays is a no-op
    got = pt.trace_radiance(ro[:6].reshape(2, 3, 3), rd[:6].reshape(2, 3, 3), SPP, BOUNCES, SEED)
    assert got.mean.shape == got.moment.shape == (2, 3, 3) and got.variance.shape == (2, 3)
    full = pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED)
    assert G.same_or_nan(got.mean.reshape(-1, 3), full.mean[:6]).all()
    assert pt.trace_radiance(np.zeros((0, 3)), np.zeros((0, 3)), SPP).mean.shape == (0, 3)
    p = N.RadianceParams(SPP, 0, SEED, BOUNCES, N.PT_RADIANCE_RAY)
    assert pt._L.pt_trace_radiance(pt._ctx, None, None, 0, ctypes.byref(p), None, None) == N.PT_OK
    pt.close()


@pytest.mark.parametrize("mode", MODES)
def test_ragged_sample_counts_match_the_reference(gpu, mode):
    """spp 1, 3, 64 and 65 on the first 16 rays of c2: below, at and past a wave's 64 lanes."""
    ro, rd = _rays("c2")
    colours = _colours("c2", mode, True, 16, 65)
    pt = _tracer("c2")
    for spp in (1, 3, 64, 65):
        got = pt.trace_radiance(ro[:16], rd[:16], spp, BOUNCES, SEED, mode)
        _assert_same((got.mean, got.moment), B.fold(colours[:, :spp]), f"{mode} spp {spp}")
    pt.close()


def test_null_outputs(gpu):
    ro, rd = (np.ascontiguousarray(a[:100]) for a in _rays("c2"))
    pt = _tracer("c2")
    full = pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED)
    p = N.RadianceParams(SPP, 0, SEED, BOUNCES, N.PT_RADIANCE_RAY)
    mean, moment = np.empty((100, 3), F), np.empty((100, 3), F)
    call = lambda a, b: pt._L.pt_trace_radiance(pt._ctx, N.fptr(ro), N.fptr(rd), 100, ctypes.byref(p), a, b)  # noqa: E731
    assert call(N.fptr(mean), None) == N.PT_OK and call(None, N.fptr(moment)) == N.PT_OK and call(None, None) == N.PT_OK
    _assert_same((mean, moment), (full.mean, full.moment), "one output at a time")
    pt.close()


def test_chunking_does_not_show(gpu):
    """radiance_samples at its minimum, spp = 16384: four rays fill a chunk, so
    five cross a boundary; the bits are those of one chunk, and the stream is
    the reference's."""
    ro, rd = _rays("tiny")
    finite = np.nonzero(np.isfinite(ro).all(-1) & np.isfinite(rd).all(-1))[0][:5]
    o, d = np.ascontiguousarray(ro[finite]), np.ascontiguousarray(rd[finite])
    assert finite.tolist() == [0, 1, 2, 3, 4]  # (so the reference's ray indices are the call's)
    pt = _tracer("tiny")
    assert pt.get_option("radiance_samples") == float(1 << 22)
    whole = pt.trace_radiance(o, d, 16384, BOUNCES, SEED)
    pt.set_option("radiance_samples", N.PT_RADIANCE_MAX_SPP)
    assert pt.get_option("radiance_samples") == 65536.0
    chunked = pt.trace_radiance(o, d, 16384, BOUNCES, SEED)
    _assert_same((chunked.mean, chunked.moment), (whole.mean, whole.moment), "two chunks against one")
    assert np.isfinite(whole.mean).all() and (whole.mean > 0).any(-1).all()
    # the first ray's first 64 samples are the reference's, and the whole call goes on from them
    first = pt.trace_radiance(o[:1], d[:1], 64, BOUNCES, SEED)
    _assert_same((first.mean, first.moment), B.fold(_colours("tiny", "ray", True, 1, 64)), "the first ray's first 64 samples")
    rest = pt.trace_radiance(o[:1], d[:1], 16384 - 64, BOUNCES, SEED, previous=first)
    assert rest.samples == 16384
    _assert_same((rest.mean, rest.moment), (whole.mean[:1], whole.moment[:1]), "64 samples, then the rest")
    assert G.refused(pt.set_option, "radiance_samples", 65535)[0] == N.PT_ERR_INVALID  # one ray must fit
    pt.close()


@pytest.mark.parametrize("mode", MODES)
def test_continuation(gpu, mode):
    ro, rd = _rays("c3")
    pt = _tracer("c3")
    whole = pt.trace_radiance(ro, rd, 8, BOUNCES, SEED, mode)
    first = pt.trace_radiance(ro, rd, 3, BOUNCES, SEED, mode)
    keep = first.mean.copy()
    second = pt.trace_radiance(ro, rd, 5, BOUNCES, SEED, mode, previous=first)
    assert second.samples == 8 and np.array_equal(G.bits(first.mean), G.bits(keep))  # previous is left as it was
    _assert_same((second.mean, second.moment), (whole.mean, whole.moment), f"{mode}: 3 + 5 against 8")
    assert not G.same_or_nan(first.mean, whole.mean).all()
    assert np.isnan(second.mean[255:]).all() and np.isnan(second.moment[255:]).all()
    # ... a non-finite ray answers NaN whatever the running values hold
    fake = first._replace(mean=np.ones_like(first.mean), moment=np.ones_like(first.moment))
    again = pt.trace_radiance(ro, rd, 5, BOUNCES, SEED, mode, previous=fake)
    assert np.isnan(again.mean[255:]).all() and np.isnan(again.moment[255:]).all() and np.isfinite(again.mean[:36]).all()
    pt.close()


def test_no_bounces_is_emission_and_sky(gpu):
    """bounces = 0: the first segment's emission, or the sky where it misses; no sample draws anything that shows."""
    ro, rd = _rays("c2")
    pt = _tracer("c2")
    got = pt.trace_radiance(ro, rd, SPP, 0, SEED)
    _assert_same((got.mean[:64], got.moment[:64]), B.fold(_colours("c2", "ray", True, 64, SPP, 0)), "bounces 0")
    other = pt.trace_radiance(ro, rd, SPP, 0, SEED + 1)
    _assert_same((other.mean, other.moment), (got.mean, got.moment), "bounces 0, another seed")
    hits = pt.trace_rays(ro, rd)
    miss = np.nonzero(~hits.hit)[0]
    assert len(miss) >= 1 and hits.hit[:255].sum() >= 10
    sky = P.sky_fields(_sky())
    for i in miss[:10]:
        g = np.array(P.sky_radiance(sky, [F(v) for v in rd[i]])[0], F)
        want = B.fold(np.repeat((F(0.0) + g * F(1.0))[None, None], SPP, 1))
        _assert_same((got.mean[i:i + 1], got.moment[i:i + 1]), want, f"the sky along ray {i}")
    deeper = pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED)
    assert not G.same_or_nan(deeper.mean, got.mean).all()
    pt.close()


def test_the_sky_enters_the_camera_and_tiles_do_not(gpu):
    ro, rd = _rays("c2")
    pt = _tracer("c2", sky=False)
    dark = pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED)
    pt.set_sky(_sky())
    lit = pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED)
    assert not G.same_or_nan(lit.mean, dark.mean).all() and np.nansum(lit.mean) > np.nansum(dark.mean)
    pt.look_at(EYE, TARGET, aperture=0.05, focus=3.0)
    pt.set_tiles(1, 2)
    moved = pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED)
    _assert_same((moved.mean, moved.moment), (lit.mean, lit.moment), "after pt_set_camera and pt_set_tiles(1, 2)")
    # bounces=None is the settings' value (2 here)
    two = pt.trace_radiance(ro, rd, SPP, seed=SEED)
    _assert_same((two.mean, two.moment), tuple(pt.trace_radiance(ro, rd, SPP, 2, SEED)[:2]), "bounces None")
    pt.close()


def test_isolation(gpu):
    """The image, the moments, the guides with their valid flag and the history are bit-identical before and after."""
    ro, rd = _rays("c2")
    pt = _tracer("c2", kernel="binned", moments=1)
    k = G.constants(16, 16, 1, 0)
    pt.look_at(EYE, TARGET)
    pt.dispatch(k, 2)
    assert pt.get_option("guides_valid") == 0.0
    pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED)
    assert pt.get_option("guides_valid") == 0.0  # a query renders no guides
    pt.render_guides(k)
    pt.accumulate_history()
    state = lambda: [pt.get_option(o) for o in ("guides_valid", "moments_valid", "moment_frames", "history_valid",  # noqa: E731
                                                "history_views", "kernel")]
    snap = lambda: b"".join(x.tobytes() for x in (pt.read_image(), *pt.read_guides(), pt.read_moments(),  # noqa: E731
                                                  *pt.read_history()))
    st, sn = state(), snap()
    assert st[:5] == [1.0, 1.0, 2.0, 1.0, 1.0]
    cam, sky = bytes(pt.get_camera()[0]), bytes(pt.get_sky()[0])
    for mode in MODES:
        pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED, mode)
    assert state() == st and snap() == sn
    assert bytes(pt.get_camera()[0]) == cam and bytes(pt.get_sky()[0]) == sky
    assert pt.read_image()[..., :3].mean() > 0
    pt.close()


def test_refusals_in_their_order(gpu):
    """Each refusal of the contract's list, the one before it winning, on a
    context without a program (so every one comes before PT_ERR_STATE); the
    sentinel-filled outputs stay unwritten."""
    L = N.lib()
    rays = np.zeros((4, 3), F)
    rays[:, 2] = 1.0
    rp = rays.ctypes.data_as(FP)
    mean, moment = np.full((4, 3), 5.0, F), np.full((4, 3), 9.0, F)
    mp, qp = mean.ctypes.data_as(FP), moment.ctypes.data_as(FP)
    untouched = lambda: (mean == 5.0).all() and (moment == 9.0).all()  # noqa: E731
    good = dict(spp=4, sample0=0, seed=1, bounces=2, mode=N.PT_RADIANCE_RAY)
    par = lambda **kw: ctypes.byref(N.RadianceParams(**{**good, **kw}))  # noqa: E731
    pt = _tracer(None)
    ctx = pt._ctx

    def refused(why, *args):
        assert L.pt_trace_radiance(*args) == N.PT_ERR_INVALID, why
        assert why.encode() in L.pt_last_error(ctx), (why, L.pt_last_error(ctx))
        assert untouched(), why

    assert L.pt_trace_radiance(None, rp, rp, 4, par(), mp, qp) == N.PT_ERR_INVALID
    refused("null radiance parameters", ctx, rp, rp, N.PT_RAYS_MAX + 1, None, mp, qp)
    refused("PT_RAYS_MAX", ctx, None, rp, N.PT_RAYS_MAX + 1, par(spp=0), mp, qp)
    refused("PT_RAYS_MAX", ctx, rp, rp, 0xFFFFFFFF, par(), mp, qp)
    refused("null ray", ctx, None, rp, 4, par(spp=0), mp, qp)
    refused("null ray", ctx, rp, None, 4, par(mode=2), mp, qp)
    refused("spp outside", ctx, rp, rp, 4, par(spp=0, sample0=3), None, qp)
    refused("spp outside", ctx, rp, rp, 4, par(spp=N.PT_RADIANCE_MAX_SPP + 1), mp, qp)
    refused("sample0 + spp", ctx, rp, rp, 4, par(sample0=(1 << 24) - 3, bounces=-1), mp, qp)
    refused("sample0 + spp", ctx, rp, rp, 4, par(sample0=0xFFFFFFFF), mp, qp)
    refused("negative bounces", ctx, rp, rp, 4, par(bounces=-1, mode=7), mp, qp)
    refused("bad radiance mode", ctx, rp, rp, 4, par(mode=2, sample0=3), None, qp)
    refused("bad radiance mode", ctx, rp, rp, 4, par(mode=-1), mp, qp)
    refused("continuation", ctx, rp, rp, 4, par(sample0=3), None, qp)
    refused("continuation", ctx, rp, rp, 4, par(sample0=3), mp, None)
    # the ranges' last valid values pass these checks: then no program, then no data
    edge = par(spp=N.PT_RADIANCE_MAX_SPP, sample0=(1 << 24) - N.PT_RADIANCE_MAX_SPP, bounces=0, mode=N.PT_RADIANCE_HEMISPHERE)
    assert L.pt_trace_radiance(ctx, rp, rp, 4, edge, mp, qp) == N.PT_ERR_STATE
    assert L.pt_trace_radiance(ctx, None, None, 0, par(), None, None) == N.PT_ERR_STATE
    prog = scenes.SCENES["c2"]().compile(CompData())
    pt.remake_pipeline(prog)
    assert L.pt_trace_radiance(ctx, rp, rp, 4, par(), mp, qp) == N.PT_ERR_STATE
    assert untouched()
    pt.set_data(prog.data)
    refused("continuation", ctx, rp, rp, 4, par(sample0=3), None, None)
    # and the next valid call works
    assert L.pt_trace_radiance(ctx, rp, rp, 4, par(), mp, qp) == N.PT_OK and not untouched()
    with pytest.raises(ValueError):
        pt.trace_radiance(rays, rays, 4, mode="sphere")
    with pytest.raises(ValueError):
        pt.trace_radiance(rays, rays[:2], 4)
    pt.close()


def test_baking(gpu):
    """bake_mesh is trace_radiance over Mesh.bake_rays, its first vertices the reference's; irradiance() is pi x the mean."""
    ed = scenes.SCENES["tiny"]()
    prog, rows = ed.compile(CompData()), ed.rows()
    pt = _tracer(prog)
    mesh = pt.extract_mesh((-1.0, -1.2, 1.2), (2.0, 1.2, 3.6), resolution=16)  # (the lamp and the box)
    nv = len(mesh.positions)
    print(f"tiny at resolution 16: {nv} vertices")
    assert nv >= 64
    for mode, rmode in (("irradiance", "hemisphere"), ("view", "ray")):
        baked = pt.bake_mesh(mesh, 4, mode=mode, bounces=BOUNCES, seed=SEED)
        o, d = mesh.bake_rays(mode)
        direct = pt.trace_radiance(o, d, 4, BOUNCES, SEED, rmode)
        assert baked.mode == rmode and baked.samples == 4 and baked.mean.shape == (nv, 3)
        _assert_same((baked.mean, baked.moment), (direct.mean, direct.moment), f"bake_mesh {mode}")
        want = B.radiance(rows, o[:64], d[:64], 4, 0, SEED, BOUNCES, rmode, _sky())
        _assert_same((baked.mean[:64], baked.moment[:64]), want, f"bake_mesh {mode} against the reference")
        assert np.isfinite(baked.mean).all() and (baked.mean > 0).any()
        colours = mesh.lit_colors(baked, prog)
        assert colours.shape == (nv, 3) and colours.min() >= 0.0 and colours.max() <= 1.0 and colours.max() > 0.0
    more = pt.bake_mesh(mesh, 4, mode="view", bounces=BOUNCES, seed=SEED, previous=baked)
    assert more.samples == 8
    _assert_same((more.mean, more.moment), tuple(pt.bake_mesh(mesh, 8, mode="view", bounces=BOUNCES, seed=SEED)[:2]), "4 + 4")
    e = pt.irradiance(mesh.positions, mesh.normals, 4, BOUNCES, SEED)
    hemi = pt.bake_mesh(mesh, 4, bounces=BOUNCES, seed=SEED)
    assert e.dtype == np.float32 and np.array_equal(G.bits(e), G.bits(hemi.mean * F(np.pi)))
    pt.close()


def test_timers_and_memory(gpu):
    ro, rd = _rays("c2")
    pt = _tracer("c2")
    assert pt.get_option("radiance_ms") == 0.0 and pt.get_option("radiance_bytes") == 0.0
    pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED)
    total, first = pt.get_option("radiance_ms"), pt.get_option("radiance_first_ms")
    assert total > 0.0 and 0.0 < first < total
    # rays and directions, means and moments 12 B per ray each, first hits 32 B per ray, colours 16 B per sample
    assert pt.get_option("radiance_bytes") == 257 * (4 * 12 + 32 + SPP * 16)
    pt.trace_radiance(ro, rd, SPP, BOUNCES, SEED, "hemisphere")
    assert pt.get_option("radiance_ms") > 0.0 and pt.get_option("radiance_first_ms") == 0.0
    pt.close()
