"""CPU: tests/bakeref.py, the reference of the radiance queries (DESIGN.md
3.32), and the host-only mesh baking helpers (Mesh.bake_rays,
Mesh.lit_colors).  No GPU."""
import numpy as np
import pytest

import bakeref as B
import gpuharness as G
import pyref as P
import rayref as R
from compute_path_tracer_amd import scenes
from compute_path_tracer_amd.mesh import Mesh
from compute_path_tracer_amd.path_tracer import Radiance
from compute_path_tracer_amd.sdf_editor import CompData

F = np.float32


def test_seed_known_answers():
    """(i, seed, k) -> ((i * 1973 + seed * 9277 + k * 26699) mod 2^32) | 1, worked out by hand; the last five wrap."""
    for (i, seed, k), want in (((0, 0, 0), 1), ((1, 0, 0), 1973), ((0, 1, 0), 9277), ((0, 0, 1), 26699),
                               ((2, 3, 4), 138573), ((256, 7, 7), 756921),
                               ((67108863, 0, 0), 3556767819), ((0, 0xFFFFFFFF, 0), 4294958019),
                               ((5, 123456789, 16777215), 4105605183),
                               ((67108863, 4294967295, 16777215), 520055747),
                               ((4, 0, 160867), 28629)):
        assert B.seed_of(i, seed, k) == want, (i, seed, k)
    # gen_rng's form: pixel (a, b) of a w x h image whose a and b come out as i and seed
    assert B.seed_of(3, 5, 9) == ((3 * 1973 + 5 * 9277 + 9 * 26699) | 1)


def test_hemisphere_directions_are_cosine_distributed():
    n = P.normalize([F(0.36), F(0.48), F(0.8)])
    dots = []
    for i in range(4096):
        d = B.hemisphere_direction(n, P.Rng(B.seed_of(i, 7, 0)))
        assert abs(float(P.length(d)) - 1.0) < 1e-6
        dots.append(float(P.dot(d, n)))
    dots = np.array(dots)
    print(f"mean dot {dots.mean():.4f} (2/3 for the cosine distribution), least {dots.min():.3g}")
    assert abs(dots.mean() - 2.0 / 3.0) < 0.02
    assert dots.min() >= -1e-6


def test_hemisphere_draw_is_the_paths_diffuse_draw():
    """Two draws, z first: the direction pyref.path_trace forms after its specular draw."""
    rng, n = P.Rng(12345), [F(0.0), F(1.0), F(0.0)]
    z = rng.f01() * F(2.0) - F(1.0)
    a = rng.f01() * P.PI2
    r = F(np.sqrt(F(1.0) - z * z))
    sa, ca = P.sincos(a)
    want = P.normalize([n[0] + r * ca, n[1] + r * sa, n[2] + z])
    rng2 = P.Rng(12345)
    got = B.hemisphere_direction(n, rng2)
    assert [float(v) for v in got] == [float(v) for v in want] and rng2.s == rng.s


@pytest.mark.parametrize("mode", ["ray", "hemisphere"])
def test_continuation_equals_one_call(mode):
    """spp = 8 equals spp = 3, then sample0 = 3 with spp = 5, bit for bit; a non-finite ray stays NaN."""
    rows = scenes.SCENES["c2"]().rows()
    ro, rd = R.ray_set("c2")
    pick = [0, 14, 40, 100, 200, 255]  # (255: the NaN ray)
    ro, rd = ro[pick], rd[pick]
    sky = G.sky()
    whole = B.radiance(rows, ro, rd, 8, 0, 7, 4, mode, sky)
    first = B.radiance(rows, ro, rd, 3, 0, 7, 4, mode, sky)
    second = B.radiance(rows, ro, rd, 5, 3, 7, 4, mode, sky, previous=first)
    for a, b in zip(whole, second):
        assert G.same_or_nan(a, b).all()
    assert np.isnan(whole[0][5]).all() and np.isnan(whole[1][5]).all()
    assert np.isfinite(whole[0][:5]).all() and (whole[0][:5] > 0).any()
    assert not G.same_or_nan(first[0][:5], whole[0][:5]).all()
    # the first sample alone is its colour, and its moment the colour's square
    one = B.radiance(rows, ro[:2], rd[:2], 1, 0, 7, 4, mode, sky)
    col = B.sample_colours(rows, ro[:2], rd[:2], 1, 0, 7, 4, mode, sky)[:, 0]
    assert np.array_equal(one[0], col * F(1.0)) and np.array_equal(one[1], col * col)


def test_a_repeated_colour_does_not_fold_to_itself():
    """x * (1 - w) + x * w is not x: the fold of spp equal colours must run, no short cut."""
    x = np.array([[F(0.1), F(0.7), F(1.3)]], F)
    differs = []
    for spp in range(1, 65):
        mean, moment = B.fold(np.repeat(x[:, None], spp, 1))
        if (mean != x).any():
            differs.append(spp)
    print("sample counts at which the folded mean differs from the repeated colour:", differs[:16])
    assert differs and 1 not in differs


def test_bake_rays_and_lit_colors():
    prog = scenes.SCENES["c2"]().compile(CompData())
    pos = np.array([(0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (-0.5, 0.25, 0.125)], F)
    nrm = np.array([(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.6, -0.8)], F)
    mesh = Mesh(pos, nrm, [0, 1, -1], [(0, 1, 2)])
    o, d = mesh.bake_rays("irradiance")
    assert o.dtype == d.dtype == np.float32
    assert np.array_equal(o, pos + nrm * F(0.03)) and np.array_equal(d, nrm)
    assert o[0].tolist() == [0.0, float(F(0.03)), 0.0] and o[1].tolist() == [float(F(1.0) + F(0.03)), 2.0, 3.0]
    o2, d2 = mesh.bake_rays("view", offset=0.5)
    assert np.array_equal(o2, pos + nrm * F(0.5)) and np.array_equal(d2, -nrm)
    with pytest.raises(ValueError):
        mesh.bake_rays("albedo")
    mean = np.array([(0.5, 2.0, -1.0), (0.25, 0.0, 1.0), (1.0, 1.0, np.nan)], F)
    gamma = lambda v: np.clip(v, F(0.0), F(1.0)) ** F(1.0 / 2.2)  # noqa: E731
    view = mesh.lit_colors(Radiance(mean, mean * mean, 4, "ray"))
    assert view.dtype == np.float32 and view.shape == (3, 3)
    assert G.same_or_nan(view, gamma(mean).astype(F)).all()
    assert view[0].tolist() == [float(F(0.5) ** F(1.0 / 2.2)), 1.0, 0.0] and np.isnan(view[2, 2])
    albedo = mesh.vertex_colors(prog)
    assert (albedo[2] == 0).all() and (albedo[:2] > 0).any()
    lit = mesh.lit_colors(Radiance(mean, mean * mean, 4, "hemisphere"), prog)
    assert G.same_or_nan(lit, gamma(albedo * mean).astype(F)).all()
    with pytest.raises(ValueError):
        mesh.lit_colors(Radiance(mean, mean * mean, 4, "hemisphere"))  # an irradiance bake needs the albedo
    with pytest.raises(ValueError):
        mesh.lit_colors(Radiance(mean[:2], mean[:2], 4, "ray"))


def test_variance_of_the_mean():
    mean = np.array([[(0.5, 0.25, 1.0)], [(np.nan, 0.0, 0.0)]], F)
    moment = np.array([[(0.5, 0.0625, 0.5)], [(1.0, 1.0, 0.0)]], F)
    r = Radiance(mean, moment, 5, "ray")
    assert r.variance.shape == (2, 1) and r.variance.dtype == np.float32
    # (0.5 - 0.25) / 4 + 0 + max(0.5 - 1, 0) / 4; a NaN channel drops out
    assert r.variance[0, 0] == F(0.0625) and r.variance[1, 0] == F(0.25)
