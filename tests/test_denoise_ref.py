"""Pins tests/denoiseref.py's a-trous filter on the CPU: the
properties the contract promises, on inputs whose answer is known without
running any other implementation."""
import numpy as np

import denoiseref as D

F = np.float32
OFF = dict(sigma_color=0.0, sigma_depth=0.0, sigma_albedo=0.0)


def _flat_guides(h, w, normal=(0.0, 0.0, -1.0), t=3.0, albedo=(0.5, 0.5, 0.5), hit=1.0):
    g0 = np.zeros((h, w, 4), np.float32)
    g1 = np.zeros((h, w, 4), np.float32)
    g0[..., :3], g0[..., 3] = normal, t
    g1[..., :3], g1[..., 3] = albedo, hit
    return g0, g1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_flat_image_comes_back_bit_identical():
    # w * 1 is w (and w * 2 is exact), so sc and sw are the same sums and sc / sw is the value
    g0, g1 = _flat_guides(19, 23)
    for v in (1.0, 2.0):
        img = np.full((19, 23, 4), v, np.float32)
        for params in (dict(), OFF, dict(OFF, normal_power_log2=0)):
            out = D.atrous(img, g0, g1, iterations=5, **params)
            assert np.array_equal(_bits(out), _bits(img))


def test_normal_edge_is_preserved_exactly():
    h, w = 21, 40
    img = np.ones((h, w, 4), np.float32)
    img[:, w // 2:, :3] = 2.0
    g0, g1 = _flat_guides(h, w, normal=(1.0, 0.0, 0.0))
    g0[:, w // 2:, :3] = (0.0, 1.0, 0.0)
    for npow in (1, 5):
        out = D.atrous(img, g0, g1, iterations=5, normal_power_log2=npow, **OFF)
        assert np.array_equal(_bits(out), _bits(img))  # the dot product is 0: nothing crosses the edge
    blurred = D.atrous(img, *_flat_guides(h, w), iterations=5, normal_power_log2=1, **OFF)
    assert not np.array_equal(_bits(blurred), _bits(img))  # (without the edge in the guides it does blur)


def test_one_iteration_reduces_variance_by_the_b3_weights():
    rng = np.random.default_rng(11)
    n = 128
    img = np.ones((n, n, 4), np.float32)
    img[..., :3] = rng.uniform(0.0, 1.0, (n, n, 3)).astype(np.float32)
    out = D.atrous(img, *_flat_guides(n, n), iterations=1, **OFF)
    inner = (slice(2, n - 2), slice(2, n - 2))
    ratio = float(out[inner][..., :3].astype(np.float64).var() / img[inner][..., :3].astype(np.float64).var())
    print(f"variance ratio {ratio:.4f} (sum of the squared weights: {(70 / 256) ** 2:.4f})")
    assert 0.06 <= ratio <= 0.09


def test_special_values_stay_and_spread_nowhere():
    rng = np.random.default_rng(3)
    h, w = 24, 31
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    at = {(5, 7, 0): np.nan, (12, 20, 1): np.inf, (18, 3, 2): -np.inf, (0, 0, 0): np.nan}
    for (y, x, k), v in at.items():
        img[y, x, k] = v
    g0, g1 = _flat_guides(h, w)
    for params in (dict(), OFF):
        out = D.atrous(img, g0, g1, iterations=5, **params)
        bad = np.zeros((h, w), bool)
        for (y, x, _k) in at:
            bad[y, x] = True
            assert np.array_equal(_bits(out[y, x]), _bits(img[y, x]))  # all four channels
        assert np.isfinite(out[~bad]).all()
        assert not np.array_equal(_bits(out[~bad]), _bits(img[~bad]))


def test_hit_and_miss_texels_never_mix():
    h, w = 16, 24
    img = np.ones((h, w, 4), np.float32)
    img[:, :w // 2, :3] = 4.0  # hits
    img[:, w // 2:, :3] = 0.25  # misses (sky next to sky weighs by colour only)
    g0, g1 = _flat_guides(h, w)
    g0[:, w // 2:] = (0.0, 0.0, 0.0, 200.0)
    g1[:, w // 2:] = 0.0
    out = D.atrous(img, g0, g1, iterations=4)
    assert np.array_equal(_bits(out), _bits(img))  # each side is flat: any mixing would change it


def test_tiny_and_ragged_sizes_keep_alpha():
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (2, 3)):
        img = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
        out = D.atrous(img, *_flat_guides(h, w), iterations=5)
        assert out.shape == img.shape and np.isfinite(out).all()
        assert np.array_equal(_bits(out[..., 3]), _bits(img[..., 3]))
    one = rng.uniform(0.0, 1.0, (1, 1, 4)).astype(np.float32)
    out = D.atrous(one, *_flat_guides(1, 1), iterations=1, **OFF)  # the centre tap alone: (w c) / w
    w0 = D.H[0] * D.H[0]
    assert np.array_equal(_bits(out[0, 0, :3]), _bits((w0 * one[0, 0, :3]) / w0))


def test_constants_are_the_contract_f32_steps():
    kc, kz, ka = D.constants(3, 4.0, 0.05, 0.1)
    assert kc == [F(1.0) / (F(4.0) * F(4.0)), F(1.0) / (F(2.0) * F(2.0)), F(1.0)]
    assert kz[1] == F(1.0) / ((F(0.05) * F(2.0)) * (F(0.05) * F(2.0))) and ka == F(1.0) / (F(0.1) * F(0.1))
    assert D.constants(2, 0.0, 0.0, 0.0) == ([F(0.0)] * 2, [F(0.0)] * 2, F(0.0))
