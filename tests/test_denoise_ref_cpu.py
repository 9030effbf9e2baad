"""Properties of tests/denoise_ref.py, the numpy restatement of include/tray_denoise.h
that the device is compared with bit for bit (tests/test_gpu_denoise.py): what the
filter must do whatever computes it, and the quality condition on oracle frames."""
import numpy as np
import pytest

import denoise_frames
import denoise_ref as R
from conftest import load_golden


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rng_image(rows, width, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.random((rows, width, 3)), 0.05 + rng.random((rows, width, 3)), rng.normal(size=(rows, width, 3)),
            1.0 + 9.0 * rng.random((rows, width)))


@pytest.mark.parametrize("flags", [0, 1])
def test_constant_image_is_a_fixed_point(flags):
    """Every k and every partial sum of them is dyadic, so with a dyadic colour every product
    and sum is exact: acc = W * c and acc / W = c, bit for bit, borders included. For another
    constant each of the 25 sums, the products (together) and the division add a relative error
    of at most 2^-53: 27 * 2^-53 * 0.3 is 16.2 ulp of 0.3 (2^-54)."""
    rows, width = 19, 23
    _, albedo, normal, depth = _rng_image(rows, width)
    albedo = np.full_like(albedo, 0.5) if flags else albedo  # c_0 = colour / 0.5 stays dyadic
    for value in (0.25, 1.0, 3.0):
        c = np.full((rows, width, 3), value)
        out = R.denoise(c, albedo, np.zeros_like(normal), np.ones_like(depth), 5, flags)
        assert np.array_equal(bits(out), bits(c)), value
    c = np.full((rows, width, 3), 0.3)
    out = R.denoise(c, albedo, np.zeros_like(normal), np.ones_like(depth), 1, flags)
    assert np.abs(out - c).max() <= 17 * np.spacing(0.3)


def test_unchanged_across_a_guide_discontinuity_with_tiny_sigmas():
    """Two half-images that differ in depth (or in normal) by far more than a tiny sigma: no tap
    crosses the edge, so each half is filtered as if it were alone."""
    rows, width = 16, 24
    colour, albedo, normal, depth = _rng_image(rows, width)
    normal[:] = (0.0, 0.0, 1.0)
    depth[:] = 2.0
    split = 11
    for guide in ("depth", "normal"):
        n, z = normal.copy(), depth.copy()
        if guide == "depth":
            z[:, split:] = 7.0
        else:
            n[:, split:] = (1.0, 0.0, 0.0)
        kw = dict(iterations=4, flags=0, sigma_color=1e3, sigma_normal=1e-3, sigma_depth=1e-3)
        whole = R.denoise(colour, None, n, z, **kw)
        left = R.denoise(colour[:, :split], None, n[:, :split], z[:, :split], **kw)
        right = R.denoise(colour[:, split:], None, n[:, split:], z[:, split:], **kw)
        assert np.array_equal(bits(whole), bits(np.concatenate([left, right], axis=1))), guide
        assert not np.array_equal(whole, colour)  # it did filter within each half
    # and with a tiny colour sigma nothing but the centre tap survives: the image is unchanged
    # (acc / W = (k c) / k with k = 9/64: 9c rounds once and is divided back, within an ulp)
    same = R.denoise(colour, None, normal, depth, 3, 0, 1e-9, 1.0, 1.0)
    assert np.abs(same - colour).max() <= np.spacing(1.0)


@pytest.mark.parametrize("rows,width", [(1, 1), (1, 40), (40, 1)])
def test_degenerate_shapes(rows, width):
    colour, albedo, normal, depth = _rng_image(rows, width)
    out = R.denoise(colour, albedo, normal, depth, 8)
    assert out.shape == colour.shape and np.isfinite(out).all()
    if rows == width == 1:  # one tap, the centre: acc / W = (k c0) / k, then * m
        assert np.allclose(out, colour, rtol=4e-15, atol=0)  # 8 levels of two roundings, and the two of the albedo
    # a row image equals the same data as a column image
    t = R.denoise(colour.transpose(1, 0, 2), albedo.transpose(1, 0, 2), normal.transpose(1, 0, 2), depth.T, 8)
    assert np.array_equal(bits(t.transpose(1, 0, 2)), bits(out))


@pytest.mark.parametrize("flags", [0, 1])
def test_nan_pixel_passes_through_and_poisons_no_neighbour(flags):
    rows, width = 21, 27
    colour, albedo, normal, depth = _rng_image(rows, width)
    normal[:] = (0.0, 1.0, 0.0)
    depth[:] = 3.0
    bad = colour.copy()
    bad[9, 13] = np.nan
    bad[0, 0, 1] = np.nan  # one channel only, in a corner
    bad[20, 5] = np.inf
    out = R.denoise(bad, albedo, normal, depth, 5, flags, 10.0, 1.0, 1.0)  # wide sigmas: every tap counts
    assert np.isnan(out[9, 13]).all() and np.isnan(out[0, 0, 1]) and np.isinf(out[20, 5]).all()
    rest = np.ones((rows, width), dtype=bool)
    rest[9, 13] = rest[0, 0] = rest[20, 5] = False
    assert np.isfinite(out[rest]).all()
    # two levels reach 2 * (1 + 2) = 6 pixels: farther from the bad pixels nothing changes at all
    out2 = R.denoise(bad, albedo, normal, depth, 2, flags, 10.0, 1.0, 1.0)
    clean2 = R.denoise(colour, albedo, normal, depth, 2, flags, 10.0, 1.0, 1.0)
    yy, xx = np.mgrid[:rows, :width]
    far = np.ones((rows, width), dtype=bool)
    for y, x in ((9, 13), (0, 0), (20, 5)):
        far &= np.maximum(np.abs(yy - y), np.abs(xx - x)) > 6
    assert far.any() and np.array_equal(bits(out2[far]), bits(clean2[far]))
    assert np.isfinite(out2[rest]).all() and not np.array_equal(out2[rest & ~far], clean2[rest & ~far])
    # NaN or infinite guide values only remove taps
    z = depth.copy()
    z[4, 4], z[5, 5], z[6, 6], z[7, 7] = np.nan, np.inf, -1.0, 0.0
    n = normal.copy()
    n[8, 8] = np.nan
    out = R.denoise(colour, albedo, n, z, 5, flags, 10.0, 1.0, 1.0)
    assert np.isfinite(out).all()


def test_mse_falls_on_oracle_frames_with_the_default_sigmas(O):
    """The quality condition on the CPU: the 64x36 book cover at r = 16 against an independent
    r = 1024 frame (tests/golden/denoise_book_64x36.npz, from the oracle; the noisy frame is
    rendered again here to see the file is the oracle's)."""
    g = load_golden("denoise_book_64x36")
    spheres, cam = O.rich_scene(denoise_frames.SEED), denoise_frames.camera_state(O, 64, 36)
    noisy = O.render(spheres, denoise_frames.DEFAULT_BG, cam, 64, 36, 16, denoise_frames.DEPTH,
                     denoise_frames.RADIUS, denoise_frames.SEED, workers=2, segments=False)
    assert np.array_equal(bits(noisy), bits(g["noisy"]))
    rows = [3, 17, 30]  # the guides: three rows of them from the oracle again
    a, n, z = denoise_frames.oracle_guides(O, spheres, cam, 64, 36, 16, rows=rows)
    assert np.array_equal(bits(a), bits(g["albedo"][rows])) and np.array_equal(bits(n), bits(g["normal"][rows]))
    assert np.array_equal(bits(z), bits(g["depth"][rows]))
    out = R.denoise(g["noisy"], g["albedo"], g["normal"], g["depth"])  # the default parameters
    before = float(np.mean((g["noisy"] - g["target"]) ** 2))
    after = float(np.mean((out - g["target"]) ** 2))
    print(f"MSE noisy {before:.6e} denoised {after:.6e} ratio {after / before:.4f}")
    assert after < before


def test_restatement_defaults_are_the_library_defaults(L):
    import inspect

    p = L.denoise_params(4, 4)
    d = {k: v.default for k, v in inspect.signature(R.denoise).parameters.items() if v.default is not inspect._empty}
    assert (d["iterations"], d["flags"], d["sigma_color"], d["sigma_normal"], d["sigma_depth"]) == \
        (p.iterations, p.flags, p.sigma_color, p.sigma_normal, p.sigma_depth)
    assert R.FLOOR == 2.0 ** -10 and R.H5 == (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
