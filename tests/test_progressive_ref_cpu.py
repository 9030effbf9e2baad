"""tests/progressive_ref.py, the numpy restatement of include/tray_progressive.h, on the CPU:
the properties the header states for the accumulator, the metric and the variance-guided
filter, and the two quality conditions on oracle frames. The device is compared with this
restatement bit for bit in tests/test_gpu_progressive.py."""
import numpy as np
import pytest

import denoise_frames as F
import denoise_ref as DR
import progressive_ref as R
from conftest import DEFAULT_BG, load_golden

U = 2.0 ** -53
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ Welford --
def test_welford_equals_numpy_within_the_derived_bound():
    """With M = max |x| and u = 2^-53. Mean: each step rounds x - mean, t / n and the sum, each on
    values <= 2M, so a step adds at most 4uM (first order) and n steps 4nuM; np.mean's own sum is
    within nuM. Bound: 5nuM. M2: the step's term t * (x - mean) is a product of two values <= 2M
    that each carry the mean's error (<= 4nuM) and one rounding (<= 2uM), plus the product's and
    the sum's roundings (<= 4uM^2 each, M2 <= 4nM^2 rounded per step): at most
    (16n + 12 + 4n) u M^2 per step, (20n^2 + 12n) u M^2 over n steps, divided by n (n - 1) for
    the variance of the mean; np.var's two-pass result is within 4nuM^2 / (n (n - 1))."""
    rng = np.random.default_rng(1)
    for n in (2, 5, 16):
        x = rng.random((n, 9, 11, 3))
        mean, m2, count = R.fold(None, x)
        assert count == n
        M = float(np.abs(x).max())
        assert np.abs(mean - np.mean(x, axis=0)).max() <= 5 * n * U * M
        bound = (20 * n * n + 16 * n) * U * M * M / (n * (n - 1))
        assert np.abs(R.variance_of_mean(m2, n) - np.var(x, axis=0, ddof=1) / n).max() <= bound
        assert (m2 >= 0).all()  # rounding is monotone: the new mean lies between the old one and x


def test_splitting_the_fold_changes_no_bit():
    x = np.random.default_rng(2).normal(size=(5, 7, 5, 3))
    whole = R.fold(None, x)
    for first in (1, 2, 4):
        part = R.fold(R.fold(None, x[:first]), x[first:])
        assert part[2] == 5 and np.array_equal(bits(part[0]), bits(whole[0]))
        assert np.array_equal(bits(part[1]), bits(whole[1]))
    state = R.fold(None, x[:2])
    keep = (state[0].copy(), state[1].copy())
    R.fold(state, x[2:])
    assert np.array_equal(state[0], keep[0]) and np.array_equal(state[1], keep[1])  # inputs are not modified


def test_one_frame_has_infinite_variance_and_counts_every_pixel():
    x = np.random.default_rng(3).random((1, 4, 6, 3))
    mean, m2, n = R.fold(None, x)
    assert n == 1 and np.array_equal(bits(mean), bits(x[0])) and not m2.any()
    assert np.isposinf(R.variance_of_mean(m2, n)).all()
    count, most, converged = R.metric(mean, m2, n, tolerance=1e6)
    assert count == 24 and most == INF and not converged.any()


def test_a_nan_stays_in_its_pixel_and_counts():
    x = np.random.default_rng(4).random((4, 5, 6, 3))
    x[2, 1, 3, 0] = NAN
    x[1, 4, 0, 2] = INF
    mean, m2, n = R.fold(None, x)
    bad = np.zeros(mean.shape, dtype=bool)
    bad[1, 3, 0] = bad[4, 0, 2] = True
    assert np.array_equal(~np.isfinite(mean), bad) and np.array_equal(~np.isfinite(m2), bad)
    count, most, converged = R.metric(mean, m2, n, tolerance=1e6)
    assert count == 2 and not converged[1, 3] and not converged[4, 0] and np.isfinite(most)
    clean = x.copy()
    clean[:, 1, 3] = clean[:, 4, 0] = 0.5  # the two pixels without noise (q = 0): the same maximum
    assert R.metric(*R.fold(None, clean), tolerance=1e6)[:2] == (0, most)


def test_metric_rule():
    """v <= T * max(e, floor): tolerance 0 converges only a pixel without noise; the floor
    takes over for dark pixels."""
    x = np.zeros((3, 1, 3, 3))
    x[:, 0, 0] = 0.5  # no noise
    x[:, 0, 1] = [[0.5] * 3, [0.6] * 3, [0.7] * 3]
    x[:, 0, 2] = [[0.0] * 3, [1e-4] * 3, [2e-4] * 3]  # dark: measured against the floor
    mean, m2, n = R.fold(None, x)
    assert R.metric(mean, m2, n, tolerance=0.0)[0] == 2
    var = R.variance_of_mean(m2, n)
    v, e = var.sum(axis=-1), (mean * mean).sum(axis=-1)
    assert e[0, 2] < R.FLOOR < e[0, 1]
    count, most, converged = R.metric(mean, m2, n)
    assert converged[0, 0] and converged[0, 2] and not converged[0, 1]  # 0.1 / sqrt(3) / 0.6 > 0.05
    assert most == pytest.approx(v[0, 1] / e[0, 1], rel=1e-12)
    assert R.metric(mean, m2, n, floor=1e-12)[0] == 2  # without the floor the dark pixel is noisy


# ------------------------------------------------------------------- filter --
@pytest.fixture(scope="module")
def book():
    return load_golden("denoise_book_64x36")


def guides_of(g):
    return g["albedo"], g["normal"], g["depth"]


def test_zero_variance_returns_the_input_within_the_epsilon_bound(book):
    """With zero variance den = epsilon, so a tap is taken only when |d|^2 < epsilon: every
    taken colour is within sqrt(epsilon) of the centre's per channel, and so is their weighted
    mean. The mean of up to 25 terms rounds at most 27 times, < 32 u |c|. Over the levels, in
    demodulated units, and back through m <= max m, plus the two roundings of (colour / m) * m:
    |out - colour| <= iterations * (sqrt(epsilon) + 32 u max|c_0|) * max m + 2 u max|colour|."""
    colour = book["noisy"]
    albedo, normal, depth = guides_of(book)
    zero = np.zeros_like(colour)
    for eps in (1e-12, 1e-20):
        out, v = R.denoise_variance(colour, zero, albedo, normal, depth, epsilon=eps)
        m = DR.floor_albedo(albedo)
        bound = 5 * (np.sqrt(eps) + 32 * U * np.abs(colour / m).max()) * m.max() + 2 * U * np.abs(colour).max()
        err = float(np.abs(out - colour).max())
        print(f"zero variance, epsilon {eps:g}: L-inf {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert not v.any()  # and the propagated variance stays zero
    assert bound < 1e-9


def test_infinite_variance_is_the_filter_with_the_colour_term_off(book):
    """g = inf gives r = 0 and x_c = 0: b(x_c) = 1 at every tap. tray_denoise.h with a
    sigma_color whose square overflows has q_c = 1 / inf = 0: the same weights, the same bits."""
    colour = book["noisy"]
    albedo, normal, depth = guides_of(book)
    inf = np.full_like(colour, INF)
    for flags in (1, 0):
        out, v = R.denoise_variance(colour, inf, albedo, normal, depth, flags=flags)
        off = DR.denoise(colour, albedo, normal, depth, flags=flags, sigma_color=1e200)
        assert np.array_equal(bits(out), bits(off)) and np.isposinf(v).all()
        assert not np.array_equal(out, DR.denoise(colour, albedo, normal, depth, flags=flags))


@pytest.mark.parametrize("rows,width", [(1, 1), (1, 9), (9, 1), (2, 3)])
def test_degenerate_shapes(rows, width):
    rng = np.random.default_rng(5)
    colour = 0.5 + 0.01 * rng.random((rows, width, 3))
    variance = np.full((rows, width, 3), 1e-4)
    out, v = R.denoise_variance(colour, variance, flags=0, iterations=8)
    assert out.shape == colour.shape and v.shape == (rows, width)
    assert np.isfinite(out).all() and np.isfinite(v).all() and (v > 0).all()
    assert out.min() >= colour.min() - 1e-15 and out.max() <= colour.max() + 1e-15  # weighted means
    if rows * width == 1:  # the centre tap alone: (k c) / k and (k^2 v) / (k k)
        assert np.allclose(out, colour, rtol=4 * U, atol=0) and np.allclose(v, 3e-4, rtol=8 * U, atol=0)


@pytest.mark.parametrize("flags", [0, 1])
def test_nan_colour_and_nan_variance_reach_no_neighbours_colour(flags):
    rng = np.random.default_rng(6)
    rows, width = 12, 14
    colour = 0.5 + 0.05 * rng.random((rows, width, 3))
    albedo = 0.4 + 0.2 * rng.random((rows, width, 3))
    variance = np.full((rows, width, 3), 4e-4)
    colour[5, 6, 1] = NAN
    variance[8, 3, 2] = NAN
    out, v = R.denoise_variance(colour, variance, albedo, flags=flags, iterations=3)
    bad = np.zeros((rows, width), dtype=bool)
    bad[5, 6] = True
    assert np.array_equal(np.isnan(out).any(axis=-1), bad)  # the NaN colour: its own pixel only
    assert np.isnan(out[5, 6, 1]) and np.isnan(v[8, 3])  # and the NaN variance stays in the noise plane
    clean_v = variance.copy()
    clean_v[8, 3] = 4e-4
    clean, _ = R.denoise_variance(colour, clean_v, albedo, flags=flags, iterations=3)
    assert not np.array_equal(out[8, 3], clean[8, 3])  # that pixel fell back to epsilon alone
    assert np.abs(out[8, 3] - colour[8, 3]).max() < 1e-5


def test_propagated_variance_of_a_constant_image():
    """Constant colour: every in-image tap has w = k, so v_1 = (sum k^2) / (sum k)^2 * v; in the
    interior sum k = 1 and sum k^2 = (sum h^2)^2 = (35 / 128)^2."""
    rows, width, v0 = 9, 11, 3e-3
    colour = np.full((rows, width, 3), 0.25)
    variance = np.full((rows, width, 3), v0 / 4)  # (v/4 + v/4) + v/4 is not v0 exactly: take the sum
    s = (variance[0, 0, 0] + variance[0, 0, 1]) + variance[0, 0, 2]
    out, v = R.denoise_variance(colour, variance, flags=0, iterations=1)
    assert np.array_equal(out, colour)
    h = np.array(DR.H5)
    for y, x in ((4, 5), (0, 0), (1, 9), (8, 10), (0, 5)):
        ky = h[[d + 2 for d in range(-2, 3) if 0 <= y + d < rows]]
        kx = h[[d + 2 for d in range(-2, 3) if 0 <= x + d < width]]
        k = np.outer(ky, kx)
        assert v[y, x] == pytest.approx((k * k).sum() / k.sum() ** 2 * s, rel=1e-14), (y, x)
    assert v[4, 5] == pytest.approx((35 / 128) ** 2 * s, rel=1e-14)


def test_prefilter_renormalises_at_the_border():
    v = np.full((5, 6), 2.0)
    for s in (1, 2, 4, 8):
        assert np.array_equal(R.prefilter(v, s), v)
    v[0, 0] = 18.0
    g = R.prefilter(v, 1)
    assert g[0, 0] == (0.25 * 18 + 0.125 * 2 + 0.125 * 2 + 0.0625 * 2) / 0.5625 and g[1, 1] == 2 + 16 * 0.0625
    assert g[0, 2] == 2.0 and R.prefilter(v, 2)[2, 2] == 3.0 and R.prefilter(v, 8)[0, 0] == 18.0


def test_restatement_defaults_are_the_library_defaults(L):
    import inspect

    p = L.denoise_variance_params(4, 4)
    d = {k: v.default for k, v in inspect.signature(R.denoise_variance).parameters.items()
         if v.default is not inspect.Parameter.empty and v.default is not None}
    assert d == dict(iterations=p.iterations, flags=p.flags, sigma_variance=p.sigma_variance,
                     sigma_normal=p.sigma_normal, sigma_depth=p.sigma_depth, epsilon=p.epsilon)
    mp = L.accum_metric_params()
    assert (R.TOLERANCE, R.FLOOR) == (mp.tolerance, mp.floor)


# ------------------------------------------------------- quality conditions --
def test_quality_conditions_on_oracle_frames(O, book):
    """The 64x36 book cover, seed 2, d = 50: passes rendered by the oracle (sample words 0..255),
    the guides and the r = 1024 target of tests/golden/denoise_book_64x36.npz (words 1024..2047),
    default parameters. (a) 4 passes of r = 4: the variance-guided mean is closer to the target
    than the mean. (b) 16 passes of r = 16: closer than the plain filter of tray_denoise.h with
    its defaults on the same mean. Conditions, not tuned numbers; the ratios are printed
    (DESIGN.md 8k)."""
    spheres = O.rich_scene(F.SEED)
    cam = F.camera_state(O, 64, 36)
    albedo, normal, depth = guides_of(book)
    target = book["target"]
    mse = lambda a: float(np.mean((a - target) ** 2))  # noqa: E731

    def state(r, passes):
        frames = np.stack([O.render(spheres, DEFAULT_BG, cam, 64, 36, r, F.DEPTH, F.RADIUS, F.SEED, workers=4,
                                    segments=False, pass_=p) for p in range(passes)])
        mean, m2, n = R.fold(None, frames)
        return frames, mean, R.variance_of_mean(m2, n)

    frames, mean, variance = state(4, 4)
    guided, _ = R.denoise_variance(mean, variance, albedo, normal, depth)
    print(f"(a) 4 x r=4: MSE mean {mse(mean):.6e}, variance-guided {mse(guided):.6e}, "
          f"ratio {mse(guided) / mse(mean):.4f}")
    assert mse(guided) < mse(mean)

    frames, mean, variance = state(16, 16)
    assert np.array_equal(frames[0], book["noisy"])  # pass 0 at r = 16 is the file's noisy frame
    guided, _ = R.denoise_variance(mean, variance, albedo, normal, depth)
    plain = DR.denoise(mean, albedo, normal, depth)
    print(f"(b) 16 x r=16: MSE mean {mse(mean):.6e}, variance-guided {mse(guided):.6e} "
          f"(ratio {mse(guided) / mse(mean):.4f}), plain filter {mse(plain):.6e} "
          f"(ratio {mse(plain) / mse(mean):.4f})")
    assert mse(guided) < mse(plain)
