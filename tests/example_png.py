"""The rules that pin a frame to the reference's example.png past the first hit,
once, for the oracle (test_example_png_cpu.py) and the device
(test_gpu_example_png.py). Fixtures and their derivation:
tests/golden/make_example_pins.py.

Metal cap (example_metal_cap.npz, METAL.n pixels of rows METAL.y0..METAL.y1 - 1):
a frame rendered at r=64, d=50, radius 0.5 with RICH_SETUP obeys
  (a) Scene.Hit count 128 at every masked pixel (64 samples x hit + sky);
  (b) |byte - PNG byte| <= 1 everywhere, blue == 188 (0.5 linear) exactly;
  (c) a differing R or G channel only where
      srgb_boundary_distance < SKY_EDGE_PINHOLE + SPREAD_FACTOR * spread,
      spread = the channel's footprint_spread. SPREAD_FACTOR = 0.2 is derived: a
      linear function of range `spread` on a uniform disc has sigma = spread/4,
      a 64-sample mean sigma = spread/32, the difference of two independent
      means sigma = 0.044 spread; 0.2 is 4.5 of those;
  (d) (c) exempts at most EXEMPT_SHARE = 0.40 of the R/G channels: >= 60 % of
      them are byte-exact pins;
  (e) differing channels <= MISS_FACTOR = 1.25 x the largest count of the
      numpy restatement against the PNG (4 jitter seeds, in the fixture);
  (f) for R and G, |mean(continuous sRGB - PNG byte)| over the mask and over
      each of its four quadrants <= BIAS_FACTOR = 3 x the largest such value
      of the numpy restatement (same seeds and regions, in the fixture);
  (g) the pixel-centre pinhole frame (r=1, aperture 0) equals analytic_color
      at zero offsets bit for bit, has Scene.Hit count 2, and obeys (b), (c).

Lambertian cap (example_lambert_cap.npz): per channel, the mean byte over the
cap lies within T = 5 SE + S of the PNG's mean, SE and S from the fixture, and
T <= 1 byte.
"""
import functools
import sys
import types

import numpy as np

from conftest import GOLDEN, SKY_EDGE_PINHOLE, load_golden, srgb_boundary_distance

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_example_pins as pins  # noqa: E402

SPP, DEPTH, RADIUS, WIDTH, HEIGHT = 64, 50, 0.5, 1280, 720
SPREAD_FACTOR = 0.2
EXEMPT_SHARE = 0.40
MISS_FACTOR = 1.25
BIAS_FACTOR = 3.0
BLUE = 188
LAMBERT_SE_FACTOR = 5.0
LAMBERT_T_MAX = 1.0


def _load(name):
    g = load_golden(name)
    h, w = (int(v) for v in g["shape"])
    mask = np.unpackbits(g["mask"])[: h * w].reshape(h, w).astype(bool)
    rows = np.nonzero(mask.any(1))[0]
    ys, xs = np.nonzero(mask)
    y0, y1 = int(rows.min()), int(rows.max()) + 1
    return g, dict(mask=mask, band=mask[y0:y1], y0=y0, y1=y1, xs=xs, ys=ys, n=int(mask.sum()),
                   rgb=g["rgb"].astype(int))


@functools.lru_cache(maxsize=None)
def metal_cap():
    g, d = _load("example_metal_cap")
    xmid, ymid = (int(v) for v in g["quadrant_split"])
    return types.SimpleNamespace(**d, regions=pins.quadrants(d["mask"], xmid, ymid),
                                 spread=pins.footprint_spread(d["mask"]),
                                 miss_max=int(g["restatement_misses"].max()),
                                 bias_max=float(g["restatement_bias"].max()))


@functools.lru_cache(maxsize=None)
def lambert_cap():
    g, d = _load("example_lambert_cap")
    se, s = g["standard_error"], g["scene_spread"]
    return types.SimpleNamespace(**d, se=se, scene_spread=s, scene_seeds=[int(v) for v in g["scene_seeds"]],
                                 tolerance=LAMBERT_SE_FACTOR * se + s, png_mean=d["rgb"].mean(0))


def _bytes_and_exemptions(lin, u8, what):
    """(b) and (c) on the metal mask; returns (miss, exempt) for the rules that follow."""
    m = metal_cap()
    d = np.abs(u8.astype(int) - m.rgb)
    miss = d > 0
    exempt = srgb_boundary_distance(lin) < SKY_EDGE_PINHOLE + SPREAD_FACTOR * m.spread
    outside = miss[:, :2] & ~exempt[:, :2]
    edge = srgb_boundary_distance(lin)[:, :2] - SKY_EDGE_PINHOLE
    ratio = float((edge[miss[:, :2]] / m.spread[:, :2][miss[:, :2]]).max()) if miss[:, :2].any() else 0.0
    print(f"{what}: max byte difference {int(d.max())}, differing channels {int(miss.sum())}, "
          f"exact pixels {float((~miss).all(1).mean()):.4f}, blue {np.unique(u8[:, 2])}, "
          f"misses outside the exemption {int(outside.sum())}, worst (distance - {SKY_EDGE_PINHOLE}) / spread "
          f"of a miss {ratio:.3f}")
    assert d.max() <= 1, f"{what}: (b) a byte is {int(d.max())} off example.png"
    assert np.all(u8[:, 2] == BLUE), f"{what}: (b) blue is not {BLUE} everywhere"
    assert not outside.any(), f"{what}: (c) {int(outside.sum())} channels differ away from a rounding boundary"
    return miss, exempt


def check_metal_frame(lin, u8, seg, what):
    """Rules (a)..(f) for an r=64 frame: lin [N, 3] linear, u8 [N, 3] its ToSRGBA bytes and
    seg [N] Scene.Hit counts at the metal mask's pixels (row-major). Returns the figures."""
    m = metal_cap()
    assert lin.shape == (m.n, 3) and u8.shape == (m.n, 3) and seg.shape == (m.n,)
    assert np.all(seg == 2 * SPP), f"{what}: (a) {int((seg != 2 * SPP).sum())} pixels are not hit + sky per sample"
    miss, exempt = _bytes_and_exemptions(lin, u8, what)
    share = float(exempt[:, :2].mean())
    cont = pins.srgb255(lin)
    means = [(cont[r][:, :2] - m.rgb[r][:, :2]).mean(0) for r in m.regions]
    bias = max(float(np.abs(v).max()) for v in means)
    print(f"{what}: exempt share {share:.4f} (<= {EXEMPT_SHARE}), differing channels {int(miss.sum())} "
          f"(<= {MISS_FACTOR} x {m.miss_max}), bias whole mask R, G {means[0]}, worst region {bias:.5f} "
          f"(<= {BIAS_FACTOR} x {m.bias_max:.5f})")
    assert share <= EXEMPT_SHARE, f"{what}: (d) {share:.3f} of the R/G channels are exempt"
    assert miss.sum() <= MISS_FACTOR * m.miss_max, f"{what}: (e) {int(miss.sum())} differing channels"
    assert bias <= BIAS_FACTOR * m.bias_max, f"{what}: (f) bias {bias:.5f} bytes"
    return dict(share=share, misses=int(miss.sum()), bias=bias)


def check_metal_pinhole(lin0, u8, seg, what):
    """Rule (g) for the r=1, aperture-0 frame at the metal mask's pixels."""
    m = metal_cap()
    want = pins.analytic_color(m.xs, m.ys)
    assert np.all(seg == 2), f"{what}: (g) {int((seg != 2).sum())} pixel-centre rays are not hit + sky"
    diff = lin0.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), f"{what}: (g) {int(diff.sum())} channels differ from analytic_color, " \
                           f"max {np.abs(lin0 - want).max():.3e}"
    _bytes_and_exemptions(lin0, u8, what)


def check_lambert_mean(u8, what):
    """The Lambertian cap statistic for u8 [N, 3], the frame's bytes at the cap's pixels."""
    c = lambert_cap()
    assert u8.shape == (c.n, 3)
    mean = u8.astype(np.float64).mean(0)
    print(f"{what}: cap mean {mean}, example.png {c.png_mean}, T {c.tolerance} = {LAMBERT_SE_FACTOR} x {c.se} + "
          f"{c.scene_spread}")
    assert np.all(c.tolerance <= LAMBERT_T_MAX)
    assert np.all(np.abs(mean - c.png_mean) <= c.tolerance), f"{what}: cap mean {mean} for {c.png_mean}"
    return mean


def pinhole_setup(setup):
    s = np.array(setup, dtype=np.float64)
    s[12] = 0.0
    return s


def oracle_pixels(O, scene, camera, xs, ys, spp, seed, workers):
    """O.render_pixels split over threads (the C call releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor

    parts = np.array_split(np.arange(len(xs)), max(1, min(len(xs), 8 * workers)))
    with ThreadPoolExecutor(workers) as ex:
        out = list(ex.map(lambda p: O.render_pixels(scene, pins_bg(), camera, WIDTH, HEIGHT, spp, DEPTH, RADIUS,
                                                    seed, xs[p], ys[p]), parts))
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def pins_bg():
    return np.array([*pins.BG[0], *pins.BG[1]])


def lambert_scene_spread(O, camera, workers, rng_seed=2):
    """S of the Lambertian statistic: max - min, per channel, of the oracle's cap mean byte
    over the fixture's scene seeds with the RNG seed held fixed. Only this spread
    enters the tolerance, never the means' location."""
    c = lambert_cap()
    means = []
    for scene_seed in c.scene_seeds:
        lin, _ = oracle_pixels(O, O.rich_scene(scene_seed), camera, c.xs, c.ys, SPP, rng_seed, workers)
        means.append(O.to_srgba(lin)[:, :3].astype(np.float64).mean(0))
    means = np.array(means)
    return means.max(0) - means.min(0), means
