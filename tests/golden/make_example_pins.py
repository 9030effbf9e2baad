"""Generate tests/golden/example_metal_cap.npz and example_lambert_cap.npz (run
from the repo root):

    python tests/golden/make_example_pins.py [--reference /root/reference]

The reference's own output example.png (`tray -save example.png -r 64 -s 8
-d 50 -seed 2`, 1280x720, r=64, d=50; see make_sky_mask.py) holds the Go
binary's pixels of a RichScene whose small spheres are unknown (fortio.org/rand
is not vendored). Two regions of it do not depend on them, or only weakly. This
file is the only one that opens example.png; it uses make_golden.py's numpy
restatement of Camera.Initialize and numpy, neither oracle/ nor the kernel.

1. The upper cap of the Metal{Fuzz: 0} sphere at (4,1,0) (objects.go:171-172).
   Camera rays from y = 2 reach a point with y > 1 above every small sphere
   (all inside y <= 0.4, make_sky_mask.py); a reflection that points upward
   leaves from y > 1 and can only meet the two other R = 1 spheres or the sky.
   Where it meets the sky, a sample's colour is
       Mul(albedo, AmbientLight.Hit(Reflect(Unit(d), n)))
   (objects.go:49-73, materials.go:28-37, vec3.go:133-135): no draw but the
   anti-aliasing and the lens offsets, and Scene.Hit is called exactly twice.
   A pixel is in the METAL MASK when every ray of its footprint
     * hits the (4,1,0) sphere first (of the four fixed spheres) at a point with
       y > 1 + MARGIN,
     * reflects with a unit direction of y > MARGIN,
     * and the reflected ray misses the (0,1,0) and (-4,1,0) spheres enlarged to
       R = ENLARGED.
   The footprint is the pixel-centre ray plus N_AA = 16 points on the
   anti-aliasing circle x N_LENS = 8 points on the lens circle, each circle
   also paired with the other's centre, at FACTOR = 1.1 x the radii (0.5 px,
   tracer.go:138 RayRadius; 0.05, camera.go:85). With MARGIN = 0.02 that gives
   72,347 pixels in rows 55..278.
   The fixture also records what an independent 64-sample restatement (this
   file's analytic_color under numpy's own jitter streams, RESTATEMENT_SEEDS)
   differs from example.png by: the number of differing channels per seed and
   the largest |mean(continuous sRGB - PNG byte)| over R, G, the whole mask and
   its four quadrants. Both numbers bound what tests/example_png.py accepts.

2. The upper cap of the Lambertian sphere at (-4,1,0) (objects.go:168-169):
   scene-dependent only through what diffuse bounces see of the small spheres,
   so only its MEAN is a pin. A pixel is in the LAMBERT MASK when every ray of
   the same footprint hits that sphere first at y > LAMBERT_Y; footprint rays
   that hit the (0,1,0) or the (4,1,0) sphere enlarged to R = ENLARGED
   (both overlap it as seen from the camera) exclude the pixel. LAMBERT_Y = 1.5
   gives 3,515 pixels (rows 59..111). The fixture records SE, the standard
   error of the PNG's own mean byte (variance of horizontally adjacent masked
   pixels' differences / 2 / N), and S = LAMBERT_SCENE_SPREAD, the max - min of the C oracle's cap
   mean over the scene seeds 2..9 at RNG seed 2. S is measured by
   tests/example_png.py:lambert_scene_spread (this file does not touch the
   oracle) and tests/test_example_png_cpu.py checks the constant against it.
   The glass sphere's cap is NOT a pin: its mean moves by +-5 bytes with the
   scene, so it is left out.
"""
from __future__ import annotations

import argparse
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import add, camera_initialize, cross, dot, mul, reflect, smul, sub, unit  # noqa: E402

W, H = 1280, 720
SPP = 64
RAY_RADIUS = 0.5     # tracer.go:138 (README's example uses the default)
LENS_RADIUS = 0.05   # Aperture / 2 (camera.go:85), RichSceneCamera's 0.1
MARGIN = 0.02
N_AA, N_LENS, FACTOR = 16, 8, 1.1
ENLARGED = 1.05
LAMBERT_Y = 1.5
RESTATEMENT_SEEDS = (1, 2, 3, 4)
GROUND = ((0.0, -1000.0, 0.0), 1000.0)
GLASS, LAMBERT, METAL = ((0.0, 1.0, 0.0), 1.0), ((-4.0, 1.0, 0.0), 1.0), ((4.0, 1.0, 0.0), 1.0)
ALBEDO = (0.7, 0.6, 0.5)                               # objects.go:171
BG = ((1.0, 1.0, 1.0), (0.4, 0.65, 1.0))               # DefaultBackground, objects.go:106-110
# tests/example_png.py:lambert_scene_spread(): oracle cap means over scene seeds 2..9, RNG seed 2
LAMBERT_SCENE_SEEDS = tuple(range(2, 10))
LAMBERT_SCENE_SPREAD = (0.16045519, 0.06742532, 0.09871977)


@functools.lru_cache(maxsize=None)
def rich_camera():
    """RichSceneCamera (camera.go:144-154) at 1280x720: position, pixel00, pixel_x,
    pixel_y from make_golden.camera_initialize, and the defocus disc vectors
    restated with the same operations (camera.go:79-87)."""
    cam = camera_initialize((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 10.0, W, H)
    f64 = np.float64
    pos = tuple(f64(c) for c in (13, 2, 3))
    w = unit(sub(pos, (f64(0), f64(0), f64(0))))
    u = unit(cross((f64(0), f64(1), f64(0)), w))
    v = cross(w, u)
    r = f64(0.1) / f64(2)
    return dict(pos=pos, p00=tuple(cam[3:6]), px=tuple(cam[6:9]), py=tuple(cam[9:12]), du=smul(u, r), dv=smul(v, r))


def srgb255(linear):
    """255 x the sRGB transfer of a linear colour (LinearToSrgb's value before it rounds)."""
    c = np.clip(np.asarray(linear, dtype=np.float64), 0.0, 1.0)
    return 255.0 * np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(c, 1 / 2.4) - 0.055)


def camera_ray(xs, ys, aa_offsets=None, lens_offsets=None):
    """Camera.GetRay (camera.go:113-142) for pixel coordinates xs, ys (float arrays),
    anti-aliasing offsets [..., 2] in pixels (None: the pixel centre) and lens
    offsets [..., 2] on the unit disc already scaled, i.e. InDisc(1.0)'s pair
    (None: Aperture == 0, the branch is not taken). Returns (origin, direction)."""
    c = rich_camera()
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    ox, oy = (0.0, 0.0) if aa_offsets is None else (np.asarray(aa_offsets)[..., 0], np.asarray(aa_offsets)[..., 1])
    sample = add(add(c["p00"], smul(c["px"], xs + ox)), smul(c["py"], ys + oy))
    dirn = sub(sample, c["pos"])
    org = tuple(np.full(np.shape(dirn[0]), p) for p in c["pos"])
    if lens_offsets is not None:
        dx, dy = np.asarray(lens_offsets)[..., 0], np.asarray(lens_offsets)[..., 1]
        offset = add(smul(c["du"], dx), smul(c["dv"], dy))
        focus_point = add(c["pos"], smul(dirn, np.float64(10.0) / np.float64(10.0)))
        org = add(c["pos"], offset)
        dirn = sub(focus_point, org)
        org = tuple(np.broadcast_to(o, np.shape(dirn[0])) for o in org)
    return org, dirn


def sphere_root(org, dirn, sphere, radius=None):
    """Sphere.Hit's root in (1e-6, inf) (objects.go:81-97), inf where it misses."""
    center, r = sphere
    r = r if radius is None else radius
    oc = sub(tuple(np.float64(v) for v in center), org)
    a = dot(dirn, dirn)
    h = dot(dirn, oc)
    cc = dot(oc, oc) - r * r
    disc = h * h - a * cc
    ok = disc >= 0
    sq = np.sqrt(np.where(ok, disc, 0.0))
    r1, r2 = (h - sq) / a, (h + sq) / a
    root = np.where(r1 > 1e-6, r1, np.where(r2 > 1e-6, r2, np.inf))
    return np.where(ok, root, np.inf)


def hit_record(org, dirn, sphere, root):
    """Point and face normal of Sphere.Hit (objects.go:98-101, 19-26)."""
    center, r = sphere
    point = add(org, smul(dirn, root))
    outward = sub(point, tuple(np.float64(v) for v in center))
    outward = (outward[0] / r, outward[1] / r, outward[2] / r)
    front = dot(dirn, outward) < 0
    return point, tuple(np.where(front, outward[k], -outward[k]) for k in range(3))


def metal_bounce(xs, ys, aa_offsets=None, lens_offsets=None):
    """One sample through the (4,1,0) mirror: (root, point, reflected) of the camera ray."""
    org, dirn = camera_ray(xs, ys, aa_offsets, lens_offsets)
    with np.errstate(invalid="ignore", over="ignore"):
        root = sphere_root(org, dirn, METAL)
        safe = np.where(np.isfinite(root), root, 1.0)
        point, normal = hit_record(org, dirn, METAL, safe)
        reflected = reflect(unit(dirn), normal)  # Metal.Scatter, Fuzz == 0 (materials.go:29-33)
    return org, dirn, root, point, normal, reflected


def analytic_color(xs, ys, aa_offsets=None, lens_offsets=None):
    """The linear colour of one sample of a METAL MASK pixel: hit -> reflect -> sky x
    albedo, vectorised, evaluation order as the Go source (see render_rngfree in
    make_golden.py). Meaningless where the ray is not a passing ray. [..., 3]."""
    _, _, _, _, _, reflected = metal_bounce(xs, ys, aa_offsets, lens_offsets)
    u = unit(reflected)  # AmbientLight.Hit (objects.go:68-73)
    t = 0.5 * (u[1] + 1.0)
    sky = add(smul(tuple(np.float64(v) for v in BG[0]), 1.0 - t), smul(tuple(np.float64(v) for v in BG[1]), t))
    col = mul(tuple(np.float64(v) for v in ALBEDO), sky)  # Mul(attenuation, RayColor(scattered))
    return np.stack(np.broadcast_arrays(*col), axis=-1)


def footprint_offsets():
    """[(aa_offset, lens_offset)]: the centre, then each boundary circle against the
    other's centre and against the other's boundary points, at FACTOR x the radii."""
    aa = [(FACTOR * RAY_RADIUS * np.cos(a), FACTOR * RAY_RADIUS * np.sin(a))
          for a in np.arange(N_AA) * (2 * np.pi / N_AA)]
    lens = [(FACTOR * np.cos(a), FACTOR * np.sin(a)) for a in np.arange(N_LENS) * (2 * np.pi / N_LENS)]
    zero = (0.0, 0.0)
    return ([(zero, zero)] + [(a, zero) for a in aa] + [(zero, le) for le in lens]
            + [(a, le) for a in aa for le in lens])


def _metal_passes(xs, ys, aa, lens):
    org, dirn, root, point, normal, reflected = metal_bounce(xs, ys, aa, lens)
    ok = np.isfinite(root)
    for other in (GROUND, GLASS, LAMBERT):  # the mirror is the closest of the fixed spheres
        ok &= sphere_root(org, dirn, other) > root
    ok &= point[1] > 1.0 + MARGIN
    ok &= dot(reflected, normal) > 0
    ok &= unit(reflected)[1] > MARGIN
    for other in (GLASS, LAMBERT):
        ok &= ~np.isfinite(sphere_root(point, reflected, other, ENLARGED))
    return ok


def _lambert_passes(xs, ys, aa, lens):
    org, dirn = camera_ray(xs, ys, aa, lens)
    root = sphere_root(org, dirn, LAMBERT)
    ok = np.isfinite(root)
    point, _ = hit_record(org, dirn, LAMBERT, np.where(ok, root, 1.0))
    ok &= point[1] > LAMBERT_Y
    ok &= sphere_root(org, dirn, GROUND) > root
    for other in (GLASS, METAL):
        ok &= ~np.isfinite(sphere_root(org, dirn, other, ENLARGED))
    return ok


def _footprint_mask(passes):
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        idx = np.nonzero(passes(xs, ys, None, None))[0]  # the pinhole centre ray first: it thins the image out
        for aa, lens in footprint_offsets():
            idx = idx[passes(xs[idx], ys[idx], np.array(aa), np.array(lens))]
    mask = np.zeros(H * W, dtype=bool)
    mask[idx] = True
    return mask.reshape(H, W)


def metal_mask():
    return _footprint_mask(_metal_passes)


def lambert_mask():
    return _footprint_mask(_lambert_passes)


def footprint_spread(mask):
    """Per pixel of `mask` (row-major) and channel: max - min of the continuous sRGB
    value (srgb255) over the footprint samples. [N, 3] bytes."""
    ys, xs = np.nonzero(mask)
    lo = hi = srgb255(analytic_color(xs, ys))
    for aa, lens in footprint_offsets():
        e = srgb255(analytic_color(xs, ys, np.array(aa), np.array(lens)))
        lo, hi = np.minimum(lo, e), np.maximum(hi, e)
    return hi - lo


def in_disc(rng, n, radius):
    """A uniform point of the disc, n times (rand.InDisc's distribution, not its stream)."""
    r, th = radius * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=-1)


def restatement(mask, seed):
    """RenderLines (tracer.go:120-155) at r = 64 on the mask's pixels with numpy's own
    jitter streams: the linear mean colour [N, 3]."""
    ys, xs = np.nonzero(mask)
    rng = np.random.default_rng(seed)
    total = np.zeros((len(xs), 3))
    for _ in range(SPP):
        aa = in_disc(rng, len(xs), RAY_RADIUS)
        lens = in_disc(rng, len(xs), 1.0)
        total = total + analytic_color(xs, ys, aa, lens)
    return total * (1.0 / SPP)


def quadrants(mask, xmid, ymid):
    """Whole mask + its four quadrants about (xmid, ymid), as boolean selections of the mask's pixels."""
    ys, xs = np.nonzero(mask)
    left, top = xs < xmid, ys < ymid
    return [np.ones(len(xs), dtype=bool)] + [(left == a) & (top == b) for a in (True, False) for b in (True, False)]


def bias(cont, rgb, regions):
    """max over regions and R, G of |mean(continuous sRGB - PNG byte)|."""
    d = cont[:, :2] - rgb[:, :2]
    return max(float(np.abs(d[r].mean(0)).max()) for r in regions)


def png_standard_error(mask, img):
    """SE of the PNG's own mean byte over the mask, per channel: the noise variance of
    one pixel is half the variance of horizontally adjacent masked pixels' differences."""
    pair = mask[:, 1:] & mask[:, :-1]
    diff = img[:, 1:].astype(np.float64)[pair] - img[:, :-1].astype(np.float64)[pair]
    return np.sqrt(diff.var(0) / 2.0 / mask.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    from PIL import Image

    img = np.asarray(Image.open(os.path.join(args.reference, "example.png")).convert("RGB"))
    assert img.shape == (H, W, 3)

    mask = metal_mask()
    rgb = img[mask]
    ys, xs = np.nonzero(mask)
    xmid, ymid = int(np.median(xs)), int(np.median(ys))
    regions = quadrants(mask, xmid, ymid)
    spread = footprint_spread(mask)
    misses, biases = [], []
    for seed in RESTATEMENT_SEEDS:
        cont = srgb255(restatement(mask, seed))
        d = np.floor(cont + 0.5).astype(int) - rgb
        misses.append(int((d != 0).sum()))
        biases.append(bias(cont, rgb, regions))
        print("restatement seed", seed, "max", int(np.abs(d).max()), "differing channels", misses[-1], "exact pixels",
              float((d == 0).all(1).mean()), "bias", biases[-1])
    np.savez_compressed(os.path.join(HERE, "example_metal_cap.npz"), mask=np.packbits(mask), shape=np.array([H, W]),
                        rgb=rgb, quadrant_split=np.array([xmid, ymid]), restatement_misses=np.array(misses),
                        restatement_bias=np.array(biases),
                        note="example.png pixels whose whole camera footprint reflects off the (4,1,0) mirror into "
                             "the sky in any RichScene (tests/golden/make_example_pins.py)")
    rows = np.nonzero(mask.any(1))[0]
    print("example_metal_cap", int(mask.sum()), "pixels, rows", int(rows.min()), "..", int(rows.max()),
          "mean spread", spread[:, :2].mean(), "blue", np.unique(rgb[:, 2]))

    lmask = lambert_mask()
    lrgb = img[lmask]
    se = png_standard_error(lmask, img)
    np.savez_compressed(os.path.join(HERE, "example_lambert_cap.npz"), mask=np.packbits(lmask),
                        shape=np.array([H, W]), rgb=lrgb, y_threshold=LAMBERT_Y, standard_error=se,
                        scene_spread=np.array(LAMBERT_SCENE_SPREAD), scene_seeds=np.array(LAMBERT_SCENE_SEEDS),
                        note="example.png pixels whose whole camera footprint lands on the upper cap of the "
                             "(-4,1,0) Lambertian sphere (tests/golden/make_example_pins.py)")
    rows = np.nonzero(lmask.any(1))[0]
    print("example_lambert_cap", int(lmask.sum()), "pixels, rows", int(rows.min()), "..", int(rows.max()), "mean",
          lrgb.mean(0), "SE", se)


if __name__ == "__main__":
    main()
