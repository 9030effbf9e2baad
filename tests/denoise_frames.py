"""Book-cover frames from the CPU oracle for the denoiser's tests and sigma sweep
(tools/denoise_sweep.py): a noisy frame, a target of many more samples, and the
guides of include/tray_aov.h reduced from the oracle's own rays and hit records
(first-hit albedo, normal and depth means over the frame's samples)."""
import numpy as np

from conftest import DEFAULT_BG, RICH_SETUP

SEED, DEPTH, RADIUS = 2, 50, 0.5


def camera_state(O, w, h):
    return np.asarray(O.camera_initialize(RICH_SETUP, w, h)[1], dtype=np.float64)


def oracle_guides(O, spheres, cam, w, h, r, seed=SEED, pass_=0, rows=None):
    """albedo (h, w, 3), normal (h, w, 3), depth (h, w) as tray_render_aov_async defines them;
    rows: only these image rows, in this order."""
    from oracle.oracle import SPHERE_DTYPE

    far = np.zeros(1, dtype=SPHERE_DTYPE)  # a scene no ray reaches: RayColor at depth 1 is AmbientLight.Hit
    far["center"], far["radius"], far["material"], far["albedo"] = (5e8, -7e8, 3e8), 1.0, 1, 0.5
    rows = list(range(h)) if rows is None else list(rows)
    albedo, normal, depth = np.zeros((len(rows), w, 3)), np.zeros((len(rows), w, 3)), np.zeros((len(rows), w))
    inv = 1.0 / r
    for j, y in enumerate(rows):
        for x in range(w):
            a, n, z, count = np.zeros(3), np.zeros(3), 0.0, 0
            for s in range(r):
                pixel, word = y * w + x, pass_ * r + s
                off = O.in_disc(seed, pixel, word, 0, RADIUS) if r > 1 else (0.0, 0.0)
                o, d = O.get_ray(cam, float(x), float(y), off[0], off[1], seed, pixel, word)
                idx, rec = O.scene_hit(spheres, o, d, 1e-6, np.inf)
                if idx >= 0:
                    a = a + (1.0 if spheres["material"][idx] == 3 else spheres["albedo"][idx])
                    n = n + rec[3:6]
                    z = z + rec[6] * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                    count += 1
                else:
                    a = a + O.ray_color(far, DEFAULT_BG, np.zeros(3), d, 1)[0]
            albedo[j, x], normal[j, x] = a * inv, n * inv
            depth[j, x] = z / count if count else 0.0
    return albedo, normal, depth


def book_cover(O, w, h, r_noisy, r_target, workers=4):
    """(noisy, target, albedo, normal, depth) of the w x h book cover (seed 2, d = 50): the noisy
    frame and its guides at pass 0, the target at pass 1, so its samples are independent."""
    spheres = O.rich_scene(SEED)
    cam = camera_state(O, w, h)
    noisy = O.render(spheres, DEFAULT_BG, cam, w, h, r_noisy, DEPTH, RADIUS, SEED, workers=workers, segments=False)
    target = O.render(spheres, DEFAULT_BG, cam, w, h, r_target, DEPTH, RADIUS, SEED, workers=workers,
                      segments=False, pass_=1)
    return (noisy, target) + oracle_guides(O, spheres, cam, w, h, r_noisy)
