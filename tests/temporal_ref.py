"""include/tray_temporal.h restated in numpy from the header's text (not from the kernel): the
centre rays, the projection into the previous camera, the taps and the fold. The centre rays'
hits (index, t) are an input: the oracle's Scene.Hit on the CPU, tray_scene_hit_async on the
device. numpy's element-wise + - * / on float64 are the correctly rounded IEEE operations and
never contract into an FMA, so the expectation against the device is equality of bit patterns.

A camera is the 21 doubles of tray_camera: position, pixel00, pixel_x, pixel_y (3 each), then
what the step does not read.
"""
import numpy as np

f8 = np.float64
MAX_HISTORY, DEPTH_TOLERANCE, SNAP = 32, 0.1, 2.0 ** -20  # tray_temporal_default_params


def _cam(camera):
    c = np.asarray(camera, dtype=f8).reshape(-1)
    return c[0:3], c[3:6], c[6:9], c[9:12]  # position, pixel00, pixel_x, pixel_y


def dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def centre_rays(camera, width, height):
    """Section 2a: (o (3,), d (height, width, 3))."""
    o, p00, pxv, pyv = _cam(camera)
    x = np.arange(width, dtype=f8)[None, :, None]
    y = np.arange(height, dtype=f8)[:, None, None]
    s = (p00 + pxv * x) + pyv * y
    return o.copy(), s - o


def oracle_hits(O, spheres, camera, width, height):
    """Scene.Hit(o, d, (1e-6, +inf)) of every centre ray by the oracle: (index int32, t float64)."""
    o, d = centre_rays(camera, width, height)
    index = np.full((height, width), -1, dtype=np.int32)
    t = np.full((height, width), np.inf)
    for y in range(height):
        for x in range(width):
            i, rec = O.scene_hit(spheres, o, d[y, x], 1e-6, np.inf)
            if i >= 0:
                index[y, x], t[y, x] = i, rec[6]
    return index, t


def project(camera, prev_camera, width, height, index, t):
    """Sections 2b and 2c: (z, u, v, in_range)."""
    o, d = centre_rays(camera, width, height)
    P, p00, pxv, pyv = _cam(prev_camera)
    with np.errstate(all="ignore"):
        hit = index >= 0
        Q = o + d * np.where(hit, t, 0.0)[..., None]
        e = np.where(hit[..., None], Q - P, d)
        n = cross(pxv, pyv)
        c0 = p00 - P
        z = dot(n, e) / dot(n, c0)
        g = e / z[..., None] - c0
        u = dot(g, pxv) / dot(pxv, pxv)
        v = dot(g, pyv) / dot(pyv, pyv)
        in_range = (z > 0) & (u > -1) & (u < f8(width)) & (v > -1) & (v < f8(height))
    return z, u, v, in_range


def snapped_mask(u, v, snap=SNAP):
    with np.errstate(all="ignore"):
        return (np.abs(u - np.floor(u + 0.5)) <= snap) & (np.abs(v - np.floor(v + 0.5)) <= snap)


def step(camera, prev_camera, frame, hits, history=None, max_history=MAX_HISTORY, depth_tolerance=DEPTH_TOLERANCE,
         snap=SNAP):
    """One step. hits: (index, t) of `camera`'s centre rays; history: None or a dict with colour,
    age, index, depth. Returns (state dict, (fresh, age_sum))."""
    frame = np.asarray(frame, dtype=f8)
    height, width = frame.shape[:2]
    index = np.asarray(hits[0], dtype=np.int32)
    t = np.where(index >= 0, np.asarray(hits[1], dtype=f8), np.inf)
    colour = frame.copy()
    age = np.ones((height, width), dtype=np.int32)
    if history is not None and prev_camera is not None and max_history > 1 and frame.size:
        z, u, v, in_range = project(camera, prev_camera, width, height, index, t)
        hc, ha = np.asarray(history["colour"], dtype=f8), np.asarray(history["age"], dtype=np.int32)
        hi, hd = np.asarray(history["index"], dtype=np.int32), np.asarray(history["depth"], dtype=f8)
        with np.errstate(all="ignore"):
            xr, yr = np.floor(u + 0.5), np.floor(v + 0.5)
            snapped = (np.abs(u - xr) <= snap) & (np.abs(v - yr) <= snap)
            x0, y0 = np.where(snapped, xr, np.floor(u)), np.where(snapped, yr, np.floor(v))
            a, b = u - x0, v - y0
            one, zero = np.ones_like(u), np.zeros_like(u)
            weights = [np.where(snapped, one, (1 - a) * (1 - b)), np.where(snapped, zero, a * (1 - b)),
                       np.where(snapped, zero, (1 - a) * b), np.where(snapped, zero, a * b)]
            bound = f8(depth_tolerance) * z
            W = np.zeros((height, width))
            H = np.zeros((height, width, 3))
            A = np.full((height, width), np.iinfo(np.int32).max, dtype=np.int32)
            for j, w in enumerate(weights):
                tx, ty = x0 + (j & 1), y0 + (j >> 1)
                inside = in_range & (w > 0) & (tx >= 0) & (tx < width) & (ty >= 0) & (ty < height)
                ix = np.where(inside, tx, 0).astype(np.int64)
                iy = np.where(inside, ty, 0).astype(np.int64)
                c = hc[iy, ix]
                take = (inside & (ha[iy, ix] >= 1) & (hi[iy, ix] == index) &
                        ((index < 0) | (np.abs(hd[iy, ix] - z) <= bound)) & ~np.isnan(c).any(axis=-1))
                W = np.where(take, W + w, W)
                H = np.where(take[..., None], H + w[..., None] * c, H)
                A = np.where(take, np.minimum(A, ha[iy, ix]), A)
            use = in_range & (W > 0)
            h = H / np.where(use, W, 1.0)[..., None]
            k = np.minimum(A, np.int32(max_history - 1)) + np.int32(1)
            folded = h + (frame - h) / np.where(use, k, 1).astype(f8)[..., None]
        colour = np.where(use[..., None], folded, frame)
        age = np.where(use, k, 1).astype(np.int32)
    state = dict(colour=colour, age=age, index=index.copy(), depth=t.copy())
    return state, (int((age == 1).sum()) if history is None or max_history <= 1 else int((~use).sum()),
                   int(age.astype(np.int64).sum()))


def orbit_setup(setup, degrees):
    """A camera setup (13 doubles: position, look_at, up, ...) with the position turned about look_at
    around the up axis by `degrees`: tray_amd.ray.Orbit on the oracle's arrays."""
    from tray_amd import ray

    s = np.asarray(setup, dtype=f8).copy()
    s[0:3] = ray.orbit_position(tuple(s[0:3]), tuple(s[3:6]), tuple(s[6:9]), degrees)
    return s
