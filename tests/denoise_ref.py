"""include/tray_denoise.h restated in numpy, tap by tap, from the header's text
(not from the kernel): shifted slices in the contract's tap order. numpy's
element-wise + - * / on float64 are the correctly rounded IEEE operations and
never contract into an FMA, so the expectation against the device is equality
of bit patterns.
"""
import numpy as np

H5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)  # h[dy], h[dx] for -2..2
FLOOR = 2.0 ** -10
DEMODULATE = 1


def edge_stop(x):
    """b(x) = (1 - x) * (1 - x) if x < 1, else 0 (a NaN x gives 0)."""
    y = 1.0 - x
    return np.where(x < 1.0, y * y, 0.0)


def floor_albedo(a):
    """m(a) = a if a > 2^-10, else 2^-10 (also for NaN)."""
    return np.where(a > FLOOR, a, FLOOR)


def denoise(colour, albedo=None, normal=None, depth=None, iterations=5, flags=DEMODULATE, sigma_color=0.5,
            sigma_normal=0.5, sigma_depth=0.0625):
    """The filter of include/tray_denoise.h on host arrays: colour (rows, width, 3),
    albedo / normal (rows, width, 3) or None, depth (rows, width) or None."""
    f8 = np.float64
    colour = np.asarray(colour, dtype=f8)
    rows, width = colour.shape[:2]
    with np.errstate(all="ignore"):
        q_n = f8(1.0) / (f8(sigma_normal) * f8(sigma_normal))
        q_z = f8(1.0) / (f8(sigma_depth) * f8(sigma_depth))
        if depth is not None:
            z = np.asarray(depth, dtype=f8)
            u = np.where(z > 0.0, f8(1.0) / np.where(z > 0.0, z, 1.0), 0.0)
        if normal is not None:
            n = np.asarray(normal, dtype=f8)
        if flags & DEMODULATE:
            m = floor_albedo(np.asarray(albedo, dtype=f8))
            c = colour / m
        else:
            c = colour.copy()
        sigma_c = f8(sigma_color)
        for i in range(iterations):
            s = 1 << i
            q_c = f8(1.0) / (sigma_c * sigma_c)
            acc = np.zeros((rows, width, 3))
            wsum = np.zeros((rows, width))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    # pixels p whose tap q = p + (ox, oy) lies inside the image
                    y0, y1 = max(0, -oy), min(rows, rows - oy)
                    x0, x1 = max(0, -ox), min(width, width - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    k = H5[dy + 2] * H5[dx + 2]
                    d = c[P] - c[Q]
                    x_c = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * q_c
                    w = k * edge_stop(x_c)
                    if normal is not None:
                        e = n[P] - n[Q]
                        x_n = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) * q_n
                        w = w * edge_stop(x_n)
                    if depth is not None:
                        t = (z[P] - z[Q]) * np.where(z[P] >= z[Q], u[P], u[Q])
                        x_z = (t * t) * q_z
                        w = w * edge_stop(x_z)
                    take = w > 0.0  # a tap whose w is not > 0 is skipped
                    cq = c[Q]
                    for ch in range(3):
                        acc[P + (ch,)] = np.where(take, acc[P + (ch,)] + w * cq[..., ch], acc[P + (ch,)])
                    wsum[P] = np.where(take, wsum[P] + w, wsum[P])
            have = wsum > 0.0
            safe = np.where(have, wsum, 1.0)
            c = np.where(have[..., None], acc / safe[..., None], c)
            sigma_c = sigma_c * f8(0.5)
        return c * m if flags & DEMODULATE else c
