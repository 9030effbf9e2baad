"""include/tray_adaptive.h sections 3 and 4 restated in numpy from the header's text (not from
the kernels): Welford's fold with a count per pixel over a list of pixels, and the selection
step (per-pixel variance and metric, dilation, ascending compaction, the record). numpy's
element-wise + - * / on float64 are the correctly rounded IEEE operations and never contract
into an FMA, so the expectation against the device is equality of bit patterns.
"""
import numpy as np

from progressive_ref import FLOOR, TOLERANCE

f8 = np.float64
MIN_PASSES, MAX_PASSES, DILATE = 8, 64, 1  # tray_adaptive_default_params


def fold_sparse(mean, m2, count, pixels, values):
    """mean, m2: (rows, width, 3); count: (rows, width) int32; pixels: (n,) distinct compact indices;
    values: (k, n, 3). Returns new (mean, m2, count); the inputs are not modified. A pixel whose
    count is 0 starts from zero whatever its buffers hold; an entry outside the image is skipped."""
    mean, m2, count = np.array(mean, dtype=f8), np.array(m2, dtype=f8), np.array(count, dtype=np.int32)
    fm, f2, fc = mean.reshape(-1, 3), m2.reshape(-1, 3), count.reshape(-1)
    values = np.asarray(values, dtype=f8)
    with np.errstate(all="ignore"):
        for i, p in enumerate(np.asarray(pixels, dtype=np.int64)):
            if p >= fc.size:
                continue
            n = int(fc[p])
            m, s = (fm[p].copy(), f2[p].copy()) if n > 0 else (np.zeros(3), np.zeros(3))
            for k in range(values.shape[0]):
                x = values[k, i]
                n += 1
                t = x - m
                m = m + t / f8(n)
                s = s + t * (x - m)
            fm[p], f2[p], fc[p] = m, s, n
    return mean, m2, count


def variance(m2, count):
    """Per element m2 / ((double)n * (double)(n - 1)) with the pixel's own n; +inf where n < 2."""
    n = np.asarray(count, dtype=np.int64)[..., None]
    with np.errstate(all="ignore"):
        D = n.astype(f8) * (n - 1).astype(f8)
        return np.where(n >= 2, np.asarray(m2, dtype=f8) / np.where(n >= 2, D, 1.0), np.inf)


def select(mean, m2, count, tolerance=TOLERANCE, floor=FLOOR, min_passes=MIN_PASSES, max_passes=MAX_PASSES,
           dilate=DILATE):
    """Section 4. Returns a dict: variance (rows, width, 3), needs / wanted / active (rows, width) bool,
    pixels (the ascending active list, uint32), n_active, unconverged, max_ratio, pixel_passes."""
    mean = np.asarray(mean, dtype=f8)
    count = np.asarray(count, dtype=np.int32)
    rows, width = count.shape
    var = variance(m2, count)
    with np.errstate(all="ignore"):
        T = f8(tolerance) * f8(tolerance)
        v = (var[..., 0] + var[..., 1]) + var[..., 2]
        e = (mean[..., 0] * mean[..., 0] + mean[..., 1] * mean[..., 1]) + mean[..., 2] * mean[..., 2]
        m = np.where(e > floor, e, f8(floor))
        q = v / m
        needs = ~((count >= 2) & (count >= min_passes) & (v <= T * m))
        counted = q[q >= 0.0]
    wanted = needs.copy()
    if dilate:
        padded = np.zeros((rows + 2, width + 2), dtype=bool)  # outside the image: nothing needs
        padded[1:-1, 1:-1] = needs
        for dy in range(3):
            for dx in range(3):
                wanted |= padded[dy:dy + rows, dx:dx + width]
    active = wanted & (count < max_passes)
    return dict(variance=var, needs=needs, wanted=wanted, active=active,
                pixels=np.flatnonzero(active.reshape(-1)).astype(np.uint32), n_active=int(active.sum()),
                unconverged=int(needs.sum()), max_ratio=float(counted.max()) if counted.size else 0.0,
                pixel_passes=int(count.astype(np.int64).sum()))
