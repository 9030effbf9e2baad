"""include/tray_progressive.h restated in numpy from the header's text (not from the
kernels): Welford's fold frame by frame, the variance of the mean and the
convergence metric, and the variance-guided a-trous filter as shifted slices in
the contract's tap order. numpy's element-wise + - * / on float64 are the
correctly rounded IEEE operations and never contract into an FMA, so the
expectation against the device is equality of bit patterns.
"""
import numpy as np

from denoise_ref import DEMODULATE, H5, edge_stop, floor_albedo

H3 = (0.25, 0.5, 0.25)  # h3[dy], h3[dx] for -1..1
TOLERANCE, FLOOR = 0.05, 2.0 ** -10  # tray_accum_metric_default_params
f8 = np.float64


# ------------------------------------------------------------ 1. accumulator --
def fold(state, frames):
    """state: None (count 0) or (mean, m2, count); frames: (k, ...) float64. Returns the new
    (mean, m2, count); the inputs are not modified."""
    frames = np.asarray(frames, dtype=f8)
    if state is None or state[2] == 0:
        mean, m2, n = np.zeros(frames.shape[1:]), np.zeros(frames.shape[1:]), 0
    else:
        mean, m2, n = state[0].copy(), state[1].copy(), int(state[2])
    with np.errstate(all="ignore"):
        for x in frames:
            n += 1
            t = x - mean
            mean = mean + t / f8(n)
            m2 = m2 + t * (x - mean)
    return mean, m2, n


# ------------------------------------------------ 2. variance and the metric --
def variance_of_mean(m2, n):
    if n < 2:
        return np.full(np.shape(m2), np.inf)
    with np.errstate(all="ignore"):
        return np.asarray(m2, dtype=f8) / (f8(n) * f8(n - 1))


def metric(mean, m2, n, tolerance=TOLERANCE, floor=FLOOR):
    """(unconverged, max_ratio, converged mask) for a (..., 3) state of n frames."""
    var = variance_of_mean(m2, n)
    with np.errstate(all="ignore"):
        T = f8(tolerance) * f8(tolerance)
        v = (var[..., 0] + var[..., 1]) + var[..., 2]
        e = (mean[..., 0] * mean[..., 0] + mean[..., 1] * mean[..., 1]) + mean[..., 2] * mean[..., 2]
        m = np.where(e > floor, e, f8(floor))
        q = v / m
        converged = (v <= T * m) if n >= 2 else np.zeros(v.shape, dtype=bool)
        counted = q[q >= 0.0]
    return int((~converged).sum()), float(counted.max()) if counted.size else 0.0, converged


# ----------------------------------------------- 3. variance-guided filter --
def _shift(rows, width, oy, ox):
    """Slices P, Q with Q = P + (ox, oy) inside the image, or None."""
    y0, y1 = max(0, -oy), min(rows, rows - oy)
    x0, x1 = max(0, -ox), min(width, width - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def prefilter(v, s):
    """g_i: the 3 x 3 binomial mean of v at spacing s over the in-image points."""
    rows, width = v.shape
    G, B = np.zeros((rows, width)), np.zeros((rows, width))
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            PQ = _shift(rows, width, s * dy, s * dx)
            if PQ is None:
                continue
            P, Q = PQ
            k3 = H3[dy + 1] * H3[dx + 1]
            G[P] = G[P] + k3 * v[Q]
            B[P] = B[P] + k3
    return G / B


def denoise_variance(colour, variance, albedo=None, normal=None, depth=None, iterations=5, flags=DEMODULATE,
                     sigma_variance=3.0, sigma_normal=0.5, sigma_depth=0.0625, epsilon=1e-12):
    """Section 3 on host arrays: colour, variance (rows, width, 3); albedo / normal (rows, width, 3)
    or None, depth (rows, width) or None. Returns (out, v_iterations)."""
    colour = np.asarray(colour, dtype=f8)
    variance = np.asarray(variance, dtype=f8)
    rows, width = colour.shape[:2]
    with np.errstate(all="ignore"):
        q_n = f8(1.0) / (f8(sigma_normal) * f8(sigma_normal))
        q_z = f8(1.0) / (f8(sigma_depth) * f8(sigma_depth))
        S, eps = f8(sigma_variance) * f8(sigma_variance), f8(epsilon)
        if depth is not None:
            z = np.asarray(depth, dtype=f8)
            u = np.where(z > 0.0, f8(1.0) / np.where(z > 0.0, z, 1.0), 0.0)
        if normal is not None:
            n = np.asarray(normal, dtype=f8)
        if flags & DEMODULATE:
            m = floor_albedo(np.asarray(albedo, dtype=f8))
            c = colour / m
            vm = variance / (m * m)
            v = (vm[..., 0] + vm[..., 1]) + vm[..., 2]
        else:
            c = colour.copy()
            v = (variance[..., 0] + variance[..., 1]) + variance[..., 2]
        for i in range(iterations):
            s = 1 << i
            g = prefilter(v, s)
            r = f8(1.0) / np.where(g > 0.0, S * g + eps, eps)
            acc = np.zeros((rows, width, 3))
            wsum = np.zeros((rows, width))
            vacc = np.zeros((rows, width))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    PQ = _shift(rows, width, s * dy, s * dx)
                    if PQ is None:
                        continue
                    P, Q = PQ
                    k = H5[dy + 2] * H5[dx + 2]
                    d = c[P] - c[Q]
                    x_c = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * r[P]
                    w = k * edge_stop(x_c)
                    if normal is not None:
                        e = n[P] - n[Q]
                        x_n = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) * q_n
                        w = w * edge_stop(x_n)
                    if depth is not None:
                        t = (z[P] - z[Q]) * np.where(z[P] >= z[Q], u[P], u[Q])
                        x_z = (t * t) * q_z
                        w = w * edge_stop(x_z)
                    take = w > 0.0
                    cq = c[Q]
                    for ch in range(3):
                        acc[P + (ch,)] = np.where(take, acc[P + (ch,)] + w * cq[..., ch], acc[P + (ch,)])
                    wsum[P] = np.where(take, wsum[P] + w, wsum[P])
                    vacc[P] = np.where(take, vacc[P] + (w * w) * v[Q], vacc[P])
            have = wsum > 0.0
            safe = np.where(have, wsum, 1.0)
            c = np.where(have[..., None], acc / safe[..., None], c)
            v = np.where(have, vacc / (safe * safe), v)
        return (c * m if flags & DEMODULATE else c), v
