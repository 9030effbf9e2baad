"""include/tray_temporal_variance.h restated in numpy from the header's text (not from the kernel):
tray_temporal.h's step (the projection of tests/temporal_ref.py; the taps and the fold written out
again here, because the gather of M2 runs over the same taken taps) with the M2 gather, the cap's
scaling, Welford's fold and the variance of the mean; the variance of listed pixels; and the refill
chain of section 4 on top of tests/adaptive_ref.py. numpy's element-wise + - * / on float64 are the
correctly rounded IEEE operations and never contract into an FMA, so the expectation against the
device is equality of bit patterns.
"""
import numpy as np

import adaptive_ref
import temporal_ref as T

f8 = np.float64
MAX_HISTORY, DEPTH_TOLERANCE, SNAP = T.MAX_HISTORY, T.DEPTH_TOLERANCE, T.SNAP
REFILL_TOLERANCE = 1e150  # finite with a finite square: only the count decides (section 4)


def variance_of(m2, age):
    """Section 2e: m2 / ((double)k * (double)(k - 1)) per element, +inf where k < 2."""
    m2 = np.asarray(m2, dtype=f8)
    k = np.asarray(age, dtype=np.int32)
    kd = np.where(k < 2, 2, k).astype(f8)
    with np.errstate(all="ignore"):
        v = m2 / (kd * (kd - 1.0))[..., None]
    return np.where((k < 2)[..., None], np.inf, v)


def step(camera, prev_camera, frame, hits, history=None, max_history=MAX_HISTORY, depth_tolerance=DEPTH_TOLERANCE,
         snap=SNAP):
    """One step. hits: (index, t) of `camera`'s centre rays; history: None or a dict with colour, m2,
    age, index, depth. Returns (state dict with m2, variance, (fresh, age_sum))."""
    frame = np.asarray(frame, dtype=f8)
    height, width = frame.shape[:2]
    index = np.asarray(hits[0], dtype=np.int32)
    t = np.where(index >= 0, np.asarray(hits[1], dtype=f8), np.inf)
    colour = frame.copy()
    m2 = np.zeros_like(frame)
    age = np.ones((height, width), dtype=np.int32)
    use = np.zeros((height, width), dtype=bool)
    if history is not None and prev_camera is not None and max_history > 1 and frame.size:
        z, u, v, in_range = T.project(camera, prev_camera, width, height, index, t)
        hc, hm = np.asarray(history["colour"], dtype=f8), np.asarray(history["m2"], dtype=f8)
        ha = np.asarray(history["age"], dtype=np.int32)
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
            M = np.zeros((height, width, 3))
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
                M = np.where(take[..., None], M + w[..., None] * hm[iy, ix], M)  # 2a: the same taps, the same order
                A = np.where(take, np.minimum(A, ha[iy, ix]), A)
            use = in_range & (W > 0)
            Ws = np.where(use, W, 1.0)[..., None]
            h = H / Ws
            m = M / Ws
            k = np.where(use, np.minimum(A, np.int32(max_history - 1)) + np.int32(1), 2).astype(np.int32)
            n0 = k - 1
            As = np.where(use, A, 2).astype(np.int64)
            scale = (n0 - 1).astype(f8) / (As - 1).astype(f8)  # 2b: one division ...
            m = np.where((As > n0)[..., None], m * scale[..., None], m)  # ... then one multiplication per channel
            tt = frame - h
            folded = h + tt / k.astype(f8)[..., None]  # tray_temporal.h's expression
            m2_folded = m + tt * (frame - folded)  # 2c: Welford's update with the new colour
        colour = np.where(use[..., None], folded, frame)
        m2 = np.where(use[..., None], m2_folded, 0.0)
        age = np.where(use, k, 1).astype(np.int32)
    state = dict(colour=colour, m2=m2, age=age, index=index.copy(), depth=t.copy())
    record = (int((~use).sum()), int(age.astype(np.int64).sum()))
    return state, variance_of(m2, age), record


def list_variance(state, pixels, variance):
    """Section 3: `variance` (height x width x 3) with formula 2e written for the listed pixels
    (None: every pixel); an entry >= height x width is skipped; the rest keeps its values."""
    full = variance_of(state["m2"], state["age"])
    if pixels is None:
        return full
    out = np.array(variance, dtype=f8, copy=True)
    px = state["age"].size
    flat, src = out.reshape(px, 3), full.reshape(px, 3)
    for p in np.asarray(pixels, dtype=np.int64):
        if 0 <= p < px:
            flat[p] = src[p]
    return out


def refill_list(state, refill, max_history, dilate=1, tolerance=REFILL_TOLERANCE):
    """Section 4's selection on the state viewed as an adaptive state: adaptive_ref.select with
    min_passes = 1 + refill and max_passes = max_history. Returns adaptive_ref.select's dict
    (pixels: the ascending list)."""
    return adaptive_ref.select(state["colour"], state["m2"], state["age"], tolerance=tolerance,
                               min_passes=1 + refill, max_passes=max_history, dilate=dilate)


def refill_fold(state, pixels, values):
    """Section 4's fold: adaptive_ref.fold of `values` (passes x n x 3) into colour, m2 and age of the
    listed pixels; a new state dict (index and depth are the step's)."""
    mean, m2, count = adaptive_ref.fold_sparse(state["colour"], state["m2"], state["age"], pixels, values)
    return dict(colour=mean, m2=m2, age=count.astype(np.int32), index=state["index"], depth=state["depth"])
