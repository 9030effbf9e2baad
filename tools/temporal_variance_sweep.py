"""The sweep behind the refill default and the calibration of the carried M2
(include/tray_temporal_variance.h), on the CPU: the oracle renders the frames and traces
the centre rays, tests/temporal_variance_ref.py does the steps and the refill chain.

An 8-frame orbit of the book cover at r = 4 and three small sizes, with R = 0, 1, 3, 7 refill passes per
frame for the pixels that hold fewer than 1 + R frames and their neighbours. Per size and R: the MSE
of the last accumulated frame against an independent high-sample frame of the last camera relative to
that camera's single r = 4 frame, the MSE over the pixels that are fresh in the last frame of the run
without refill, and the pixel-passes spent. Calibration rows: the mean over pixels of (squared error
against the reference, summed over channels) / (predicted variance of the mean, summed over
channels), per age bucket, for the bilinear pixels of the orbit without refill and for the snapped
pixels of a still camera; near 1 means the carried M2 is honest. The reference's own noise adds
age x r / truth to it (8 x 4 / 512 = 0.06 at age 8).

    python tools/temporal_variance_sweep.py [--out profiles/temporal_variance_sweep.jsonl] [--truth 512]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import temporal_ref as R  # noqa: E402
import temporal_variance_ref as V  # noqa: E402
from oracle import oracle as O  # noqa: E402

RICH_SETUP = np.array([13, 2, 3, 0, 0, 0, 0, 1, 0, 20.0, 10.0, 10.0, 0.1])
BG = O.DEFAULT_BACKGROUND
SIZES = ((32, 18), (48, 27), (64, 36))
REFILLS = (0, 1, 3, 7)
BUCKETS = ((2, 3), (4, 7), (8, 1 << 30))


def run(spheres, cams, hits, w, h, refill, workers):
    """The sequence with `refill` passes per frame: (state, variance, snapped mask of the last step,
    pixel-passes, per-frame list lengths)."""
    state, spent, lists = None, 0, []
    stride = 1 + refill
    for k, cam in enumerate(cams):
        def frame(j):
            return O.render(spheres, BG, cam, w, h, 4, 50, 0.5, 2, workers=workers, segments=False,
                            pass_=k * stride + j)
        state, var, rec = V.step(cam, cams[k - 1] if k else None, frame(0), hits[k], state)
        spent += w * h
        if refill:
            pixels = V.refill_list(state, refill, V.MAX_HISTORY)["pixels"]
            lists.append(len(pixels))
            if len(pixels):
                values = np.stack([frame(1 + j).reshape(-1, 3)[pixels] for j in range(refill)])
                state = V.refill_fold(state, pixels, values)
                var = V.list_variance(state, pixels, var)
                spent += refill * len(pixels)
    if len(cams) > 1:
        z, u, v, ok = R.project(cams[-1], cams[-2], w, h, *hits[-1])
        snapped = ok & R.snapped_mask(u, v)
    else:
        snapped = np.ones((h, w), dtype=bool)
    return state, var, snapped, spent, lists


def calibration(state, var, truth, mask):
    """Rows of (bucket, pixels, mean of ratios, ratio of sums) over the pixels of `mask` with a finite,
    positive predicted variance."""
    err = ((state["colour"] - truth) ** 2).sum(axis=-1)
    pred = var.sum(axis=-1)
    rows = []
    for lo, hi in BUCKETS:
        m = mask & (state["age"] >= lo) & (state["age"] <= hi) & np.isfinite(pred) & (pred > 0)
        if m.any():
            rows.append(dict(age_from=lo, age_to=min(hi, int(state["age"].max())), pixels=int(m.sum()),
                             mean_ratio=float((err[m] / pred[m]).mean()),
                             median_ratio=float(np.median(err[m] / pred[m])),
                             ratio_of_sums=float(err[m].sum() / pred[m].sum())))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_variance_sweep.jsonl"))
    ap.add_argument("--step", type=float, default=1.0, help="degrees between frames")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--truth", type=int, default=512, help="rays per pixel of the reference frame")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args(argv)
    spheres = O.rich_scene(2)
    rows = []
    for w, h in SIZES:
        cams = [O.camera_initialize(R.orbit_setup(RICH_SETUP, k * a.step), w, h)[1] for k in range(a.frames)]
        hits = [R.oracle_hits(O, spheres, c, w, h) for c in cams]
        truth = O.render(spheres, BG, cams[-1], w, h, a.truth, 50, 0.5, 77, workers=a.workers, segments=False)
        single = O.render(spheres, BG, cams[-1], w, h, 4, 50, 0.5, 2, workers=a.workers, segments=False,
                          pass_=a.frames - 1)
        mse_single = float(((single - truth) ** 2).mean())
        fresh = None
        for refill in REFILLS:
            state, var, snapped, spent, lists = run(spheres, cams, hits, w, h, refill, a.workers)
            if refill == 0:
                fresh = state["age"] == 1
                fresh_mse0 = float(((state["colour"] - truth)[fresh] ** 2).mean()) if fresh.any() else None
                for kind, mask in (("bilinear", ~snapped), ("snapped", snapped)):
                    for c in calibration(state, var, truth, mask):
                        rows.append(dict(kind="calibration", taps=kind, camera="orbit", width=w, height=h, **c))
            mse = float(((state["colour"] - truth) ** 2).mean())
            fresh_mse = float(((state["colour"] - truth)[fresh] ** 2).mean()) if fresh.any() else None
            rows.append(dict(kind="refill", width=w, height=h, step=a.step, frames=a.frames, refill=refill, mse=mse,
                             mse_single=mse_single, ratio=mse / mse_single, fresh_pixels=int(fresh.sum()),
                             fresh_mse=fresh_mse,
                             fresh_ratio=(fresh_mse / fresh_mse0) if fresh_mse0 else None,
                             pixel_passes=spent, uniform_pixel_passes=w * h * a.frames, refilled=lists,
                             mean_age=float(state["age"].mean())))
        still = [cams[-1]] * a.frames
        state, var, snapped, _, _ = run(spheres, still, [hits[-1]] * a.frames, w, h, 0, a.workers)
        for c in calibration(state, var, truth, snapped):
            rows.append(dict(kind="calibration", taps="snapped", camera="still", width=w, height=h, **c))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("refill  " + "  ".join(f"{w}x{h}: ratio fresh passes" for w, h in SIZES))
    for refill in REFILLS:
        rs = [r for r in rows if r["kind"] == "refill" and r["refill"] == refill]
        print(f"{refill:6d}  " + "  ".join(
            f"{r['ratio']:.4f} {r['fresh_ratio'] if r['fresh_ratio'] is not None else float('nan'):.4f} "
            f"{r['pixel_passes'] / r['uniform_pixel_passes']:.3f}" for r in rs))
    for r in rows:
        if r["kind"] == "calibration":
            print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
