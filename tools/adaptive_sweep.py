"""The sweep behind tray_adaptive_default_params, on the CPU: oracle passes of
the book cover (r = 16, passes 0 .. max_passes + batch - 2) and an independent high-sample
target (pass 1 of r = 4096: sample words 4096 .. 8191), folded and selected by the numpy
restatements tests/progressive_ref.py and tests/adaptive_ref.py.

A pixel's pass k does not depend on which pixels are rendered with it, so the adaptive state of
a pixel with count c is the uniform state after c passes: the sweep renders the uniform passes
once per size and plays Tracer.RenderAdaptive's loop on them for min_passes in {2, 4, 8} x
dilate in {0, 1}, against Tracer.RenderProgressive's loop (uniform batches until no pixel is
unconverged) at the same tolerance. Prints one JSON line per setting and size: the MSE against
the target and the pixel-passes of both, and their ratios. Early stopping on a noisy variance
estimate biases dark, rare-event pixels: that is what the MSE ratio at a small min_passes shows.

    python tools/adaptive_sweep.py [--sizes 32x18,48x27,64x36] [--max-passes 32] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> None:
    import adaptive_ref as A
    import denoise_frames as F
    import progressive_ref as P
    from conftest import DEFAULT_BG
    from oracle import oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32x18,48x27,64x36")
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--target", type=int, default=4096)
    ap.add_argument("--max-passes", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--tolerance", type=float, default=0.05)
    ap.add_argument("--out")
    a = ap.parse_args()
    workers = min(16, os.cpu_count() or 1)
    spheres = O.rich_scene(F.SEED)
    top = a.max_passes + a.batch - 1
    lines = []
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        cam = F.camera_state(O, w, h)

        def render(r, pass_):
            return O.render(spheres, DEFAULT_BG, cam, w, h, r, F.DEPTH, F.RADIUS, F.SEED, workers=workers,
                            segments=False, pass_=pass_)

        target = render(a.target, 1)
        frames = np.stack([render(a.r, k) for k in range(top)])
        states, s = {}, None
        for c in range(1, top + 1):  # the uniform state after c passes
            s = P.fold(s, frames[c - 1:c])
            states[c] = s
        mse = lambda img: float(np.mean((img - target) ** 2))  # noqa: E731
        # RenderProgressive: batches until nothing is unconverged, or max_passes
        n = 0
        while n < a.max_passes:
            n = min(n + a.batch, a.max_passes)
            if n >= 2 and P.metric(states[n][0], states[n][1], n, a.tolerance)[0] == 0:
                break
        uniform = dict(passes=n, pixel_passes=n * w * h, mse=mse(states[n][0]))
        for min_passes in (2, 4, 8):
            for dilate in (0, 1):
                counts = np.full((h, w), min_passes, dtype=np.int32)
                while True:
                    mean, m2 = np.empty((h, w, 3)), np.empty((h, w, 3))
                    for c in np.unique(counts):
                        mean[counts == c], m2[counts == c] = states[c][0][counts == c], states[c][1][counts == c]
                    sel = A.select(mean, m2, counts, a.tolerance, P.FLOOR, min_passes, a.max_passes, dilate)
                    if sel["n_active"] == 0:
                        break
                    counts[sel["active"]] += a.batch
                rec = dict(size=size, r=a.r, tolerance=a.tolerance, max_passes=a.max_passes, batch=a.batch,
                           target=a.target, min_passes=min_passes, dilate=dilate, mse=mse(mean),
                           pixel_passes=int(counts.sum()), unconverged=sel["unconverged"], uniform=uniform,
                           mse_ratio=mse(mean) / uniform["mse"],
                           pixel_pass_ratio=int(counts.sum()) / uniform["pixel_passes"])
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    for min_passes in (2, 4, 8):
        for dilate in (0, 1):
            mine = [r for r in lines if (r["min_passes"], r["dilate"]) == (min_passes, dilate)]
            ratios = [r["mse_ratio"] for r in mine]
            print(json.dumps(dict(summary=dict(min_passes=min_passes, dilate=dilate, worst_mse_ratio=max(ratios),
                                               spread=max(ratios) - min(ratios),
                                               mean_pixel_pass_ratio=float(np.mean([r["pixel_pass_ratio"]
                                                                                    for r in mine]))))))
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
