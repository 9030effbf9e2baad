"""The sweep behind tray_denoise_variance_default_params, on the CPU: oracle
passes of the book cover (seed 2, d = 50) folded by the numpy restatement
tests/progressive_ref.py into means of 16 (4 passes of r = 4), 64 (4 of r = 16) and 256 (16 of
r = 16) samples, filtered by the restatement's variance-guided filter over a grid of
sigma_variance and epsilon, against a target of r = 1024 at pass 1 (sample words 1024..2047:
disjoint from the words 0..255 of the passes). The guides are those of the r = 16 frame at pass
0 (tests/denoise_frames.py). Prints one JSON line per setting with MSE(filtered, target) /
MSE(mean, target) per size and sample count, and the same ratio for the plain filter of
tray_denoise.h with its defaults.

    python tools/progressive_sweep.py [--sizes 64x36,96x54,160x90] [--sigma-variance 1,2,4] [--epsilon 1e-12] [--out FILE]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SIGMA_VARIANCE = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
EPSILON = (1e-12, 1e-8, 1e-5)
STATES = ((16, 4, 4), (64, 16, 4), (256, 16, 16))  # samples in the mean: r, passes


def main() -> None:
    import denoise_frames as F
    import denoise_ref
    import progressive_ref as R
    from conftest import DEFAULT_BG
    from oracle import oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x36,96x54,160x90")
    ap.add_argument("--target", type=int, default=1024)
    ap.add_argument("--sigma-variance", default=",".join(map(str, SIGMA_VARIANCE)))
    ap.add_argument("--epsilon", default=",".join(map(str, EPSILON)))
    ap.add_argument("--out")
    a = ap.parse_args()
    workers = min(16, os.cpu_count() or 1)
    spheres = O.rich_scene(F.SEED)
    data = {}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        cam = F.camera_state(O, w, h)
        render = lambda r, p: O.render(spheres, DEFAULT_BG, cam, w, h, r, F.DEPTH, F.RADIUS, F.SEED,  # noqa: E731
                                       workers=workers, segments=False, pass_=p)
        passes = {4: [render(4, p) for p in range(4)], 16: [render(16, p) for p in range(16)]}
        target = render(a.target, 1)
        guides = F.oracle_guides(O, spheres, cam, w, h, 16)
        for samples, r, n in STATES:
            mean, m2, count = R.fold(None, np.stack(passes[r][:n]))
            data[size, samples] = (mean, R.variance_of_mean(m2, count), target, guides)
    mse = lambda x, t: float(np.mean((x - t) ** 2))  # noqa: E731
    plain = {"filter": "tray_denoise.h defaults"}
    for (size, samples), (mean, _, target, g) in data.items():
        plain[f"{size}@{samples}"] = mse(denoise_ref.denoise(mean, *g), target) / mse(mean, target)
    print(json.dumps(plain), flush=True)
    lines = []
    grid = [tuple(float(v) for v in s.split(",")) for s in (a.sigma_variance, a.epsilon)]
    for sv, eps in itertools.product(*grid):
        rec = {"sigma_variance": sv, "epsilon": eps}
        for (size, samples), (mean, variance, target, g) in data.items():
            out, _ = R.denoise_variance(mean, variance, *g, sigma_variance=sv, epsilon=eps)
            rec[f"{size}@{samples}"] = mse(out, target) / mse(mean, target)
        for samples, _, _ in STATES:
            rec[f"mean@{samples}"] = float(np.mean([v for k, v in rec.items() if k.endswith(f"@{samples}")
                                                    and not k.startswith("mean")]))
        rec["mean_ratio"] = float(np.mean([rec[f"mean@{s}"] for s, _, _ in STATES]))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    print(json.dumps({"best": min(lines, key=lambda r: r["mean_ratio"])}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(plain) + "\n")
            for rec in sorted(lines, key=lambda r: r["mean_ratio"]):
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
