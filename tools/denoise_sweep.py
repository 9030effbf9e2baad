"""The sigma sweep behind tray_denoise_default_params, on the CPU:
oracle frames of the book cover (noisy r = 16 at pass 0, target r = 1024 at pass
1, guides reduced from the oracle's hit records), filtered by the numpy
restatement tests/denoise_ref.py over a grid of sigmas. Prints one JSON line per
setting: MSE(denoised, target) / MSE(noisy, target).

    python tools/denoise_sweep.py [--sizes 64x36,96x54] [--sigma-color 0.25,0.5] [--modes 5:1] [--out FILE]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SIGMA_COLOR = (0.125, 0.25, 0.5, 1.0, 2.0)
SIGMA_NORMAL = (0.25, 0.5, 1.0)
SIGMA_DEPTH = (0.0625, 0.25, 0.75)


def main() -> None:
    import denoise_frames
    import denoise_ref
    from oracle import oracle as O

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64x36,96x54")
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--target", type=int, default=1024)
    ap.add_argument("--sigma-color", default=",".join(map(str, SIGMA_COLOR)))
    ap.add_argument("--sigma-normal", default=",".join(map(str, SIGMA_NORMAL)))
    ap.add_argument("--sigma-depth", default=",".join(map(str, SIGMA_DEPTH)))
    ap.add_argument("--modes", default="5:1,5:0,3:1", help="iterations:demodulate pairs")
    ap.add_argument("--out")
    a = ap.parse_args()
    grid = [tuple(float(v) for v in g.split(",")) for g in (a.sigma_color, a.sigma_normal, a.sigma_depth)]
    modes = [tuple(int(v) for v in m.split(":")) for m in a.modes.split(",")]
    frames = {}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        frames[size] = denoise_frames.book_cover(O, w, h, a.r, a.target, workers=min(16, os.cpu_count() or 1))
    lines = []
    for it, demod in modes:
        for sc, sn, sz in itertools.product(*grid):
            rec = {"iterations": it, "demodulate": demod, "sigma_color": sc, "sigma_normal": sn, "sigma_depth": sz}
            for size, (noisy, target, albedo, normal, depth) in frames.items():
                out = denoise_ref.denoise(noisy, albedo, normal, depth, it, demod, sc, sn, sz)
                rec["mse_ratio_" + size] = float(np.mean((out - target) ** 2) / np.mean((noisy - target) ** 2))
            rec["mean_ratio"] = float(np.mean([v for k, v in rec.items() if k.startswith("mse_ratio_")]))
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    best = min(lines, key=lambda r: r["mean_ratio"])
    print(json.dumps({"best": best}))
    if a.out:
        with open(a.out, "w") as f:
            for rec in sorted(lines, key=lambda r: r["mean_ratio"]):
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
