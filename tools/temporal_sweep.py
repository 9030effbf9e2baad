"""The sweep behind tray_temporal_default_params (include/tray_temporal.h), on the CPU:
the oracle renders the frames and traces the centre rays, tests/temporal_ref.py does the steps.

An 8-frame orbit of the book cover at r = 4 and three small sizes; for max_history x depth_tolerance
the MSE of the last accumulated frame against an independent high-sample frame of the last camera,
relative to the MSE of that camera's single r = 4 frame (below 1: the history helped). Also the
static case (every pixel must snap at snap = 2^-20) and, for the default row, the ratio per
material class of the last frame's centre hit (view-dependent surfaces gain less).

    python tools/temporal_sweep.py [--out profiles/temporal_sweep.jsonl] [--step 1.0] [--truth 1024]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import temporal_ref as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

RICH_SETUP = np.array([13, 2, 3, 0, 0, 0, 0, 1, 0, 20.0, 10.0, 10.0, 0.1])
BG = O.DEFAULT_BACKGROUND
SIZES = ((32, 18), (48, 27), (64, 36))
HISTORIES, TOLERANCES = (8, 16, 32, 64), (0.02, 0.1, 0.5)
CLASSES = {1: "lambertian", 2: "metal", 3: "dielectric", -1: "sky"}  # tray_material, and a miss


def sequence(spheres, w, h, n, step, workers):
    cams = [O.camera_initialize(R.orbit_setup(RICH_SETUP, k * step), w, h)[1] for k in range(n)]
    frames = [O.render(spheres, BG, c, w, h, 4, 50, 0.5, 2, workers=workers, segments=False, pass_=k)
              for k, c in enumerate(cams)]
    hits = [R.oracle_hits(O, spheres, c, w, h) for c in cams]
    return cams, frames, hits


def accumulate(cams, frames, hits, **params):
    state, fresh = None, []
    for k in range(len(cams)):
        state, rec = R.step(cams[k], cams[k - 1] if k else None, frames[k], hits[k], state, **params)
        fresh.append(rec[0])
    return state, fresh


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_sweep.jsonl"))
    ap.add_argument("--step", type=float, default=1.0, help="degrees between frames")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--truth", type=int, default=1024, help="rays per pixel of the reference frame")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args(argv)
    spheres = O.rich_scene(2)
    material = np.asarray(spheres["material"])
    rows = []
    for w, h in SIZES:
        cams, frames, hits = sequence(spheres, w, h, a.frames, a.step, a.workers)
        truth = O.render(spheres, BG, cams[-1], w, h, a.truth, 50, 0.5, 77, workers=a.workers, segments=False)
        single = float(((frames[-1] - truth) ** 2).mean())
        z, u, v, ok = R.project(cams[0], cams[0], w, h, *hits[0])
        rows.append(dict(kind="static", width=w, height=h, in_range=int(ok.sum()), snapped=int(R.snapped_mask(u, v).sum()),
                         pixels=w * h, max_offset=float(max(np.abs(u - np.round(u)).max(), np.abs(v - np.round(v)).max()))))
        for mh in HISTORIES:
            for tol in TOLERANCES:
                state, fresh = accumulate(cams, frames, hits, max_history=mh, depth_tolerance=tol)
                mse = float(((state["colour"] - truth) ** 2).mean())
                rows.append(dict(kind="orbit", width=w, height=h, step=a.step, frames=a.frames, max_history=mh,
                                 depth_tolerance=tol, mse=mse, mse_single=single, ratio=mse / single,
                                 fresh_last=fresh[-1], mean_age=float(state["age"].mean())))
        state, _ = accumulate(cams, frames, hits)  # the defaults, per material class of the last centre hit
        cls = np.where(hits[-1][0] >= 0, material[np.maximum(hits[-1][0], 0)], -1)
        for c, name in CLASSES.items():
            m = cls == c
            if m.any():
                one = float(((frames[-1][m] - truth[m]) ** 2).mean())
                rows.append(dict(kind="class", width=w, height=h, material=name, pixels=int(m.sum()),
                                 ratio=float(((state["colour"][m] - truth[m]) ** 2).mean()) / one))
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("max_history depth_tolerance  " + "  ".join(f"{w}x{h}" for w, h in SIZES) + "   mean")
    for mh in HISTORIES:
        for tol in TOLERANCES:
            rs = [r["ratio"] for r in rows if r["kind"] == "orbit" and r["max_history"] == mh
                  and r["depth_tolerance"] == tol]
            print(f"{mh:11d} {tol:15.2f}  " + "  ".join(f"{x:.4f}" for x in rs) + f"   {np.mean(rs):.4f}")
    for r in rows:
        if r["kind"] != "orbit":
            print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
