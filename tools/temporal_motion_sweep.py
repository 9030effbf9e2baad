"""What temporal reprojection across scene updates gains (include/tray_temporal_motion.h),
on the CPU: the oracle renders the frames and traces the centre rays, tests/temporal_motion_ref.py
does the steps, tests/temporal_variance_ref.py the refill chain.

The ray.Bounce animation of the book cover (the small spheres hop) over 8 frames at r = 4 and three
small sizes, under a still camera: the MSE of the last accumulated frame against an independent
high-sample frame of the last geometry, relative to the MSE of that geometry's single r = 4 frame
(below 1: the history helped), over the whole frame, over the pixels of moved spheres, and over the
pixels fresh in the last frame without and with refill = 3. And one row per size where a single large
mirror sphere moves and everything else stands still, over the pixels of UNMOVED spheres: what the
lag of the shading costs (history follows surfaces, not light).

    python tools/temporal_motion_sweep.py [--out profiles/temporal_motion_sweep.jsonl] [--truth 1024]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import temporal_motion_ref as M  # noqa: E402
import temporal_ref as R  # noqa: E402
import temporal_variance_ref as V  # noqa: E402
from oracle import oracle as O  # noqa: E402

RICH_SETUP = np.array([13, 2, 3, 0, 0, 0, 0, 1, 0, 20.0, 10.0, 10.0, 0.1])
BG = O.DEFAULT_BACKGROUND
SIZES = ((32, 18), (48, 27), (64, 36))
BOUNCE_STEP, REFILL = 0.4, 3  # tray_amd.ray.BOUNCE_STEP, REFILL_DEFAULT


def geometry(spheres):
    return np.ascontiguousarray(np.concatenate([spheres["center"], spheres["radius"][:, None]], axis=1))


def with_geometry(spheres, g):
    s = spheres.copy()
    s["center"], s["radius"] = g[:, :3], g[:, 3]
    return s


def bounce(spheres, frames):
    """tray_amd.ray.Bounce on the oracle's array."""
    g = geometry(spheres)
    out = np.repeat(g[None], frames, axis=0)
    small = np.nonzero(g[:, 3] < 0.5)[0]
    for k in range(frames):
        out[k, small, 1] = g[small, 3] + np.abs(np.sin(small + BOUNCE_STEP * k))
    return out


def mirror(spheres, frames):
    """The large metal sphere slides 0.25 along x per frame; nothing else moves."""
    g = geometry(spheres)
    big = int(np.nonzero((g[:, 3] == 1.0) & (np.asarray(spheres["material"]) == 2))[0][0])
    out = np.repeat(g[None], frames, axis=0)
    out[:, big, 0] += 0.25 * np.arange(frames)
    return out


def run(spheres, geos, cam, w, h, refill, workers):
    """The animation through the restatement: (last state, the fresh mask of the last step, the last
    single frame, the last hits)."""
    state, stride = None, 1 + refill
    for k, g in enumerate(geos):
        s = with_geometry(spheres, g)
        frame = O.render(s, BG, cam, w, h, 4, 50, 0.5, 2, workers=workers, segments=False, pass_=k * stride)
        hits = R.oracle_hits(O, s, cam, w, h)
        state, _, rec, _ = M.step(cam, cam if k else None, frame, hits, state, g, geos[k - 1] if k else g, True)
        fresh = state["age"] == 1
        if refill:
            sel = V.refill_list(state, refill, M.MAX_HISTORY)
            px = np.asarray(sel["pixels"], dtype=np.int64)
            if len(px):
                vals = np.stack([O.render_pixels(s, BG, cam, w, h, 4, 50, 0.5, 2, px % w, px // w,
                                                 pass_=k * stride + 1 + j)[0] for j in range(refill)])
                state = V.refill_fold(state, px, vals)
    return state, fresh, frame, hits


def ratio(state, single, truth, mask):
    if not mask.any():
        return None
    return float(((state["colour"] - truth)[mask] ** 2).mean()) / float(((single - truth)[mask] ** 2).mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_motion_sweep.jsonl"))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--truth", type=int, default=1024, help="rays per pixel of the reference frame")
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args(argv)
    spheres = O.rich_scene(2)
    rows = []
    for w, h in SIZES:
        cam = O.camera_initialize(RICH_SETUP, w, h)[1]
        for kind, geos in (("bounce", bounce(spheres, a.frames)), ("mirror", mirror(spheres, a.frames))):
            last = with_geometry(spheres, geos[-1])
            truth = O.render(last, BG, cam, w, h, a.truth, 50, 0.5, 77, workers=a.workers, segments=False)
            state, fresh, single, hits = run(spheres, geos, cam, w, h, 0, a.workers)
            moved_sphere = (geos[-1] != geos[0]).any(axis=1)
            on_moved = np.where(hits[0] >= 0, moved_sphere[np.maximum(hits[0], 0)], False)
            every = np.ones((h, w), dtype=bool)
            row = dict(kind=kind, width=w, height=h, frames=a.frames, truth=a.truth, fresh_last=int(fresh.sum()),
                       mean_age=float(state["age"].mean()), pixels_on_moved=int(on_moved.sum()),
                       ratio=ratio(state, single, truth, every), ratio_on_moved=ratio(state, single, truth, on_moved),
                       ratio_on_unmoved=ratio(state, single, truth, ~on_moved),
                       ratio_fresh_last=ratio(state, single, truth, fresh))
            if kind == "bounce":
                state3, _, _, _ = run(spheres, geos, cam, w, h, REFILL, a.workers)
                row.update(refill=REFILL, ratio_refill=ratio(state3, single, truth, every),
                           ratio_fresh_last_refill=ratio(state3, single, truth, fresh))
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
