#!/usr/bin/env python3
"""Times of the adaptive path (include/tray_adaptive.h) on a C2-sized frame (book cover, seed 2,
1280x720, r = 16).

(a) tray_render_pixels_async per sample against tray_render_passes_async with the ordered sum on
    the same frame, at active fractions near 1, 0.5, 0.25 and 0.1. The lists come from a real
    state (8 uniform passes folded): the list of fraction f is what tray_adaptive_select_async
    writes at the tolerance, found by bisection, that leaves about f of the pixels active, so it
    has the shape of a real round (the noisy regions, dilated), not random pixels. The break-even
    fraction is where the list's time, interpolated, reaches the full frame's.
(b) tray_adaptive_select_async and tray_adaptive_fold_async (4 passes) in ms at those fractions.
(c) Wall time and pixel-passes of Tracer.RenderAdaptive against Tracer.RenderProgressive, to the
    library's tolerance, max_passes 32, the same seed.

(a) and (b) alternate inside one process and are timed with device events after a warm-up, as the
median over --repeats windows; minimum and maximum are in the file. (c) is host wall time, the
median of --runs runs each. Prints one JSON line and writes it to --out:

    python tools/adaptive_bench.py [--repeats 9] [--out profiles/adaptive_bench_c2.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACTIONS = (1.0, 0.5, 0.25, 0.1)
WARM, BATCH, MAX_PASSES = 8, 4, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3, help="calls per timed window")
    ap.add_argument("--runs", type=int, default=3, help="runs of each whole loop in (c)")
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--out", default="profiles/adaptive_bench_c2.json")
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import CONFIGS
    from tray_amd import _lib, ray

    label, seed, half, W, H, _, depth = CONFIGS["c2"]
    spheres = ray.rich_scene_array(seed, half)
    cam = ray.RichSceneCamera()
    cam.Initialize(W, H)
    bg = ray._background(ray.DefaultBackground())
    ordered = _lib.make_params(W, H, depth, args.r, 0.5, seed, flags=_lib.FLAG_ORDERED_SUM)
    p = _lib.make_params(W, H, depth, args.r, 0.5, seed)
    stream = torch.cuda.current_stream().cuda_stream
    dev = _lib.DeviceScene(spheres, bg, 0)
    f64 = dict(dtype=torch.float64, device="cuda")
    n = W * H
    frames = torch.empty((WARM, H, W, 3), **f64)
    dev.render_passes_async(cam._state, ordered, WARM, frames.data_ptr(), stream)
    mean0, m20 = torch.empty((H, W, 3), **f64), torch.empty((H, W, 3), **f64)
    acc = _lib.Accum(mean0.data_ptr(), m20.data_ptr(), W, H, 0, 0)
    _lib.accum_fold_async(acc, frames.data_ptr(), WARM, 0, stream)
    count0 = torch.full((H, W), WARM, dtype=torch.int32, device="cuda")
    mean, m2, count = mean0.clone(), m20.clone(), count0.clone()
    state = _lib.AdaptiveState(mean.data_ptr(), m2.data_ptr(), count.data_ptr(), W, H)
    nbytes = _lib.adaptive_workspace_bytes(W, H)
    work = torch.empty((nbytes // 8,), **f64)
    record = torch.empty((4,), **f64)
    variance = torch.empty((H, W, 3), **f64)
    one = frames[:1]
    values = torch.empty((BATCH, n, 3), **f64)

    def select(tolerance, lst, var_ptr=None):
        ap_ = _lib.adaptive_params(tolerance=tolerance, min_passes=WARM, max_passes=MAX_PASSES)
        _lib.adaptive_select_async(state, ap_, lst.data_ptr(), record.data_ptr(), work.data_ptr(), nbytes, var_ptr, 0,
                                   stream)

    def active(tolerance, lst):
        select(tolerance, lst)
        return int(record.cpu().numpy().view(_lib.ADAPTIVE_RECORD_DTYPE)[0]["n_active"])

    lists = {}
    for f in FRACTIONS:
        lst = torch.empty((n,), dtype=torch.int32, device="cuda")
        lo, hi = 0.0, 4.0  # the active set shrinks as the tolerance grows
        if f < 1.0:
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if active(mid, lst) > f * n else (lo, mid)
        lists[f] = (lst, hi if f < 1.0 else 0.0, active(hi if f < 1.0 else 0.0, lst))

    def full_pass():
        dev.render_passes_async(cam._state, ordered, 1, one.data_ptr(), stream)

    def pixels_job(f):
        lst, _, k = lists[f]
        return lambda: dev.render_pixels_async(cam._state, p, lst.data_ptr(), k, values.data_ptr(), 1,
                                               pass_plane_ptr=count0.data_ptr(), stream=stream)

    def select_job(f):
        lst, tol, _ = lists[f]
        scratch = torch.empty((n,), dtype=torch.int32, device="cuda")
        return lambda: select(tol, scratch, variance.data_ptr())

    def fold_job(f):
        lst, _, k = lists[f]

        def job():  # the counts grow by 4 per call, as in the loop; the values do not matter to the time
            _lib.adaptive_fold_async(state, lst.data_ptr(), k, values.data_ptr(), BATCH, 0, stream)
        return job

    jobs = {"full_pass_ordered": full_pass}
    for f in FRACTIONS:
        jobs[f"pixels_{f}"] = pixels_job(f)
        jobs[f"select_{f}"] = select_job(f)
    for job in jobs.values():
        job()
    torch.cuda.synchronize()
    times = {k: [] for k in jobs}

    def window(name, job, inner):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            job()
        t1.record()
        t1.synchronize()
        times.setdefault(name, []).append(t0.elapsed_time(t1) / inner)

    for _ in range(args.repeats):
        for name, job in jobs.items():
            window(name, job, args.inner)
    for f in FRACTIONS:  # after the selects: the folds change the counts the lists were made from
        job = fold_job(f)
        job()
        for _ in range(args.repeats):
            window(f"fold4_{f}", job, 1)
    torch.cuda.synchronize()
    ms = {k: statistics.median(v) for k, v in times.items()}
    full_ns = ms["full_pass_ordered"] * 1e6 / (n * args.r)
    rows, xs, ys = [], [], []
    for f in FRACTIONS:
        k = lists[f][2]
        rows.append({"asked": f, "fraction": round(k / n, 4), "n_active": k, "tolerance": lists[f][1],
                     "ms": round(ms[f"pixels_{f}"], 4),
                     "ns_per_sample": round(ms[f"pixels_{f}"] * 1e6 / (k * args.r), 4),
                     "over_full_per_sample": round(ms[f"pixels_{f}"] * 1e6 / (k * args.r) / full_ns, 4),
                     "select_ms": round(ms[f"select_{f}"], 4), "fold4_ms": round(ms[f"fold4_{f}"], 4)})
        xs.append(k / n)
        ys.append(ms[f"pixels_{f}"])
    order = np.argsort(xs)
    xs, ys = np.array(xs)[order], np.array(ys)[order]
    breakeven = float(np.interp(ms["full_pass_ordered"], ys, xs)) if ys[0] < ms["full_pass_ordered"] < ys[-1] else None

    # (c) the whole loops, wall time
    def tracer():
        t = ray.New(W, H)
        t.Camera = ray.RichSceneCamera()
        t.NumRaysPerPixel, t.MaxDepth, t.Seed = args.r, depth, seed
        return t

    scene = ray.Scene.from_array(spheres)
    loops = {}
    for name in ("RenderProgressive", "RenderAdaptive"):
        t = tracer()
        wall = []
        for i in range(args.runs + 1):  # the first run warms the allocator and is not kept
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            getattr(t, name)(scene, MAX_PASSES)
            torch.cuda.synchronize()
            if i:
                wall.append(time.perf_counter() - t0)
        passes = t.pixel_passes if name == "RenderAdaptive" else t.passes * n
        loops[name] = {"wall_s": round(statistics.median(wall), 4), "wall_s_min_max": [round(min(wall), 4),
                                                                                      round(max(wall), 4)],
                       "pixel_passes": int(passes), "max_passes_in_a_pixel": int(t.passes),
                       "unconverged": int(t.unconverged), "max_ratio": float(t.max_ratio)}
    dev.release()
    res = {
        "scene": label.split(" 1280")[0], "width": W, "height": H, "rays_per_pixel": args.r, "warm_up_passes": WARM,
        "repeats": args.repeats, "inner": args.inner, "runs": args.runs,
        "full_pass_ordered_ms": round(ms["full_pass_ordered"], 4), "full_pass_ns_per_sample": round(full_ns, 4),
        "pixels": rows, "break_even_fraction": breakeven,
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
        "loops": loops,
        "adaptive_over_progressive_wall": round(loops["RenderAdaptive"]["wall_s"] /
                                                loops["RenderProgressive"]["wall_s"], 4),
        "adaptive_over_progressive_pixel_passes": round(loops["RenderAdaptive"]["pixel_passes"] /
                                                        loops["RenderProgressive"]["pixel_passes"], 4),
        "code_object_sha256": _lib.code_object_sha256(),
    }
    print(json.dumps(res))
    if args.out:
        path = os.path.join(ROOT, args.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
