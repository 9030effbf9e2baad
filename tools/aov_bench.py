#!/usr/bin/env python3
"""Time of the first-hit feature buffers (include/tray_aov.h) on the C2 scene
(book cover, seed 2) at 1280x720, beside the only other way to the same data
and beside a render.

At rays_per_pixel = 4 (3.7 M samples, so that the composition's per-sample
buffers fit as in tools/query_bench.py) the fused tray_render_aov_async (all
five buffers) is timed against tray_camera_rays_async + tray_scene_hit_async
at the same ray count: the two launches a caller needs before reducing per
pixel on their own (that reduction, and the sky colours of the misses, are not
in the composition's time). At rays_per_pixel = 64 the fused call is timed
alone, beside one tray_render_async frame of the same params, for scale.
Each job is timed with device events after a warm-up, as the median over
--repeats windows of back-to-back launches; the jobs alternate inside one
process, so a drift of the machine hits them alike. Prints one JSON line and
writes it to --out:

    python tools/aov_bench.py [--repeats 15] [--out profiles/aov_bench_c2.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_PIXEL_OUT = 3 * 8 + 3 * 8 + 8 + 8 + 4  # albedo, normal, depth, coverage, index
BYTES_PER_SAMPLE_COMPOSED = 48 + 64  # a tray_ray and a tray_hit written (and the ray read again)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="launches per timed window of the r = 4 jobs")
    ap.add_argument("--out", default="profiles/aov_bench_c2.json", help="where (under the repository) the result goes")
    args = ap.parse_args()
    import torch

    from bench import CONFIGS
    from tray_amd import _lib, ray

    label, seed, half, W, H, _, depth = CONFIGS["c2"]
    spheres = ray.rich_scene_array(seed, half)
    cam = ray.RichSceneCamera()
    cam.Initialize(W, H)
    bg = ray._background(ray.DefaultBackground())
    p4 = _lib.make_params(W, H, depth, 4, 0.5, seed, output=_lib.OUT_RGB_F32)
    p64 = _lib.make_params(W, H, depth, 64, 0.5, seed, output=_lib.OUT_RGB_F32)
    n4 = _lib.camera_rays_count(p4)
    stream = torch.cuda.current_stream().cuda_stream
    dev = _lib.DeviceScene(spheres, bg, 0)

    rays = torch.empty((n4, 6), dtype=torch.float64, device="cuda")
    hits = torch.empty((n4, 8), dtype=torch.float64, device="cuda")
    frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    bufs = {name: torch.empty((H, W, ch)[: 3 if ch > 1 else 2],
                              dtype=torch.float64 if name != "index" else torch.int32, device="cuda")
            for name, ch, _ in _lib.AOV_BUFFERS}
    ptrs = [bufs[name].data_ptr() for name, _, _ in _lib.AOV_BUFFERS]

    def composed():
        _lib.camera_rays_async(cam._state, p4, rays.data_ptr(), None, 0, stream)
        dev.hit_async(rays.data_ptr(), n4, hits.data_ptr(), stream=stream)

    jobs = {
        "aov_r4": (lambda: dev.render_aov_async(cam._state, p4, *ptrs, stream=stream), args.inner),
        "composed_r4": (composed, args.inner),
        "aov_r64": (lambda: dev.render_aov_async(cam._state, p64, *ptrs, stream=stream), 1),
        "render_r64": (lambda: dev.render_async(cam._state, p64, frame.data_ptr(), None, stream), 1),
    }
    for job, _ in jobs.values():  # warm-up: code objects, the render's launch context and work order
        job()
        job()
    torch.cuda.synchronize()
    times = {k: [] for k in jobs}
    for _ in range(args.repeats):
        for name, (job, inner) in jobs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                job()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / inner)
    ms = {k: statistics.median(v) for k, v in times.items()}

    # untimed: the fused call and the composition saw the same first hits (sample 0's index, coverage)
    jobs["aov_r4"][0]()
    composed()
    torch.cuda.synchronize()
    index = hits.view(torch.int32)[:, 14].reshape(H, W, 4)
    assert torch.equal(bufs["index"], index[:, :, 0]), "index differs from the composition's"
    assert torch.equal(bufs["coverage"], (index >= 0).sum(dim=2).to(torch.float64) * 0.25), "coverage differs"
    covered = float(bufs["coverage"].mean().item())
    dev.release()

    out = {
        "scene": label.split(" 1280")[0], "width": W, "height": H, "max_depth": depth, "repeats": args.repeats,
        "launches_per_window": {k: inner for k, (_, inner) in jobs.items()},
        "samples_r4": n4, "samples_r64": _lib.camera_rays_count(p64), "mean_coverage_r4": round(covered, 4),
        "ms": {k: round(v, 4) for k, v in ms.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
        "aov_r4_msamples_s": round(n4 / ms["aov_r4"] / 1e3, 1),
        "composed_r4_msamples_s": round(n4 / ms["composed_r4"] / 1e3, 1),
        "aov_r64_msamples_s": round(_lib.camera_rays_count(p64) / ms["aov_r64"] / 1e3, 1),
        "composed_over_aov_r4": round(ms["composed_r4"] / ms["aov_r4"], 3),
        "render_over_aov_r64": round(ms["render_r64"] / ms["aov_r64"], 2),
        "bytes_per_pixel_written_aov": BYTES_PER_PIXEL_OUT,
        "bytes_per_pixel_written_composed_r4": BYTES_PER_SAMPLE_COMPOSED * 4,
        "bytes_per_pixel_written_composed_r64": BYTES_PER_SAMPLE_COMPOSED * 64,
        "code_object_sha256": _lib.code_object_sha256(),
    }
    print(json.dumps(out))
    if args.out:
        path = os.path.join(ROOT, args.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
