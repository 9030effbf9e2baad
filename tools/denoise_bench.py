#!/usr/bin/env python3
"""Time of the guided a-trous denoiser (include/tray_denoise.h) on a C2-sized
frame (book cover, seed 2, 1280x720, r = 16) with the default parameters, beside
the render and the feature buffers of the same frame.

The whole call (5 launches) is timed, and the calls with 1 .. 5 iterations: level
i's time is the difference of the calls with i + 1 and i iterations (the call is
one launch per level; the last level's store also remodulates). Against the
algorithmic traffic of a level, 7 doubles read and 3 written per pixel (80 B),
that gives the bandwidth a level achieves. With --ab-lib (a build of `make -C
tray_amd denoise_ab`, whose levels read their taps from global memory) the same
jobs run on that library too, alternating with the product's inside one
process, after its output was checked to have the same bits. That variant divides by the
albedo (level 0) and takes 1/depth at every tap, where the product does so once per staged point;
the `plain` jobs (no flag, no depth guide) time both without those divisions. Each job is timed
with device events after a warm-up, as the median over --repeats windows of
--inner back-to-back calls. Prints one JSON line and writes it to --out:

    python tools/denoise_bench.py [--ab-lib tray_amd/build/libtray_amd_denoise_global.so]
                                  [--repeats 15] [--out profiles/denoise_bench_c2.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_PIXEL_LEVEL = (7 + 3) * 8  # colour, normal, depth read; colour written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--r", type=int, default=16, help="rays per pixel of the frame")
    ap.add_argument("--ab-lib", default="", help="a denoise_ab build to time beside the product")
    ap.add_argument("--out", default="profiles/denoise_bench_c2.json", help="where (under the repository) the result goes")
    args = ap.parse_args()
    import torch

    from bench import CONFIGS
    from tray_amd import _lib, ray

    label, seed, half, W, H, _, depth = CONFIGS["c2"]
    spheres = ray.rich_scene_array(seed, half)
    cam = ray.RichSceneCamera()
    cam.Initialize(W, H)
    bg = ray._background(ray.DefaultBackground())
    p = _lib.make_params(W, H, depth, args.r, 0.5, seed)
    stream = torch.cuda.current_stream().cuda_stream
    dev = _lib.DeviceScene(spheres, bg, 0)
    f64 = dict(dtype=torch.float64, device="cuda")
    colour, out, out_ab = (torch.empty((H, W, 3), **f64) for _ in range(3))
    albedo, normal, depth_buf = torch.empty((H, W, 3), **f64), torch.empty((H, W, 3), **f64), torch.empty((H, W), **f64)
    dp = {it: _lib.denoise_params(W, H, iterations=it) for it in range(1, 6)}
    assert dp[5].iterations == _lib.denoise_params(W, H).iterations  # the default
    need = _lib.denoise_workspace_bytes(dp[5])
    work = torch.empty((need // 8,), **f64)

    def render():
        dev.render_async(cam._state, p, colour.data_ptr(), None, stream)

    def aov():
        dev.render_aov_async(cam._state, p, albedo.data_ptr(), normal.data_ptr(), depth_buf.data_ptr(), stream=stream)

    def denoise(it, lib_path=None, dst=out):
        return lambda: _lib.denoise_async(colour.data_ptr(), dp[it], dst.data_ptr(), work.data_ptr(), need,
                                          albedo.data_ptr(), normal.data_ptr(), depth_buf.data_ptr(), 0, stream,
                                          lib_path=lib_path)

    render()
    aov()
    torch.cuda.synchronize()
    jobs = {"render": (render, 1), "aov": (aov, 1)}
    jobs.update({f"denoise_{it}": (denoise(it), args.inner) for it in dp})
    ab = os.path.join(ROOT, args.ab_lib) if args.ab_lib else None

    def plain(lib_path=None, dst=out):
        """5 levels without the flag and without the depth guide: no variant divides per tap or per
        staged point then (only acc / W per pixel), so the two differ in how they reach the taps alone."""
        p_plain = _lib.denoise_params(W, H, flags=0)
        return lambda: _lib.denoise_async(colour.data_ptr(), p_plain, dst.data_ptr(), work.data_ptr(), need,
                                          None, normal.data_ptr(), None, 0, stream, lib_path=lib_path)

    jobs["denoise_plain"] = (plain(), args.inner)
    if ab:
        jobs.update({f"global_taps_{it}": (denoise(it, ab, out_ab), args.inner) for it in dp})
        jobs["global_taps_plain"] = (plain(ab, out_ab), args.inner)
        plain()()
        plain(ab, out_ab)()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), out_ab.view(torch.int64)), "the two variants differ (plain)"
        denoise(5)()
        denoise(5, ab, out_ab)()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), out_ab.view(torch.int64)), "the two variants differ"
    for job, _ in jobs.values():  # warm-up: code objects, the render's launch context
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
    dev.release()

    def levels(prefix):
        return [ms[f"{prefix}_1"]] + [ms[f"{prefix}_{it + 1}"] - ms[f"{prefix}_{it}"] for it in range(1, 5)]

    level_bytes = W * H * BYTES_PER_PIXEL_LEVEL
    res = {
        "scene": label.split(" 1280")[0], "width": W, "height": H, "max_depth": depth, "rays_per_pixel": args.r,
        "repeats": args.repeats, "launches_per_window": {k: inner for k, (_, inner) in jobs.items()},
        "params": {n: getattr(dp[5], n) for n, _ in _lib.DenoiseParams._fields_},
        "workspace_bytes": need,
        "ms": {k: round(v, 4) for k, v in ms.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
        "denoise_ms": round(ms["denoise_5"], 4),
        "level_ms": [round(v, 4) for v in levels("denoise")],
        "level_bytes": level_bytes,
        "level_gb_s": [round(level_bytes / v / 1e6, 1) for v in levels("denoise")],
        "denoise_over_render": round(ms["denoise_5"] / ms["render"], 3),
        "denoise_over_aov": round(ms["denoise_5"] / ms["aov"], 3),
        "code_object_sha256": _lib.code_object_sha256(),
    }
    if ab:
        res["global_taps_ms"] = round(ms["global_taps_5"], 4)
        res["global_taps_level_ms"] = [round(v, 4) for v in levels("global_taps")]
        res["global_taps_over_tiled"] = round(ms["global_taps_5"] / ms["denoise_5"], 3)
        res["plain_ms"] = {"tiled": round(ms["denoise_plain"], 4), "global_taps": round(ms["global_taps_plain"], 4),
                           "what": "5 levels, flags 0, depth guide null: no per-tap or per-point division"}
        res["plain_global_taps_over_tiled"] = round(ms["global_taps_plain"] / ms["denoise_plain"], 3)
    print(json.dumps(res))
    if args.out:
        path = os.path.join(ROOT, args.out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
