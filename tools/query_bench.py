#!/usr/bin/env python3
"""Throughput of the batched ray queries (include/tray_query.h) beside the
megakernel, on the C2 scene (book cover, seed 2) at 1280x720.

The camera rays of rays_per_pixel = 4 (3.7 M rays, tray_camera_rays_async) are
fed to tray_scene_hit_async (BVH, and TRAY_FLAG_LINEAR_SCAN) and to
tray_ray_color_async at depth 50; tray_render_async renders the same params
(the unchanged megakernel: the yardstick). Each is timed with device events
after a warm-up, as the median over --repeats of --inner back-to-back launches
(one launch is a fraction of a millisecond); segments (Scene.Hit calls)
are counted in separate, untimed launches. Prints one JSON line:

    python tools/query_bench.py [--repeats 10] [--lib other/libtray_amd.so]

The queries of include/tray_shade.h run in the same windows: the occlusion query
(t_end = inf) beside the closest hit on the same camera rays, Material.Scatter on
those rays' hit records, AmbientLight.Hit, and closest hit and occlusion again on
a ray set that starts on surfaces (the scattered rays of the first bounce). Their
figures, each with its min and max, go to --shade-out.

--lib also times the hit and colour queries of another build of the library
(tools/build_variants.sh), alternating with the in-tree build, and checks that
its results are the same bits.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed window")
    ap.add_argument("--rays-per-pixel", type=int, default=4)
    ap.add_argument("--lib", default=None, help="another build of libtray_amd.so to time beside the in-tree one")
    ap.add_argument("--shade-out", default="profiles/shade_bench_c2.json",
                    help="where (under the repository) the tray_shade.h figures go; '' writes none")
    args = ap.parse_args()
    import torch

    from bench import CONFIGS
    from tray_amd import _lib, ray

    label, seed, half, W, H, _, depth = CONFIGS["c2"]
    r = args.rays_per_pixel
    spheres = ray.rich_scene_array(seed, half)
    cam = ray.RichSceneCamera()
    cam.Initialize(W, H)
    bg = ray._background(ray.DefaultBackground())
    params = _lib.make_params(W, H, depth, r, 0.5, seed, output=_lib.OUT_RGB_F32)
    n = _lib.camera_rays_count(params)
    stream = torch.cuda.current_stream().cuda_stream
    scenes = {"tree": _lib.DeviceScene(spheres, bg, 0)}
    if args.lib:
        scenes["other"] = _lib.DeviceScene(spheres, bg, 0, os.path.abspath(args.lib))

    rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    ids = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    hits = {k: torch.empty((n, 8), dtype=torch.float64, device="cuda") for k in ("bvh", "linear", "other")}
    rgb = {k: torch.empty((n, 3), dtype=torch.float64, device="cuda") for k in ("tree", "other")}
    seg = torch.zeros(n, dtype=torch.int32, device="cuda")
    frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    frame_seg = torch.zeros((H, W), dtype=torch.int32, device="cuda")

    jobs = {
        "camera_rays": lambda: _lib.camera_rays_async(cam._state, params, rays.data_ptr(), ids.data_ptr(), 0, stream),
        "hit_bvh": lambda: scenes["tree"].hit_async(rays.data_ptr(), n, hits["bvh"].data_ptr(), stream=stream),
        "hit_linear": lambda: scenes["tree"].hit_async(rays.data_ptr(), n, hits["linear"].data_ptr(),
                                                       flags=_lib.FLAG_LINEAR_SCAN, stream=stream),
        "color": lambda: scenes["tree"].ray_color_async(rays.data_ptr(), n, depth, seed, rgb["tree"].data_ptr(),
                                                        ids.data_ptr(), None, stream=stream),
        "render": lambda: scenes["tree"].render_async(cam._state, params, frame.data_ptr(), None, stream),
    }
    # include/tray_shade.h on the same rays: occlusion (t_end = inf) beside the closest hit,
    # Material.Scatter on those rays' hit records, AmbientLight.Hit; and a second ray set that
    # starts on surfaces, the scattered rays of the first bounce, for occlusion and closest hit.
    jobs["camera_rays"]()
    jobs["hit_bvh"]()
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    scat = torch.empty((n, 10), dtype=torch.float64, device="cuda")
    sky = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    scenes["tree"].scatter_async(rays.data_ptr(), hits["bvh"].data_ptr(), n, seed, scat.data_ptr(), ids.data_ptr(), 0,
                                 stream)
    rays1 = scat[scat.view(torch.int32)[:, 18] == 1][:, 3:9].contiguous()  # bounce 1: the scattered rays
    n1 = len(rays1)
    hits1 = torch.empty((n1, 8), dtype=torch.float64, device="cuda")
    occ1 = torch.empty(n1, dtype=torch.uint8, device="cuda")
    shade_jobs = {
        "occluded": lambda: scenes["tree"].occluded_async(rays.data_ptr(), n, occ.data_ptr(), stream=stream),
        "scatter": lambda: scenes["tree"].scatter_async(rays.data_ptr(), hits["bvh"].data_ptr(), n, seed,
                                                        scat.data_ptr(), ids.data_ptr(), 0, stream),
        "sky": lambda: _lib.background_hit_async(bg, rays.data_ptr(), n, sky.data_ptr(), 0, stream),
        "hit_bvh_bounce1": lambda: scenes["tree"].hit_async(rays1.data_ptr(), n1, hits1.data_ptr(), stream=stream),
        "occluded_bounce1": lambda: scenes["tree"].occluded_async(rays1.data_ptr(), n1, occ1.data_ptr(),
                                                                   stream=stream),
    }
    jobs.update(shade_jobs)
    if args.lib:
        jobs["hit_bvh_other"] = lambda: scenes["other"].hit_async(rays.data_ptr(), n, hits["other"].data_ptr(),
                                                                  stream=stream)
        jobs["color_other"] = lambda: scenes["other"].ray_color_async(rays.data_ptr(), n, depth, seed,
                                                                      rgb["other"].data_ptr(), ids.data_ptr(), None,
                                                                      stream=stream)
    jobs["camera_rays"]()
    for job in jobs.values():  # warm-up: code objects, the render's launch context and work order
        job()
        job()
    torch.cuda.synchronize()
    times = {k: [] for k in jobs}
    for _ in range(args.repeats):  # the jobs alternate, so a drift of the machine hits them alike
        for name, job in jobs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.inner):
                job()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.inner)
    ms = {k: statistics.median(v) for k, v in times.items()}

    # untimed: the segment counts, and that every variant computed the same bits
    scenes["tree"].ray_color_async(rays.data_ptr(), n, depth, seed, rgb["tree"].data_ptr(), ids.data_ptr(),
                                   seg.data_ptr(), stream=stream)
    scenes["tree"].render_async(cam._state, params, frame.data_ptr(), frame_seg.data_ptr(), stream)
    torch.cuda.synchronize()
    color_segments, render_segments = int(seg.sum().item()), int(frame_seg.sum().item())
    assert color_segments == render_segments, (color_segments, render_segments)
    assert torch.equal(hits["bvh"], hits["linear"]), "BVH and linear-scan hits differ"
    if args.lib:
        assert torch.equal(hits["bvh"], hits["other"]) and torch.equal(rgb["tree"], rgb["other"]), "--lib differs"
    index, index1 = hits["bvh"].view(torch.int32)[:, 14], hits1.view(torch.int32)[:, 14]
    assert torch.equal(occ != 0, index >= 0) and torch.equal(occ1 != 0, index1 >= 0), "occlusion is not index >= 0"
    occluded, occluded1 = int(occ.sum().item()), int(occ1.sum().item())
    for s in scenes.values():
        s.release()

    out = {
        "scene": label.split(" 1280")[0], "width": W, "height": H, "rays_per_pixel": r, "max_depth": depth,
        "rays": n, "segments": color_segments, "repeats": args.repeats,
        "launches_per_window": args.inner,
        "ms": {k: round(v, 4) for k, v in ms.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
        "hit_bvh_mrays_s": round(n / ms["hit_bvh"] / 1e3, 1),
        "hit_linear_mrays_s": round(n / ms["hit_linear"] / 1e3, 1),
        "color_msegments_s": round(color_segments / ms["color"] / 1e3, 1),
        "render_msegments_s": round(render_segments / ms["render"] / 1e3, 1),
        "hit_bvh_over_linear": round(ms["hit_linear"] / ms["hit_bvh"], 2),
        "color_over_render": round(ms["render"] / ms["color"], 3),
        "code_object_sha256": _lib.code_object_sha256(),
    }
    if args.lib:
        out["other_lib"] = os.path.relpath(os.path.abspath(args.lib), ROOT)
        out["other_hit_bvh_mrays_s"] = round(n / ms["hit_bvh_other"] / 1e3, 1)
        out["other_color_msegments_s"] = round(color_segments / ms["color_other"] / 1e3, 1)
    print(json.dumps(out))
    if args.shade_out:
        names = ["hit_bvh"] + list(shade_jobs)
        shade = {
            "scene": out["scene"], "width": W, "height": H, "rays_per_pixel": r, "rays": n, "rays_occluded": occluded,
            "bounce1_rays": n1, "bounce1_rays_occluded": occluded1, "repeats": args.repeats,
            "launches_per_window": args.inner,
            "ms": {k: out["ms"][k] for k in names},
            "ms_min_max": {k: out["ms_min_max"][k] for k in names},
            "occluded_over_hit_bvh": round(ms["occluded"] / ms["hit_bvh"], 3),
            "occluded_over_hit_bvh_bounce1": round(ms["occluded_bounce1"] / ms["hit_bvh_bounce1"], 3),
            "scatter_mrays_s": round(n / ms["scatter"] / 1e3, 1),
            "sky_mrays_s": round(n / ms["sky"] / 1e3, 1),
            "code_object_sha256": out["code_object_sha256"],
        }
        path = os.path.join(ROOT, args.shade_out)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(shade, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
