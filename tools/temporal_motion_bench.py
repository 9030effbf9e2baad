"""The cost of following moved spheres in the temporal reprojection step
(include/tray_temporal_motion.h) on a C2-sized frame (1280 x 720 book cover, r = 4, one orbit step of
1 degree), all in one process with the arms alternating: tray_temporal_motion_step_async with m2 and
the variance plane, once with a previous geometry equal to the scene's (no sphere moved: the static
step's arithmetic after one more gather and four comparisons) and once with every sphere's previous
centre 0.001 lower (all moved), beside tray_temporal_var_step_async on the same history; and the whole
frame of `-bounce` (Tracer.RenderAnimation over ray.Bounce, 8 frames, wall clock per frame with the
readback of the frames) with and without temporal=True. Device-event times of single launches after
a warm-up: median, minimum and maximum over --repeats. DESIGN.md 8w.

    python tools/temporal_motion_bench.py [--out profiles/temporal_motion_bench_c2.json] [--repeats 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_motion_bench_c2.json"))
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8, help="frames of the -bounce animation")
    a = ap.parse_args(argv)
    import torch

    from tray_amd import _lib as L
    from tray_amd import ray

    w, h = a.width, a.height
    prev, cam = ray.RichSceneCamera(), ray.Orbit(ray.RichSceneCamera(), ray.ORBIT_STEP_DEGREES)
    prev.Initialize(w, h), cam.Initialize(w, h)
    scene = ray.RichScene(2)
    scene.Background = ray.DefaultBackground()
    dev = scene._device_scene(0)
    n = len(scene.Objects)
    stream = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")

    def planes():
        t = dict(colour=torch.empty((h, w, 3), **f64), m2=torch.zeros((h, w, 3), **f64), age=torch.empty((h, w), **i32),
                 index=torch.empty((h, w), **i32), depth=torch.empty((h, w), **f64))
        return t, L.TemporalVarState(*(t[k].data_ptr() for k in ("colour", "m2", "age", "index", "depth")), w, h)

    hist, out = planes(), planes()
    frame, variance = torch.empty((h, w, 3), **f64), torch.empty((h, w, 3), **f64)
    motion = torch.empty((h, w, 2), **f64)
    record = torch.zeros((2,), dtype=torch.int64, device="cuda")
    tp = L.temporal_params()
    # the history: four frames of the previous camera folded by the step
    for k in range(4):
        dev.render_async(prev._state, L.make_params(w, h, 50, 4, 0.5, 2, pass_=k), frame.data_ptr(), None, stream)
        src, dst = (out, hist) if k % 2 == 0 else (hist, out)
        L.temporal_var_step_async(dev.handle, prev._state, prev._state if k else None, tp, frame.data_ptr(),
                                  src[1] if k else None, dst[1], None, None, stream)
    hist, out = out, hist  # four steps: the last wrote `out`
    dev.render_async(cam._state, L.make_params(w, h, 50, 4, 0.5, 2, pass_=4), frame.data_ptr(), None, stream)
    geometry = scene._geometry()
    lower = geometry.copy()
    lower[:, 1] -= 0.001
    same_t, lower_t = torch.from_numpy(geometry).cuda(), torch.from_numpy(lower).cuda()

    def motion_step(geo, plane):
        return lambda: L.temporal_motion_step_async(dev.handle, cam._state, prev._state, geo.data_ptr(), n, tp,
                                                    frame.data_ptr(), hist[1], out[1], variance.data_ptr(), plane,
                                                    record.data_ptr(), stream)

    calls = {
        "temporal_var_step_with_variance": lambda: L.temporal_var_step_async(
            dev.handle, cam._state, prev._state, tp, frame.data_ptr(), hist[1], out[1], variance.data_ptr(),
            record.data_ptr(), stream),
        "motion_step_none_moved": motion_step(same_t, None),
        "motion_step_all_moved": motion_step(lower_t, None),
        "motion_step_all_moved_with_motion_plane": motion_step(lower_t, motion.data_ptr()),
    }
    times = {name: [] for name in calls}
    fresh = {}
    for i in range(a.warmup + a.repeats):  # the arms alternate
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
            fresh[name] = int(record.cpu().numpy()[0])
    res = dict(width=w, height=h, rays_per_pixel=4, orbit_step_degrees=ray.ORBIT_STEP_DEGREES, repeats=a.repeats,
               warmup=a.warmup, device=torch.cuda.get_device_name(0), spheres=n,
               fresh_fraction={k: v / (w * h) for k, v in fresh.items()}, ms={})
    for name, ts in times.items():
        res["ms"][name] = dict(median=statistics.median(ts), min=min(ts), max=max(ts))
    base = res["ms"]["temporal_var_step_with_variance"]["median"]
    res["none_moved_over_var_step"] = res["ms"]["motion_step_none_moved"]["median"] / base
    res["all_moved_over_var_step"] = res["ms"]["motion_step_all_moved"]["median"] / base

    # the whole -bounce frame, wall clock, the arms alternating
    def tracer():
        t = ray.New(w, h)
        t.Camera = ray.RichSceneCamera()
        t.NumRaysPerPixel, t.MaxDepth, t.Seed = 4, 50, 2
        return t

    geos = torch.from_numpy(ray.Bounce(scene, a.frames)).cuda()
    wall = {"bounce_frame": [], "bounce_frame_temporal": []}
    for i in range(2 + a.repeats):
        for name, kw in (("bounce_frame", {}), ("bounce_frame_temporal", dict(temporal=True))):
            t = tracer()
            s = ray.RichScene(2)
            s._device_scene(0)  # the upload outside the timed interval
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.RenderAnimation(s, geos, **kw)
            torch.cuda.synchronize()
            if i >= 2:
                wall[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
            s._uploaded[0][1].release()
    for name, ts in wall.items():
        res["ms"][name] = dict(median=statistics.median(ts), min=min(ts), max=max(ts))
    res["bounce_frames"] = a.frames
    res["temporal_over_plain_bounce_frame"] = res["ms"]["bounce_frame_temporal"]["median"] / \
        res["ms"]["bounce_frame"]["median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
