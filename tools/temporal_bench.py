"""The cost of the temporal reprojection step (include/tray_temporal.h) on a C2-sized frame
(1280 x 720 book cover, r = 4), beside three other launches of the same run: the render of that
frame, tray_accum_fold_async of one frame (a comparable number of bytes: the floor) and
tray_scene_hit_async on the same width x height centre rays alone (only part of the step's work,
but it reads 48 B and stores 64 B per ray). Device-event times of single launches after a warm-up:
median, minimum and maximum over --repeats. DESIGN.md 8q.

    python tools/temporal_bench.py [--out profiles/temporal_bench_c2.json] [--repeats 30] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench_c2.json"))
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", type=float, default=None, help="degrees between the two cameras")
    a = ap.parse_args(argv)
    import torch

    import temporal_ref as R
    from tray_amd import _lib as L
    from tray_amd import ray

    w, h = a.width, a.height
    step = ray.ORBIT_STEP_DEGREES if a.step is None else a.step
    prev, cam = ray.RichSceneCamera(), ray.Orbit(ray.RichSceneCamera(), step)
    prev.Initialize(w, h), cam.Initialize(w, h)
    scene = ray.RichScene(2)
    scene.Background = ray.DefaultBackground()
    dev = scene._device_scene(0)
    stream = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device="cuda")

    def planes():
        t = [torch.empty((h, w, 3), **f64), torch.empty((h, w), dtype=torch.int32, device="cuda"),
             torch.empty((h, w), dtype=torch.int32, device="cuda"), torch.empty((h, w), **f64)]
        return t, L.TemporalState(*(x.data_ptr() for x in t), w, h)

    states = [planes(), planes()]
    frame = torch.empty((h, w, 3), **f64)
    record = torch.zeros((2,), dtype=torch.int64, device="cuda")
    tp = L.temporal_params()
    params = [L.make_params(w, h, 50, 4, 0.5, 2, pass_=k) for k in range(2)]
    # frame 0 of the previous camera is the history of every timed step
    dev.render_async(prev._state, params[0], frame.data_ptr(), None, stream)
    L.temporal_step_async(dev.handle, prev._state, None, tp, frame.data_ptr(), None, states[0][1], None, stream)
    dev.render_async(cam._state, params[1], frame.data_ptr(), None, stream)
    o, d = R.centre_rays(cam._state.as_array(), w, h)
    rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.broadcast_to(o, d.shape), d], -1))).cuda()
    hits = torch.empty((h * w, 8), **f64)
    mean, m2 = torch.zeros((h, w, 3), **f64), torch.zeros((h, w, 3), **f64)

    def fold():
        L.accum_fold_async(L.Accum(mean.data_ptr(), m2.data_ptr(), w, h, 1, 0), frame.data_ptr(), 1, 0, stream)

    calls = {
        "render_r4": lambda: dev.render_async(cam._state, params[1], frame.data_ptr(), None, stream),
        "temporal_step": lambda: L.temporal_step_async(dev.handle, cam._state, prev._state, tp, frame.data_ptr(),
                                                       states[0][1], states[1][1], record.data_ptr(), stream),
        "temporal_step_first_frame": lambda: L.temporal_step_async(dev.handle, cam._state, None, tp, frame.data_ptr(),
                                                                   None, states[1][1], None, stream),
        "accum_fold_1": fold,
        "scene_hit_centre_rays": lambda: dev.hit_async(rays.data_ptr(), h * w, hits.data_ptr(), stream=stream),
    }
    out = dict(width=w, height=h, rays_per_pixel=4, orbit_step_degrees=step, repeats=a.repeats, warmup=a.warmup,
               device=torch.cuda.get_device_name(0), ms={})
    for name, call in calls.items():
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        out["ms"][name] = dict(median=statistics.median(times), min=min(times), max=max(times))
    rec = record.cpu().numpy()
    out["fresh_fraction"] = float(rec[0]) / (w * h)
    m = out["ms"]
    out["hit_plus_fold_ms"] = m["scene_hit_centre_rays"]["median"] + m["accum_fold_1"]["median"]
    out["step_below_hit_plus_fold"] = bool(m["temporal_step"]["median"] < out["hit_plus_fold_ms"])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
