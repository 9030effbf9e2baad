"""The cost of carrying M2 through the temporal reprojection step and of the refill chain
(include/tray_temporal_variance.h) on a C2-sized frame (1280 x 720 book cover, r = 4, one orbit step
of 1 degree), all in one process: the new step with and without the variance plane beside the
version-1 step on the same history, the variance of the listed pixels and of the whole frame, the
selection, the list render and the sparse fold at the measured fresh fraction (the list the
selection gives for R = --refill), and the frame's render. Device-event times of single launches
(the selection: its four) after a warm-up: median, minimum and maximum over --repeats. DESIGN.md 8s.

    python tools/temporal_variance_bench.py [--out profiles/temporal_variance_bench_c2.json] [--repeats 30]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_variance_bench_c2.json"))
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--refill", type=int, default=None, help="R of the chain (default: the CLI's)")
    ap.add_argument("--step", type=float, default=None, help="degrees between the two cameras")
    a = ap.parse_args(argv)
    import torch

    from tray_amd import _lib as L
    from tray_amd import ray

    w, h = a.width, a.height
    refill = ray.REFILL_DEFAULT if a.refill is None else a.refill
    step = ray.ORBIT_STEP_DEGREES if a.step is None else a.step
    prev, cam = ray.RichSceneCamera(), ray.Orbit(ray.RichSceneCamera(), step)
    prev.Initialize(w, h), cam.Initialize(w, h)
    scene = ray.RichScene(2)
    scene.Background = ray.DefaultBackground()
    dev = scene._device_scene(0)
    stream = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")

    def planes():
        t = dict(colour=torch.empty((h, w, 3), **f64), m2=torch.zeros((h, w, 3), **f64), age=torch.empty((h, w), **i32),
                 index=torch.empty((h, w), **i32), depth=torch.empty((h, w), **f64))
        return (t, L.TemporalVarState(*(t[n].data_ptr() for n in ("colour", "m2", "age", "index", "depth")), w, h),
                L.TemporalState(*(t[n].data_ptr() for n in ("colour", "age", "index", "depth")), w, h))

    hist, out = planes(), planes()
    frame, variance = torch.empty((h, w, 3), **f64), torch.empty((h, w, 3), **f64)
    record = torch.zeros((2,), dtype=torch.int64, device="cuda")
    tp = L.temporal_params()
    stride = 1 + refill
    params = [L.make_params(w, h, 50, 4, 0.5, 2, pass_=k) for k in (0, stride, stride + 1)]
    # The history of every timed step: the previous camera's frame 0 after its own refill (every pixel
    # holds 1 + R frames, as in a running sequence), here simply 1 + R uniform passes folded by the step.
    for k in range(stride):
        dev.render_async(prev._state, L.make_params(w, h, 50, 4, 0.5, 2, pass_=k), frame.data_ptr(), None, stream)
        src, dst = (out, hist) if k % 2 == 0 else (hist, out)
        L.temporal_var_step_async(dev.handle, prev._state, prev._state if k else None, tp, frame.data_ptr(),
                                  src[1] if k else None, dst[1], None, None, stream)
    if stride % 2 == 0:  # the last step wrote `out`: the history is there
        hist, out = out, hist
    dev.render_async(cam._state, params[1], frame.data_ptr(), None, stream)
    # One untimed step and selection give the fresh fraction and the list; the timed selection, list
    # render and list variance then run on `out` as the step leaves it (the step is timed before them
    # and writes the same values every time).
    L.temporal_var_step_async(dev.handle, cam._state, prev._state, tp, frame.data_ptr(), hist[1], out[1],
                              variance.data_ptr(), record.data_ptr(), stream)
    ap_ = L.adaptive_params(tolerance=1e150, min_passes=stride, max_passes=int(tp.max_history), dilate=1)
    nbytes = L.adaptive_workspace_bytes(w, h)
    work = torch.empty((nbytes // 8,), **f64)
    active = torch.empty((h * w,), **i32)
    arecord = torch.empty((4,), **f64)
    ast = out[1].adaptive()

    def select():
        L.adaptive_select_async(ast, ap_, active.data_ptr(), arecord.data_ptr(), work.data_ptr(), nbytes, None, 0,
                                stream)

    select()
    n_active = int(arecord.cpu().numpy().view(L.ADAPTIVE_RECORD_DTYPE)[0]["n_active"])
    fresh = int(record.cpu().numpy()[0])
    values = torch.empty((max(refill, 1) * max(n_active, 1) * 3,), **f64)
    # the fold moves the state it is timed on, so it runs on a scratch copy whose ages are reset each time
    scratch = planes()
    for n in scratch[0]:
        scratch[0][n].copy_(out[0][n])
    sst = scratch[1].adaptive()
    age0 = out[0]["age"].clone()

    def fold():
        L.adaptive_fold_async(sst, active.data_ptr(), n_active, values.data_ptr(), refill, 0, stream)

    calls = {
        "render_r4": lambda: dev.render_async(cam._state, params[1], frame.data_ptr(), None, stream),
        "temporal_step_v1": lambda: L.temporal_step_async(dev.handle, cam._state, prev._state, tp, frame.data_ptr(),
                                                          hist[2], out[2], record.data_ptr(), stream),
        "temporal_var_step": lambda: L.temporal_var_step_async(dev.handle, cam._state, prev._state, tp,
                                                               frame.data_ptr(), hist[1], out[1], None,
                                                               record.data_ptr(), stream),
        "temporal_var_step_with_variance": lambda: L.temporal_var_step_async(
            dev.handle, cam._state, prev._state, tp, frame.data_ptr(), hist[1], out[1], variance.data_ptr(),
            record.data_ptr(), stream),
        "variance_whole_frame": lambda: L.temporal_var_variance_async(out[1], None, 0, variance.data_ptr(), 0, stream),
        "select": select,
    }
    if n_active and refill:
        calls.update({
            "variance_list": lambda: L.temporal_var_variance_async(out[1], active.data_ptr(), n_active,
                                                                   variance.data_ptr(), 0, stream),
            "render_pixels": lambda: dev.render_pixels_async(cam._state, params[2], active.data_ptr(), n_active,
                                                             values.data_ptr(), refill, stream=stream),
            "adaptive_fold": fold,
        })
    res = dict(width=w, height=h, rays_per_pixel=4, orbit_step_degrees=step, refill=refill, repeats=a.repeats,
               warmup=a.warmup, device=torch.cuda.get_device_name(0), fresh_fraction=fresh / (w * h),
               n_active=n_active, active_fraction=n_active / (w * h), ms={})
    for name, call in calls.items():
        times = []
        for i in range(a.warmup + a.repeats):
            if name == "adaptive_fold":
                scratch[0]["age"].copy_(age0)  # outside the timed interval
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        res["ms"][name] = dict(median=statistics.median(times), min=min(times), max=max(times))
    m = {k: v["median"] for k, v in res["ms"].items()}
    res["var_step_over_v1"] = m["temporal_var_step"] / m["temporal_step_v1"]
    res["var_step_with_variance_over_v1"] = m["temporal_var_step_with_variance"] / m["temporal_step_v1"]
    res["chain_ms"] = sum(m.get(k, 0.0) for k in ("select", "render_pixels", "adaptive_fold", "variance_list"))
    res["frame_ms_without_refill"] = m["render_r4"] + m["temporal_var_step_with_variance"]
    res["frame_ms_with_refill"] = res["frame_ms_without_refill"] + res["chain_ms"]
    # frame 0 lists every pixel: R passes of the whole frame through the list renderer
    every = torch.arange(h * w, **i32)
    big = torch.empty((max(refill, 1) * h * w * 3,), **f64)
    if refill:
        times = []
        for i in range(2 + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dev.render_pixels_async(cam._state, params[2], every.data_ptr(), h * w, big.data_ptr(), refill,
                                    stream=stream)
            e1.record()
            e1.synchronize()
            if i >= 2:
                times.append(e0.elapsed_time(e1))
        res["ms"]["render_pixels_frame_0_every_pixel"] = dict(median=statistics.median(times), min=min(times),
                                                              max=max(times))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
