"""What an in-place scene update (include/tray_scene_update.h) costs and what it buys, on the book
cover (C2, 486 spheres) or the dense variant (C5, 1,939 spheres). DESIGN.md 8u.

(a) New geometry that lives in DEVICE memory, made the scene's: one tray_scene_update_async and a
    stream synchronise, against what the library offered before: a device-to-host copy of the
    geometry, tray_scene_release and tray_scene_upload (which ends in a synchronous copy). Host clock
    around each arm, both ending with the device idle; the arms alternate within one process. The
    update's own device time (events around the launch) is given beside it.
(b) The price of keeping the old topology: the 1280 x 720, r = 16 render (device events around one
    tray_render_async, candidate lists and work order warm) on the tree refitted to the moved spheres
    against the same geometry freshly uploaded, for the motions of tests/scene_update_cases.py,
    alternating. The frames are compared bit for bit first.

Medians, minima and maxima over --repeats after --warmup.

    python tools/scene_update_bench.py [--scene c2|c5] [--out profiles/scene_update_bench_c2.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SCENES = {"c2": (2, 11), "c5": (7, 22)}  # tray_rich_scene's seed and half extent


def stats(times):
    return dict(median=statistics.median(times), min=min(times), max=max(times))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(SCENES), default="c2")
    ap.add_argument("--out", default=None)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--rays", type=int, default=16)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)
    out_path = a.out or os.path.join(ROOT, "profiles", f"scene_update_bench_{a.scene}.json")
    import torch

    import scene_update_cases as C
    from tray_amd import _lib as L
    from tray_amd import ray

    w, h = a.width, a.height
    A = ray.rich_scene_array(*SCENES[a.scene])
    bg = ray._background(ray.DefaultBackground())
    cam = ray.RichSceneCamera()
    cam.Initialize(w, h)
    stream = torch.cuda.current_stream().cuda_stream
    params = L.make_params(w, h, a.depth, a.rays, 0.5, 2)
    out = dict(scene=a.scene, n_spheres=len(A), width=w, height=h, rays_per_pixel=a.rays, max_depth=a.depth,
               repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0), update_ms={}, render_ms={})

    # ---- (a) update in place against copy back + release + upload --------------------------------
    geos = [torch.from_numpy(C.geometry(m(A))).cuda() for m in (C.jitter, C.lift)]  # two targets in turn
    record = torch.zeros(4, dtype=torch.float64, device="cuda")
    dev_u = L.DeviceScene(A, bg, 0)
    info = dev_u.info()
    out.update(n_nodes=info.n_nodes, n_leaves=info.n_leaves, leaf_max=info.leaf_max, bound=info.bound)
    holder = [L.DeviceScene(A, bg, 0)]
    spheres = A.copy()

    def update(k):
        dev_u.update_async(geos[k & 1].data_ptr(), len(A), record.data_ptr(), stream)
        torch.cuda.current_stream().synchronize()

    def reupload(k):
        g = geos[k & 1].cpu().numpy()  # the copy back (synchronous)
        spheres["center"], spheres["radius"] = g[:, :3], g[:, 3]
        holder[0].release()
        holder[0] = L.DeviceScene(spheres, bg, 0)

    arms = dict(update_sync=update, copy_release_upload=reupload)
    times = {name: [] for name in arms}
    for k in range(a.warmup + a.repeats):
        for name, arm in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm(k)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                times[name].append(dt)
    assert record.cpu().numpy().view(L.SCENE_UPDATE_RECORD_DTYPE)[0]["applied"] == 1
    kernel = []
    for k in range(a.warmup + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev_u.update_async(geos[k & 1].data_ptr(), len(A), record.data_ptr(), stream)
        e1.record()
        e1.synchronize()
        if k >= a.warmup:
            kernel.append(e0.elapsed_time(e1))
    out["update_ms"] = {name: stats(t) for name, t in times.items()}
    out["update_ms"]["update_device_events"] = stats(kernel)
    out["update_speedup"] = out["update_ms"]["copy_release_upload"]["median"] / out["update_ms"]["update_sync"]["median"]
    holder[0].release()

    # ---- (b) the render on the refitted tree against a fresh tree ---------------------------------
    frame = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    other = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    for motion in ("jitter", "lift", "perm"):
        B = C.MOTIONS[motion](A)
        target = torch.from_numpy(C.geometry(B)).cuda()
        dev_u.update_async(target.data_ptr(), len(A), record.data_ptr(), stream)
        torch.cuda.synchronize()
        dev_f = L.DeviceScene(B, bg, 0)
        dev_u.render_async(cam._state, params, frame.data_ptr(), None, stream)
        dev_f.render_async(cam._state, params, other.data_ptr(), None, stream)
        torch.cuda.synchronize()
        same = bool((frame.view(torch.int64) == other.view(torch.int64)).all().item())
        scenes = dict(refitted=dev_u, fresh=dev_f)
        times = {name: [] for name in scenes}
        for k in range(a.warmup + a.repeats):
            for name, dev in scenes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dev.render_async(cam._state, params, frame.data_ptr(), None, stream)
                e1.record()
                e1.synchronize()
                if k >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
        fi = dev_f.info()
        out["render_ms"][motion] = dict(refitted=stats(times["refitted"]), fresh=stats(times["fresh"]),
                                        ratio=statistics.median(times["refitted"]) / statistics.median(times["fresh"]),
                                        same_bits=same, fresh_n_nodes=fi.n_nodes, fresh_leaf_max=fi.leaf_max)
        dev_f.release()
    dev_u.release()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
