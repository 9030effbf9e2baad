#!/usr/bin/env python3
"""Times of the progressive path (include/tray_progressive.h) on a C2-sized frame (book
cover, seed 2, 1280x720): the fold of 16 pass frames into a state that already holds one
(so the state is read and written: 24 * 16 + 96 bytes per pixel), the same fold with the
variance and the convergence record fused in (+ 24 bytes per pixel written), with the record
alone, the same Welford update written as plain torch element-wise operations on the same
device tensors (what a user would compose today; its result is checked to have the same
bits first), and the variance-guided filter beside tray_denoise_async on the folded mean, per
call and per level (level i = the call with i + 1 iterations minus the call with i).

All jobs alternate inside one process; each is timed with device events after a warm-up, as
the median over --repeats windows of --inner back-to-back calls. Prints one JSON line and
writes it to --out:

    python tools/progressive_bench.py [--repeats 15] [--out profiles/progressive_bench_c2.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 16
HBM_GB_S = 6300.0  # the achievable HBM bandwidth the fold is compared with (float4 copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--r", type=int, default=4, help="rays per pixel of each pass")
    ap.add_argument("--out", default="profiles/progressive_bench_c2.json")
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
    stack = torch.empty((FRAMES + 1, H, W, 3), **f64)
    dev.render_passes_async(cam._state, p, FRAMES + 1, stack.data_ptr(), stream)
    albedo, normal, depth_buf = torch.empty((H, W, 3), **f64), torch.empty((H, W, 3), **f64), torch.empty((H, W), **f64)
    dev.render_aov_async(cam._state, p, albedo.data_ptr(), normal.data_ptr(), depth_buf.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    dev.release()
    frames = stack[1:]
    mean1, m21 = torch.empty((H, W, 3), **f64), torch.empty((H, W, 3), **f64)  # the state after frame 0
    acc = _lib.Accum(mean1.data_ptr(), m21.data_ptr(), W, H, 0, 0)
    _lib.accum_fold_async(acc, stack.data_ptr(), 1, 0, stream)
    mean, m2, variance = (torch.empty((H, W, 3), **f64) for _ in range(3))
    record = torch.empty((2,), **f64)
    mp = _lib.accum_metric_params()

    def fold(var_ptr=None, rec_ptr=None, metric=True):
        def job():
            mean.copy_(mean1)  # not timed apart: see `state_copy`, subtracted below
            m2.copy_(m21)
            a = _lib.Accum(mean.data_ptr(), m2.data_ptr(), W, H, 1, 0)
            if metric:
                _lib.accum_fold_metric_async(a, frames.data_ptr(), FRAMES, mp, var_ptr, rec_ptr, 0, stream)
            else:
                _lib.accum_fold_async(a, frames.data_ptr(), FRAMES, 0, stream)
        return job

    def state_copy():
        mean.copy_(mean1)
        m2.copy_(m21)

    t_out = {}
    # Divisors as device scalars: torch turns a division by a host scalar into a multiplication by
    # its reciprocal, which rounds differently from the contract's t / n.
    counts = [torch.tensor(float(k + 2), **f64) for k in range(FRAMES)]
    pairs = torch.tensor(float(FRAMES + 1) * float(FRAMES), **f64)

    def torch_welford():
        mu, s = mean1, m21
        for k in range(FRAMES):
            x = frames[k]
            t = x - mu
            mu = mu + t / counts[k]
            s = s + t * (x - mu)
        t_out["mean"], t_out["m2"] = mu, s

    def torch_welford_metric():
        torch_welford()
        var = t_out["m2"] / pairs
        v = (var[..., 0] + var[..., 1]) + var[..., 2]
        mu = t_out["mean"]
        e = (mu[..., 0] * mu[..., 0] + mu[..., 1] * mu[..., 1]) + mu[..., 2] * mu[..., 2]
        m = torch.where(e > mp.floor, e, torch.full_like(e, mp.floor))
        t_out["variance"] = var
        t_out["unconverged"] = (~(v <= (mp.tolerance * mp.tolerance) * m)).sum()
        t_out["max_ratio"] = (v / m).max()

    # the outputs are equal before anything is timed
    fold(variance.data_ptr(), record.data_ptr())()
    torch_welford_metric()
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))  # noqa: E731
    assert same(mean, t_out["mean"]) and same(m2, t_out["m2"]), "torch's Welford differs from the fold"
    assert same(variance, t_out["variance"]), "torch's variance differs"
    rec = record.cpu().numpy().view(_lib.ACCUM_METRIC_DTYPE)[0]
    assert int(rec["unconverged"]) == int(t_out["unconverged"]) and float(rec["max_ratio"]) == float(t_out["max_ratio"])
    folded = mean.clone()

    vp = {it: _lib.denoise_variance_params(W, H, iterations=it) for it in range(1, 6)}
    dp = {it: _lib.denoise_params(W, H, iterations=it) for it in range(1, 6)}
    need = _lib.denoise_variance_workspace_bytes(vp[5])
    work = torch.empty((need // 8,), **f64)
    out, vout = torch.empty((H, W, 3), **f64), torch.empty((H, W), **f64)

    def guided(it, plane=True):
        return lambda: _lib.denoise_variance_async(folded.data_ptr(), variance.data_ptr(), vp[it], out.data_ptr(),
                                                   work.data_ptr(), need, albedo.data_ptr(), normal.data_ptr(),
                                                   depth_buf.data_ptr(), vout.data_ptr() if plane else None, 0, stream)

    def plain(it):
        return lambda: _lib.denoise_async(folded.data_ptr(), dp[it], out.data_ptr(), work.data_ptr(), need,
                                          albedo.data_ptr(), normal.data_ptr(), depth_buf.data_ptr(), 0, stream)

    jobs = {"state_copy": state_copy, "fold": fold(metric=False), "fold_record": fold(None, record.data_ptr()),
            "fold_variance_record": fold(variance.data_ptr(), record.data_ptr()), "torch_welford": torch_welford,
            "torch_welford_metric": torch_welford_metric}
    jobs.update({f"guided_{it}": guided(it) for it in vp})
    jobs.update({f"plain_{it}": plain(it) for it in dp})
    jobs["guided_5_no_variance_out"] = guided(5, plane=False)
    for job in jobs.values():
        job()
        job()
    torch.cuda.synchronize()
    times = {k: [] for k in jobs}
    for _ in range(args.repeats):
        for name, job in jobs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.inner):
                job()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.inner)
    ms = {k: statistics.median(v) for k, v in times.items()}
    for k in ("fold", "fold_record", "fold_variance_record"):  # each call re-made its state first
        ms[k + "_kernel"] = ms[k] - ms["state_copy"]

    def levels(prefix):
        return [ms[f"{prefix}_1"]] + [ms[f"{prefix}_{it + 1}"] - ms[f"{prefix}_{it}"] for it in range(1, 5)]

    pixels = W * H
    fold_bytes = pixels * (24 * FRAMES + 96)
    res = {
        "scene": label.split(" 1280")[0], "width": W, "height": H, "frames": FRAMES, "rays_per_pixel": args.r,
        "repeats": args.repeats, "inner": args.inner,
        "ms": {k: round(v, 4) for k, v in ms.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
        "fold_bytes": fold_bytes,
        "fold_gb_s": round(fold_bytes / ms["fold_kernel"] / 1e6, 1),
        "fold_fraction_of_hbm": round(fold_bytes / ms["fold_kernel"] / 1e6 / HBM_GB_S, 3),
        "fold_variance_record_gb_s": round((fold_bytes + 24 * pixels) / ms["fold_variance_record_kernel"] / 1e6, 1),
        "torch_over_fold": round(ms["torch_welford"] / ms["fold_kernel"], 2),
        "torch_metric_over_fold_variance_record": round(ms["torch_welford_metric"] / ms["fold_variance_record_kernel"], 2),
        "guided_ms": round(ms["guided_5"], 4), "plain_ms": round(ms["plain_5"], 4),
        "guided_over_plain": round(ms["guided_5"] / ms["plain_5"], 3),
        "guided_level_ms": [round(v, 4) for v in levels("guided")],
        "plain_level_ms": [round(v, 4) for v in levels("plain")],
        "unconverged": int(rec["unconverged"]), "max_ratio": float(rec["max_ratio"]),
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
