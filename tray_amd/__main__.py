"""Render the book-cover scene to a PNG through the MI355X path: the flags of the
reference's benchmark binary (benchmark/benchmark.go:37-47; -w and -profile-cpu
have no meaning here).

    python -m tray_amd [-width 1280] [-height 720] [-r 64] [-d 50] [-seed 2] [-save out.png]
    python -m tray_amd -ansi [-s 4] ...   # main.go's terminal view, non-interactive (-exit)
    python -m tray_amd -aov PREFIX ...    # also the first-hit feature buffers (include/tray_aov.h)
    python -m tray_amd -denoise -r 16 ... # the frame filtered on the device (include/tray_denoise.h)
    python -m tray_amd -r 16 -passes 64 [-tolerance T] [-denoise] ...  # progressive: passes of -r rays until
                                          # the frame has converged (include/tray_progressive.h)
    python -m tray_amd -r 16 -passes 64 -adaptive [-denoise] ...  # the same, rendering only the pixels
                                          # that have not converged yet (include/tray_adaptive.h)
    python -m tray_amd -r 4 -orbit 8 [-orbit-step DEG] [-denoise] ...  # a camera orbit that reuses each
                                          # last frame by temporal reprojection (include/tray_temporal.h)
    python -m tray_amd -r 4 -orbit 8 -variance [-refill [R]] [-denoise] ...  # the same, carrying M2: R more passes
                                          # for the fresh pixels of each frame, and the variance-guided filter
                                          # (include/tray_temporal_variance.h)
    python -m tray_amd -r 16 -bounce 8 [-denoise] ...  # the small spheres hop: one upload, then per frame the
                                          # spheres moved and the BVH refitted on the device
                                          # (include/tray_scene_update.h)
    python -m tray_amd -r 4 -bounce 8 -temporal [-variance] [-refill [R]] [-denoise] ...  # the same, each frame
                                          # reusing the last: the history follows the hopping spheres
                                          # (include/tray_temporal_motion.h)
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from . import _lib, png, ray, terminal


def _srgba(rgb: np.ndarray) -> np.ndarray:
    """ColorF.ToSRGBA of an (H, W, 3) float64 image (the host encoder of include/tray.h)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    rgba = np.zeros(rgb.shape[:2] + (4,), dtype=np.uint8)
    _lib.check(_lib.lib().tray_to_srgba(rgb.ctypes.data, rgb.shape[0] * rgb.shape[1], rgba.ctypes.data))
    return rgba


def save_aov(prefix: str, aov: dict) -> None:
    """PREFIX.npz with the five arrays of Tracer.RenderAOV, and the two guide images a
    denoiser takes as PNGs: the albedo, and the normal mapped to colours by 0.5 n + 0.5."""
    np.savez(prefix + ".npz", **aov)
    png.save_png(prefix + "_albedo.png", _srgba(aov["albedo"]))
    png.save_png(prefix + "_normal.png", _srgba(0.5 * aov["normal"] + 0.5))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m tray_amd")
    ap.add_argument("-width", type=int, default=1280)
    ap.add_argument("-height", type=int, default=720)
    ap.add_argument("-r", type=int, default=64, help="rays per pixel")
    ap.add_argument("-d", type=int, default=50, help="max depth")
    ap.add_argument("-seed", type=int, default=2)
    ap.add_argument("-save", default="out.png", help="output PNG ('' to skip)")
    ap.add_argument("-aov", default="", metavar="PREFIX",
                    help="also write the first-hit feature buffers: PREFIX.npz, PREFIX_albedo.png, PREFIX_normal.png")
    ap.add_argument("-denoise", action="store_true",
                    help="save the frame after the guided a-trous filter (include/tray_denoise.h); "
                         "with -aov also PREFIX_denoised.png")
    ap.add_argument("-passes", type=int, default=0, metavar="N",
                    help="render progressively: up to N passes of -r rays each, folded on the device, until no "
                         "pixel is left unconverged (include/tray_progressive.h); with -denoise the "
                         "variance-guided filter")
    ap.add_argument("-tolerance", type=float, default=None, metavar="T",
                    help="with -passes: the relative standard error at which a pixel counts as converged "
                         "(default: the library's, 0.05)")
    ap.add_argument("-adaptive", action="store_true",
                    help="with -passes: render only the unconverged pixels after a uniform warm-up "
                         "(include/tray_adaptive.h); prints the pixel-passes spent against h x w x passes")
    ap.add_argument("-orbit", type=int, default=0, metavar="N",
                    help="render N frames turning the camera about LookAt around the up axis, each reusing the "
                         "last through temporal reprojection (include/tray_temporal.h); prints the fresh fraction "
                         "and the mean age per frame and saves the last frame; -denoise applies")
    ap.add_argument("-orbit-step", type=float, default=ray.ORBIT_STEP_DEGREES, metavar="DEG", dest="orbit_step",
                    help="with -orbit: degrees between frames")
    ap.add_argument("-variance", action="store_true",
                    help="with -orbit or -bounce -temporal: carry M2 with the colour "
                         "(include/tray_temporal_variance.h); -denoise is then the variance-guided filter")
    ap.add_argument("-refill", type=int, nargs="?", default=0, const=ray.REFILL_DEFAULT, metavar="R",
                    help="with -orbit -variance or -bounce -temporal -variance: R more passes per frame for the pixels "
                         "that hold fewer than 1 + R "
                         f"frames and their neighbours (default R when given without a number: {ray.REFILL_DEFAULT}); "
                         "prints the refilled pixels per frame")
    ap.add_argument("-bounce", type=int, default=0, metavar="N",
                    help="render N frames in which the small spheres hop (y = R + |sin| of a phase per sphere), "
                         "moved in place on the device with the BVH refitted (include/tray_scene_update.h); prints "
                         "per frame whether the update was applied and saves the last frame; -denoise applies")
    ap.add_argument("-temporal", action="store_true",
                    help="with -bounce: each frame reuses the last through temporal reprojection that follows the "
                         "moved spheres (include/tray_temporal_motion.h); prints the fresh fraction and the mean age "
                         "per frame; -variance, -refill and -denoise apply as with -orbit")
    ap.add_argument("-ansi", action="store_true",
                    help="render at -s x the terminal size and draw it in the terminal (main.go:86-131)")
    ap.add_argument("-s", type=float, default=4, help="supersampling factor of -ansi")
    a = ap.parse_args(argv)
    if a.ansi:
        a.width, a.height = terminal.image_size(*terminal.terminal_size(), a.s)
    t = ray.New(a.width, a.height)
    t.Camera = ray.RichSceneCamera()
    t.NumRaysPerPixel, t.MaxDepth, t.Seed = a.r, a.d, a.seed
    scene = ray.RichScene(a.seed)
    t0 = time.perf_counter()
    samples = a.width * a.height * a.r
    if a.orbit < 0 or (a.orbit and (a.passes or a.adaptive)):
        ap.error("-orbit needs N >= 1 and goes with neither -passes nor -adaptive")
    if a.temporal and not a.bounce:
        ap.error("-temporal goes with -bounce N")
    if (a.variance or a.refill) and not (a.orbit or a.temporal):
        ap.error("-variance and -refill go with -orbit N or -bounce N -temporal")
    if a.refill < 0 or (a.refill and not a.variance):
        ap.error("-refill needs R >= 0 and -variance")
    if a.bounce < 0 or (a.bounce and (a.orbit or a.passes or a.adaptive)):
        ap.error("-bounce needs N >= 1 and goes with none of -orbit, -passes and -adaptive")
    if a.bounce and a.temporal:
        img = t.RenderAnimation(scene, ray.Bounce(scene, a.bounce), denoise=a.denoise, temporal=True,
                                variance=a.variance, refill=a.refill)[-1]
        refilled = t.refilled if a.variance else [None] * a.bounce
        for k, (fresh, age, n) in enumerate(zip(t.fresh, t.mean_age, refilled)):
            print(f"frame {k}: fresh {fresh / max(a.width * a.height, 1):.4f} mean age {age:.3f}" +
                  (f" refilled {n}" if a.variance else ""))
        samples *= t.pixel_passes / max(a.width * a.height, 1) if a.variance else a.bounce
    elif a.bounce:
        img = t.RenderAnimation(scene, ray.Bounce(scene, a.bounce), denoise=a.denoise)[-1]
        for k, applied in enumerate(t.applied):
            print(f"frame {k}: {'moved in place' if applied else 'refused: uploaded afresh'}")
        samples *= a.bounce
    elif a.orbit:
        cameras = [ray.Orbit(t.Camera, k * a.orbit_step) for k in range(a.orbit)]
        if a.variance:
            img = t.RenderSequence(scene, cameras, denoise=a.denoise, variance=True, refill=a.refill)[-1]
            for k, (fresh, age, n) in enumerate(zip(t.fresh, t.mean_age, t.refilled)):
                print(f"frame {k}: fresh {fresh / max(a.width * a.height, 1):.4f} mean age {age:.3f} refilled {n}")
            samples *= t.pixel_passes / max(a.width * a.height, 1)
        else:
            img = t.RenderSequence(scene, cameras, denoise=a.denoise)[-1]
            for k, (fresh, age) in enumerate(zip(t.fresh, t.mean_age)):
                print(f"frame {k}: fresh {fresh / max(a.width * a.height, 1):.4f} mean age {age:.3f}")
            samples *= a.orbit
    elif a.adaptive:
        if a.passes <= 0:
            ap.error("-adaptive needs -passes N")
        img = t.RenderAdaptive(scene, a.passes, tolerance=a.tolerance, denoise=a.denoise)
        samples *= t.pixel_passes / max(a.width * a.height, 1)
        print(f"adaptive: {t.pixel_passes} pixel-passes of r={a.r} against {a.width * a.height * a.passes} "
              f"(h x w x passes), at most {t.passes} in a pixel, {t.unconverged} of {a.width * a.height} pixels "
              f"unconverged, worst relative error {t.max_ratio ** 0.5:.4g}")
    elif a.passes > 0:
        img = t.RenderProgressive(scene, a.passes, tolerance=a.tolerance, denoise=a.denoise)
        print(f"progressive: {t.passes} passes of r={a.r} done, {t.unconverged} of {a.width * a.height} pixels "
              f"unconverged, worst relative error {t.max_ratio ** 0.5:.4g}")
        samples *= t.passes
    else:
        img = t.RenderDenoised(scene) if a.denoise else t.Render(scene)
    dt = time.perf_counter() - t0
    print(f"rendered {a.width}x{a.height} r={a.r} d={a.d}{' denoised' if a.denoise else ''} "
          f"({len(scene.Objects)} objects) in {dt:.3f} s: {samples / dt / 1e6:.1f} Mrays/s end to end",
          file=sys.stderr)
    if a.save:
        png.save_png(a.save, img)
    if a.aov:
        save_aov(a.aov, t.RenderAOV(scene))
        if a.denoise:
            png.save_png(a.aov + "_denoised.png", img)
    if a.ansi:
        cols, rows = terminal.terminal_size()
        print(terminal.ansi_halfblocks(terminal.scale_image(img, cols, rows * 2, a.s)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
