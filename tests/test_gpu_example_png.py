"""The HIP renderer against the reference's example.png past the first hit, under
the rules of tests/example_png.py (fixtures: tests/golden/make_example_pins.py).
No oracle call: the fixtures, make_example_pins.analytic_color and the Go
binary's bytes are the only references.

Metal cap: 72,347 pixels of rows 55..278 whose whole camera footprint reflects
off the Metal{Fuzz: 0} sphere at (4,1,0) into the sky in ANY RichScene, so every
sample is Sphere.Hit -> SetFaceNormal -> Metal.Scatter -> Mul(albedo, sky).
Lambertian cap: 3,515 pixels of the (-4,1,0) sphere above y = 1.5 (rows
59..111), pinned by their mean. The glass sphere's cap is no pin (its mean
moves by +-5 bytes with the scene) and is left out. Every render is the band of
rows 55..278 (1280 x 224).

Bounds (tests/example_png.py; the fixture's numpy restatement over 4 jitter
seeds differs from example.png in 2,639..2,642 channels, bias <= 0.00392):
  (c) exemption within 0.04 + 0.2 x footprint spread of a rounding boundary;
  (d) exempt share <= 0.40; (e) differing channels <= 1.25 x 2,642 = 3,302;
  (f) |bias| <= 3 x 0.00392 = 0.0118 bytes on the mask and its quadrants;
  Lambertian cap: SE = 0.0357 / 0.0262 / 0.0221, S = 0.1605 / 0.0674 / 0.0987,
  T = 5 SE + S = 0.339 / 0.198 / 0.209 bytes (R / G / B).
Measured on the C oracle (seed 2, test_example_png_cpu.py): exempt share 0.3634,
2,654 differing channels (96.41 % of pixels exact), worst miss at 0.080 x
spread past 0.04, bias +0.0005 / -0.0028 (worst quadrant 0.0038), pinhole frame
1,828 differing channels; cap mean 121.86 / 102.33 / 85.76 for example.png's
121.77 / 102.34 / 85.75.
"""
import numpy as np
import pytest

import example_png as E
from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_parity import bg_struct, camera, gpu_render
from test_gpu_query import device_camera_rays, device_colors

pytestmark = pytest.mark.gpu

SEED = 2
FLAGS = [("bvh", 0), ("linear", 1)]


def to_bytes(L, lin):
    lin = np.ascontiguousarray(lin, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(lin), 4), dtype=np.uint8)
    L.check(L.lib().tray_to_srgba(lin.ctypes.data, len(lin), out.ctypes.data))
    return out[:, :3]


def band(L, scene, setup, spp, flags=0):
    """Rows METAL.y0..y1 - 1 of the 1280x720 frame: (linear, Scene.Hit counts)."""
    m = E.metal_cap()
    st = camera(L, setup, E.WIDTH, E.HEIGHT)
    return gpu_render(L, scene, DEFAULT_BG, st, E.WIDTH, E.HEIGHT, spp, E.DEPTH, E.RADIUS, SEED, y_start=m.y0,
                      y_end=m.y1, flags=flags)


@pytest.fixture(scope="module")
def scene2():
    from tray_amd import ray

    return ray.rich_scene_array(2)


@pytest.fixture(scope="module")
def frame2(L, scene2):
    """The seed-2 r=64 band through the BVH, shared and left unchanged."""
    lin, seg = band(L, scene2, RICH_SETUP, E.SPP)
    lin.setflags(write=False)
    seg.setflags(write=False)
    return lin, seg


@pytest.mark.parametrize("name,flags", FLAGS)
def test_metal_cap_r64(L, scene2, frame2, name, flags):
    """Rules (a)..(f) on the device's r=64 frame."""
    m = E.metal_cap()
    lin, seg = frame2 if flags == 0 else band(L, scene2, RICH_SETUP, E.SPP, L.FLAG_LINEAR_SCAN)
    E.check_metal_frame(lin[m.band], to_bytes(L, lin[m.band]), seg[m.band], f"device r=64 {name}")


@pytest.mark.parametrize("name,flags", FLAGS)
def test_metal_cap_pinhole(L, scene2, name, flags):
    """Rule (g): the pixel-centre pinhole frame is analytic_color bit for bit."""
    m = E.metal_cap()
    lin, seg = band(L, scene2, E.pinhole_setup(RICH_SETUP), 1, L.FLAG_LINEAR_SCAN if flags else 0)
    E.check_metal_pinhole(lin[m.band], to_bytes(L, lin[m.band]), seg[m.band], f"device pinhole {name}")


def test_metal_cap_is_scene_independent(L, frame2):
    """rich_scene(7) holds other small spheres; at the same RNG seed the mask's pixels do not move."""
    from tray_amd import ray

    m = E.metal_cap()
    lin7, seg7 = band(L, ray.rich_scene_array(7), RICH_SETUP, E.SPP)
    assert np.array_equal(seg7[m.band], frame2[1][m.band])
    assert np.array_equal(lin7[m.band].view(np.uint64), frame2[0][m.band].view(np.uint64))
    assert not np.array_equal(lin7, frame2[0])  # the scenes do differ elsewhere in the band


@pytest.mark.parametrize("name,flags", FLAGS)
def test_metal_cap_ray_query(L, scene2, name, flags):
    """CameraRays (r=1, pinhole) -> RayColor on the masked pixels' rays: analytic_color's bits, 2 Scene.Hit calls."""
    import torch

    m = E.metal_cap()
    st = camera(L, E.pinhole_setup(RICH_SETUP), E.WIDTH, E.HEIGHT)
    p = L.make_params(E.WIDTH, E.HEIGHT, E.DEPTH, 1, E.RADIUS, SEED, y_start=m.y0, y_end=m.y1)
    rays, ids = device_camera_rays(L, torch, st, p)
    sel = m.band.reshape(-1)
    rays = rays.cpu().numpy()[sel]
    ids = ids.cpu().numpy().view(np.uint32)[sel]
    assert np.array_equal(ids[:, 0], m.ys * E.WIDTH + m.xs) and not ids[:, 1].any()
    dev = L.DeviceScene(scene2, bg_struct(L, DEFAULT_BG), 0)
    try:
        rgb, seg = device_colors(L, torch, dev, rays, E.DEPTH, SEED, ids, L.FLAG_LINEAR_SCAN if flags else 0)
    finally:
        dev.release()
    want = E.pins.analytic_color(m.xs, m.ys)
    assert np.all(seg == 2)
    assert np.array_equal(rgb.view(np.uint64), want.view(np.uint64)), f"max {np.abs(rgb - want).max():.3e}"


def test_lambert_cap_mean(L, frame2):
    """The device's seed-2 frame: the cap's mean byte within T = 5 SE + S of example.png's."""
    m, c = E.metal_cap(), E.lambert_cap()
    assert m.y0 <= c.y0 and c.y1 <= m.y1  # the cap lies inside the shared band
    lin = frame2[0][c.y0 - m.y0:c.y1 - m.y0][c.band]
    E.check_lambert_mean(to_bytes(L, lin), "device")
