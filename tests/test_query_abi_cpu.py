"""include/tray_query.h on the CPU: the ray-query entry points are declared,
exported and bound, sit beside (not inside) the ABI 6 surface of tray.h, the
header is C99, and argument errors are reported before any device work. No
kernel is launched here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tray_query.h")
FAKE = 0x1000  # a non-null "device pointer": validation fails before anything could read it


def _declared():
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(HEADER).read(), re.M))


def test_query_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.QUERY_EXPORTS) and len(declared) == 4
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_query_version() == 1
    assert "#define TRAY_QUERY_VERSION 1" in open(HEADER).read()


def test_stable_header_unchanged_by_queries(L):
    """tray.h declares none of the query entry points and EXPORTS lists none."""
    stable = open(os.path.join(ROOT, "include", "tray.h")).read()
    for name in L.QUERY_EXPORTS:
        assert name not in stable
        assert name not in L.EXPORTS
    assert L.lib().tray_abi_version() == 6


def test_struct_sizes(L):
    assert ctypes.sizeof(L.Ray) == 48 and L.RAY_DTYPE.itemsize == 48
    assert ctypes.sizeof(L.Hit) == 64 and L.HIT_DTYPE.itemsize == 64
    assert L.HIT_DTYPE.fields["t"][1] == 48 and L.HIT_DTYPE.fields["index"][1] == 56
    assert L.HIT_DTYPE.fields["front_face"][1] == 60 and L.RAY_DTYPE.fields["direction"][1] == 24


def test_header_is_c99():
    """tests/c/tray_query_caller.c includes the header and calls every entry point
    (its typedefs also pin the struct sizes at compile time)."""
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c", "tray_query_caller.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _hit(L, scene=None, rays=FAKE, n=4, t_end=float("inf"), flags=0, hits=FAKE):
    return L.lib().tray_scene_hit_async(scene, rays, n, t_end, flags, hits, None)


def _color(L, scene=None, rays=FAKE, ids=None, n=4, depth=5, seed=1, flags=0, rgb=FAKE, seg=None):
    return L.lib().tray_ray_color_async(scene, rays, ids, n, depth, seed, flags, rgb, seg, None)


HIT_ERRORS = {
    "null_scene": (dict(), "TRAY_ERR_INVALID_ARGUMENT", b"null scene"),
    "null_rays": (dict(rays=None), "TRAY_ERR_INVALID_ARGUMENT", b"null ray buffer"),
    "null_hits": (dict(hits=None), "TRAY_ERR_INVALID_ARGUMENT", b"null result buffer"),
    "negative_n": (dict(n=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative"),
    "n_2_31": (dict(n=2**31), "TRAY_ERR_TOO_LARGE", b"2^31"),
    "unknown_flag": (dict(flags=4), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
    "ordered_sum_flag": (dict(flags=2), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
    "nan_t_end": (dict(t_end=float("nan")), "TRAY_ERR_INVALID_ARGUMENT", b"NaN"),
}


@pytest.mark.parametrize("case", sorted(HIT_ERRORS))
def test_scene_hit_argument_errors(L, case):
    kw, status, word = HIT_ERRORS[case]
    assert _hit(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


COLOR_ERRORS = {
    "null_scene": (dict(), "TRAY_ERR_INVALID_ARGUMENT", b"null scene"),
    "null_rays": (dict(rays=None), "TRAY_ERR_INVALID_ARGUMENT", b"null ray buffer"),
    "null_rgb": (dict(rgb=None), "TRAY_ERR_INVALID_ARGUMENT", b"null result buffer"),
    "negative_n": (dict(n=-7), "TRAY_ERR_INVALID_ARGUMENT", b"negative"),
    "n_2_31": (dict(n=2**31), "TRAY_ERR_TOO_LARGE", b"2^31"),
    "max_depth_0": (dict(depth=0), "TRAY_ERR_INVALID_ARGUMENT", b"max_depth"),
    "unknown_flag": (dict(flags=8), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
}


@pytest.mark.parametrize("case", sorted(COLOR_ERRORS))
def test_ray_color_argument_errors(L, case):
    kw, status, word = COLOR_ERRORS[case]
    assert _color(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_camera_rays_argument_errors(L):
    lib = L.lib()
    cam = L.CameraState()
    p = L.make_params(8, 8, 5, 2, 0.5, 1)
    inv, big = L.TRAY_ERR_INVALID_ARGUMENT, L.TRAY_ERR_TOO_LARGE
    assert lib.tray_camera_rays_async(None, ctypes.byref(p), 0, FAKE, None, None) == inv
    assert b"camera" in lib.tray_last_error()
    assert lib.tray_camera_rays_async(ctypes.byref(cam), None, 0, FAKE, None, None) == inv
    assert lib.tray_last_error()
    assert lib.tray_camera_rays_async(ctypes.byref(cam), ctypes.byref(p), 0, None, None, None) == inv
    assert b"null ray buffer" in lib.tray_last_error()
    bad = L.make_params(8, 8, 5, 0, 0.5, 1)
    assert lib.tray_camera_rays_async(ctypes.byref(cam), ctypes.byref(bad), 0, FAKE, None, None) == inv
    huge = L.make_params(4096, 4096, 5, 128, 0.5, 1)  # 2^31 rays
    assert lib.tray_camera_rays_async(ctypes.byref(cam), ctypes.byref(huge), 0, FAKE, None, None) == big
    assert b"2^31" in lib.tray_last_error()
    none = L.make_params(8, 8, 5, 2, 0.5, 1, y_start=3, y_end=3)  # an empty row set: nothing to launch
    assert lib.tray_camera_rays_async(ctypes.byref(cam), ctypes.byref(none), 0, None, None, None) == L.TRAY_OK
    assert L.camera_rays_count(p) == 128 and L.camera_rays_count(none) == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_camera_rays_without_device_fail_loudly(L):
    cam = L.CameraState()
    p = L.make_params(8, 8, 5, 2, 0.5, 1)
    assert L.lib().tray_camera_rays_async(ctypes.byref(cam), ctypes.byref(p), 0, FAKE, None, None) == L.TRAY_ERR_NO_DEVICE


def test_scene_hit_mirror_rejects_other_interval_starts(L):
    """Scene.Hit's interval start is the renderer's 1e-6: any other is refused before a device is touched."""
    from tray_amd import ray

    sc = ray.DefaultScene()
    for start in (0.0, 1e-3, -1.0):
        with pytest.raises(L.TrayError) as e:
            sc.Hit(np.zeros((1, 3)), np.ones((1, 3)), interval=(start, 10.0))
        assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT
