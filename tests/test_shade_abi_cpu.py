"""include/tray_shade.h on the CPU: Material.Scatter, AmbientLight.Hit and the
occlusion query are declared, exported and bound, sit beside (not inside) tray.h
and tray_query.h, the header is C99, and argument errors are reported before any
device work. No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tray_shade.h")
FAKE = 0x1000  # a non-null "device pointer" / handle: validation fails (or n == 0 returns) before anything reads it
INF = float("inf")


def _declared():
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(HEADER).read(), re.M))


def test_shade_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.SHADE_EXPORTS) and len(declared) == 4
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_shade_version() == 1
    text = open(HEADER).read()
    assert "#define TRAY_SHADE_VERSION 1" in text and '#include "tray_query.h"' in text


def test_stable_headers_unchanged_by_shade(L):
    """tray.h and tray_query.h declare none of the new entry points; EXPORTS and QUERY_EXPORTS list none."""
    stable = open(os.path.join(ROOT, "include", "tray.h")).read()
    query = open(os.path.join(ROOT, "include", "tray_query.h")).read()
    for name in L.SHADE_EXPORTS:
        assert name not in stable and name not in query
        assert name not in L.EXPORTS and name not in L.QUERY_EXPORTS
    assert "tray_scatter" not in stable and "tray_scatter" not in query
    assert L.lib().tray_abi_version() == 6 and L.lib().tray_query_version() == 1


def test_scatter_struct_layout(L):
    assert ctypes.sizeof(L.Scatter) == 80 and L.SCATTER_DTYPE.itemsize == 80
    assert L.Scatter.attenuation.offset == 0 and L.Scatter.ray.offset == 24
    assert L.Scatter.scattered.offset == 72 and L.Scatter.reserved.offset == 76
    f = L.SCATTER_DTYPE.fields
    assert f["attenuation"][1] == 0 and f["ray"][1] == 24 and f["scattered"][1] == 72 and f["reserved"][1] == 76
    assert f["ray"][0] == L.RAY_DTYPE


def test_header_is_c99():
    """tests/c/tray_shade_caller.c includes the header and calls every entry point
    (its typedefs also pin the struct's size and offsets at compile time)."""
    src = os.path.join(ROOT, "tests", "c", "tray_shade_caller.c")
    text = open(src).read()
    for name in ("tray_shade_version", "tray_scatter_async", "tray_background_hit_async", "tray_scene_occluded_async"):
        assert name + "(" in text, name
    assert "sizeof(tray_scatter) == 80" in text
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _scatter(L, scene=None, rays=FAKE, hits=FAKE, ids=None, n=4, bounce=0, seed=1, out=FAKE):
    return L.lib().tray_scatter_async(scene, rays, hits, ids, n, bounce, seed, out, None)


def _sky(L, bg="default", rays=FAKE, n=4, rgb=FAKE, device=0):
    b = L.Background((ctypes.c_double * 3)(1, 1, 1), (ctypes.c_double * 3)(0.4, 0.65, 1.0))
    return L.lib().tray_background_hit_async(ctypes.byref(b) if bg == "default" else bg, rays, n, rgb, device, None)


def _occluded(L, scene=None, rays=FAKE, ends=None, n=4, t_end=INF, flags=0, out=FAKE):
    return L.lib().tray_scene_occluded_async(scene, rays, ends, n, t_end, flags, out, None)


SCATTER_ERRORS = {
    "null_scene": (dict(), "TRAY_ERR_INVALID_ARGUMENT", b"null scene"),
    "null_rays": (dict(rays=None), "TRAY_ERR_INVALID_ARGUMENT", b"null ray buffer"),
    "null_hits": (dict(scene=FAKE, hits=None), "TRAY_ERR_INVALID_ARGUMENT", b"null hit buffer"),
    "null_out": (dict(out=None), "TRAY_ERR_INVALID_ARGUMENT", b"null result buffer"),
    "negative_n": (dict(n=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative"),
    "n_2_31": (dict(n=2**31), "TRAY_ERR_TOO_LARGE", b"2^31"),
}

SKY_ERRORS = {
    "null_background": (dict(bg=None), "TRAY_ERR_INVALID_ARGUMENT", b"null background"),
    "null_rays": (dict(rays=None), "TRAY_ERR_INVALID_ARGUMENT", b"null ray buffer"),
    "null_rgb": (dict(rgb=None), "TRAY_ERR_INVALID_ARGUMENT", b"null result buffer"),
    "negative_n": (dict(n=-3), "TRAY_ERR_INVALID_ARGUMENT", b"negative"),
    "n_2_31": (dict(n=2**31), "TRAY_ERR_TOO_LARGE", b"2^31"),
}

OCCLUDED_ERRORS = {
    "null_scene": (dict(), "TRAY_ERR_INVALID_ARGUMENT", b"null scene"),
    "null_rays": (dict(rays=None), "TRAY_ERR_INVALID_ARGUMENT", b"null ray buffer"),
    "null_out": (dict(out=None), "TRAY_ERR_INVALID_ARGUMENT", b"null result buffer"),
    "negative_n": (dict(n=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative"),
    "n_2_31": (dict(n=2**31), "TRAY_ERR_TOO_LARGE", b"2^31"),
    "unknown_flag": (dict(flags=4), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
    "ordered_sum_flag": (dict(flags=2), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
    "nan_t_end": (dict(t_end=float("nan")), "TRAY_ERR_INVALID_ARGUMENT", b"NaN"),
    "nan_t_end_beside_per_ray_ends": (dict(t_end=float("nan"), ends=FAKE), "TRAY_ERR_INVALID_ARGUMENT", b"NaN"),
}


def _expect(L, rc, status, word):
    assert rc == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


@pytest.mark.parametrize("case", sorted(SCATTER_ERRORS))
def test_scatter_argument_errors(L, case):
    kw, status, word = SCATTER_ERRORS[case]
    _expect(L, _scatter(L, **kw), status, word)


@pytest.mark.parametrize("case", sorted(SKY_ERRORS))
def test_background_hit_argument_errors(L, case):
    kw, status, word = SKY_ERRORS[case]
    _expect(L, _sky(L, **kw), status, word)


@pytest.mark.parametrize("case", sorted(OCCLUDED_ERRORS))
def test_occluded_argument_errors(L, case):
    kw, status, word = OCCLUDED_ERRORS[case]
    _expect(L, _occluded(L, **kw), status, word)


def test_n_zero_with_null_buffers_is_ok(L):
    """n == 0 returns before the scene handle or any buffer is looked at."""
    assert _scatter(L, scene=FAKE, rays=None, hits=None, out=None, n=0) == L.TRAY_OK
    assert _sky(L, rays=None, rgb=None, n=0) == L.TRAY_OK
    assert _occluded(L, scene=FAKE, rays=None, out=None, n=0) == L.TRAY_OK
    assert _occluded(L, scene=FAKE, rays=None, out=None, n=0, flags=L.FLAG_LINEAR_SCAN) == L.TRAY_OK


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_background_hit_without_device_fails_loudly(L):
    _expect(L, _sky(L), "TRAY_ERR_NO_DEVICE", b"")


def test_mirror_rejects_length_mismatches_before_any_device_work(L):
    from tray_amd import ray

    sc = ray.DefaultScene()
    o, d = np.zeros((3, 3)), np.ones((3, 3))
    with pytest.raises(ValueError):
        sc.Scatter(o, d, np.zeros(2, dtype=L.HIT_DTYPE), seed=1)
    with pytest.raises(ValueError):
        sc.Scatter(o, d, np.zeros(3, dtype=L.HIT_DTYPE), seed=1, ids=np.zeros((2, 2), dtype=np.uint32))
    with pytest.raises(TypeError):
        sc.Scatter(o, d, np.zeros((3, 8)), seed=1)
    with pytest.raises(ValueError):
        sc.Occluded(o, d, t_end=np.ones(4))
    assert sc._uploaded == {}
