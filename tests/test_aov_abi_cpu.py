"""include/tray_aov.h on the CPU: the first-hit feature buffers are declared,
exported and bound, sit beside (not inside) tray.h, tray_query.h and
tray_shade.h, the header is C99 and links from C, and argument errors are
reported before any device work. No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tray_aov.h")
CALLER = os.path.join(ROOT, "tests", "c", "tray_aov_caller.c")
FAKE = 0x1000  # a non-null handle / "device pointer": validation fails before anything reads it


def _declared(path=HEADER):
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(path).read(), re.M))


def test_aov_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.AOV_EXPORTS) and len(declared) == 2
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_aov_version() == 1
    text = open(HEADER).read()
    assert "#define TRAY_AOV_VERSION 1" in text and '#include "tray.h"' in text


def test_older_headers_and_lists_unchanged_by_aov(L):
    """tray.h, tray_query.h and tray_shade.h declare nothing of the new header; the three older
    export lists hold none of its symbols and still match their own headers; versions as before."""
    for header in ("tray.h", "tray_query.h", "tray_shade.h"):
        text = open(os.path.join(INCLUDE, header)).read()
        assert "tray_aov" not in text and "tray_render_aov" not in text, header
    for name in L.AOV_EXPORTS:
        assert name not in L.EXPORTS and name not in L.QUERY_EXPORTS and name not in L.SHADE_EXPORTS
    assert _declared(os.path.join(INCLUDE, "tray_query.h")) == set(L.QUERY_EXPORTS)
    assert _declared(os.path.join(INCLUDE, "tray_shade.h")) == set(L.SHADE_EXPORTS)
    assert len(L.EXPORTS) == 27 and len(L.QUERY_EXPORTS) == 4 and len(L.SHADE_EXPORTS) == 4
    lib = L.lib()
    assert lib.tray_abi_version() == 6 and lib.tray_query_version() == 1 and lib.tray_shade_version() == 1


def test_buffers_struct_layout(L):
    assert ctypes.sizeof(L.AovBuffers) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in L.AovBuffers._fields_] == ["albedo", "normal", "depth", "coverage", "index"]
    assert [n for n, _, _ in L.AOV_BUFFERS] == [n for n, _ in L.AovBuffers._fields_]


def test_header_is_c99_and_links(tmp_path):
    """tests/c/tray_aov_caller.c includes the header and calls every entry point; it compiles as
    strict C99, links against the library, and its argument-error calls run without a device."""
    text = open(CALLER).read()
    for name in ("tray_aov_version", "tray_render_aov_async"):
        assert name + "(" in text, name
    exe = str(tmp_path / "tray_aov_caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, CALLER, "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)


def _params(L, **kw):
    base = dict(width=33, height=17, max_depth=10, rays_per_pixel=3, ray_radius=0.5, seed=21)
    base.update(kw)
    return L.make_params(**base)


def _call(L, scene=FAKE, camera="ok", params="ok", out="all", **pkw):
    cam = L.CameraState()
    p = _params(L, **pkw)
    bufs = {"all": L.AovBuffers(FAKE, FAKE, FAKE, FAKE, FAKE), "none": L.AovBuffers(), None: None,
            "index": L.AovBuffers(None, None, None, None, FAKE)}[out]
    return L.lib().tray_render_aov_async(scene, ctypes.byref(cam) if camera == "ok" else None,
                                         ctypes.byref(p) if params == "ok" else None,
                                         ctypes.byref(bufs) if bufs is not None else None, None)


# The params cases are the ones tests/test_abi_cpu.py and tray_render_async refuse.
ERRORS = {
    "null_scene": (dict(scene=None), "TRAY_ERR_INVALID_ARGUMENT", b"null scene"),
    "null_camera": (dict(camera=None), "TRAY_ERR_INVALID_ARGUMENT", b"null camera"),
    "null_params": (dict(params=None), "TRAY_ERR_INVALID_ARGUMENT", b"null params"),
    "null_out": (dict(out=None), "TRAY_ERR_INVALID_ARGUMENT", b"out"),
    "all_buffers_null": (dict(out="none"), "TRAY_ERR_INVALID_ARGUMENT", b"every feature buffer is null"),
    "zero_width": (dict(width=0), "TRAY_ERR_INVALID_ARGUMENT", b"width"),
    "zero_depth": (dict(max_depth=0), "TRAY_ERR_INVALID_ARGUMENT", b"max_depth"),
    "zero_rays": (dict(rays_per_pixel=0), "TRAY_ERR_INVALID_ARGUMENT", b"rays_per_pixel"),
    "nan_radius": (dict(ray_radius=float("nan")), "TRAY_ERR_INVALID_ARGUMENT", b"ray_radius"),
    "rows_outside": (dict(y_start=3, y_end=18), "TRAY_ERR_INVALID_ARGUMENT", b"row range"),
    "tile_index": (dict(tile_rows=2, tile_count=3, tile_index=3), "TRAY_ERR_INVALID_ARGUMENT", b"tile_index"),
    "unknown_output": (dict(output=3), "TRAY_ERR_INVALID_ARGUMENT", b"output"),
    "unknown_flag": (dict(flags=4), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
    "negative_pass": (dict(pass_=-1), "TRAY_ERR_INVALID_ARGUMENT", b"pass"),
    "sample_word": (dict(rays_per_pixel=2**16, pass_=2**16), "TRAY_ERR_TOO_LARGE", b"sample word"),
    "pixels_2_31": (dict(width=2**16, height=2**15), "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels"),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_argument_errors_before_any_device_work(L, case):
    kw, status, word = ERRORS[case]
    assert _call(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_empty_row_set_is_ok_and_launches_nothing(L):
    """Known flags pass validation: with an empty row set the call returns TRAY_OK before the
    (fake) scene handle or any buffer is looked at."""
    for flags in (0, L.FLAG_LINEAR_SCAN, L.FLAG_ORDERED_SUM, L.FLAG_LINEAR_SCAN | L.FLAG_ORDERED_SUM):
        assert _call(L, y_start=5, y_end=5, flags=flags) == L.TRAY_OK
        assert _call(L, y_start=5, y_end=5, flags=flags, out="index") == L.TRAY_OK


def test_mirror_needs_no_device_to_refuse(L):
    from tray_amd import ray

    t = ray.New(8, 4)
    assert callable(t.RenderAOV)
    dev = L.DeviceScene.__new__(L.DeviceScene)  # no upload: a null handle
    dev.L, dev.handle = L.lib(), ctypes.c_void_p()
    with pytest.raises(L.TrayError) as e:
        dev.render_aov_async(L.CameraState(), _params(L), FAKE, FAKE, FAKE, FAKE, FAKE)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "null scene" in str(e.value)
