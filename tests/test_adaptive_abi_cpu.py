"""include/tray_adaptive.h on the CPU: the pixel-list renderer, the fold with per-pixel counts
and the selection step are declared, exported and bound, sit beside (not inside) the six older
headers, the header is C99 and links from C, argument errors are reported before any device
work, and the workspace size follows its formula. No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tray_adaptive.h")
CALLER = os.path.join(ROOT, "tests", "c", "tray_adaptive_caller.c")
OLDER = {"tray.h": "EXPORTS", "tray_query.h": "QUERY_EXPORTS", "tray_shade.h": "SHADE_EXPORTS",
         "tray_aov.h": "AOV_EXPORTS", "tray_denoise.h": "DENOISE_EXPORTS", "tray_progressive.h": "PROGRESSIVE_EXPORTS"}
FAKE = 0x100000  # a non-null "device pointer": validation fails before anything reads it
W, ROWS = 33, 17
PIXELS = W * ROWS
IMAGE = PIXELS * 24
INF, NAN = float("inf"), float("nan")


def _declared(path=HEADER):
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(path).read(), re.M))


def test_adaptive_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.ADAPTIVE_EXPORTS) and len(declared) == len(L.ADAPTIVE_EXPORTS) == 6
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_adaptive_version() == 1
    text = open(HEADER).read()
    assert "#define TRAY_ADAPTIVE_VERSION 1" in text
    assert '#include "tray.h"' in text and '#include "tray_progressive.h"' in text
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in L.ADAPTIVE_EXPORTS:
        assert re.search(rf"\bT {name}\b", out), name


def test_older_headers_and_lists_unchanged_by_adaptive(L):
    """The six older headers declare nothing of the new one; their export lists hold none of its
    symbols, keep their lengths and still match their headers; versions as before."""
    for header, listname in OLDER.items():
        text = open(os.path.join(INCLUDE, header)).read()
        for word in ("tray_adaptive", "TRAY_ADAPTIVE", "tray_render_pixels"):
            assert word not in text, (header, word)
        assert _declared(os.path.join(INCLUDE, header)) == set(getattr(L, listname)), header
        assert not set(L.ADAPTIVE_EXPORTS) & set(getattr(L, listname)), header
    assert (len(L.EXPORTS), len(L.QUERY_EXPORTS), len(L.SHADE_EXPORTS), len(L.AOV_EXPORTS),
            len(L.DENOISE_EXPORTS), len(L.PROGRESSIVE_EXPORTS)) == (27, 4, 4, 2, 4, 7)
    lib = L.lib()
    assert lib.tray_abi_version() == 6 and lib.tray_query_version() == 1 and lib.tray_shade_version() == 1
    assert lib.tray_aov_version() == 1 and lib.tray_denoise_version() == 1 and lib.tray_progressive_version() == 1


def _struct_fields(text, name):
    body = text[text.index(f"typedef struct {name} {{"):text.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body[body.index("{") + 1:].split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip(" *") for f in decl.split(None, 1)[1].split(",")]
    return fields


def test_struct_layouts(L):
    text = open(HEADER).read()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    for name, cls, size in (("tray_adaptive_state", L.AdaptiveState, 3 * ptr + 8),
                            ("tray_adaptive_params", L.AdaptiveParams, 32),
                            ("tray_adaptive_record", L.AdaptiveRecord, 32)):
        assert _struct_fields(text, name) == [n for n, _ in cls._fields_], name
        assert ctypes.sizeof(cls) == size, name
    assert L.AdaptiveState.count.offset == 2 * ptr and L.AdaptiveState.width.offset == 3 * ptr
    assert L.AdaptiveParams.min_passes.offset == 16 and L.AdaptiveParams.dilate.offset == 24
    assert [L.ADAPTIVE_RECORD_DTYPE.fields[n][1] for n in ("n_active", "unconverged", "max_ratio", "pixel_passes")] == \
        [0, 8, 16, 24] == [getattr(L.AdaptiveRecord, n).offset for n, _ in L.AdaptiveRecord._fields_]


def test_header_is_c99_and_links(tmp_path):
    """tests/c/tray_adaptive_caller.c includes the header and calls every entry point; it compiles as
    strict C99, links against the library, and its argument-error calls run without a device."""
    from tray_amd import _lib

    text = open(CALLER).read()
    for name in _lib.ADAPTIVE_EXPORTS:
        assert name + "(" in text, name
    exe = str(tmp_path / "tray_adaptive_caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, CALLER, "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)


def test_default_params(L):
    p = L.adaptive_params()
    mp = L.accum_metric_params()
    assert (p.tolerance, p.floor) == (mp.tolerance, mp.floor) == (0.05, 2.0 ** -10)
    assert (p.dilate, p.max_passes, p.reserved) == (1, 64, 0) and p.min_passes in (2, 4, 8)
    assert L.adaptive_params(min_passes=2).min_passes == 2
    assert L.lib().tray_adaptive_default_params(None) == L.TRAY_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        L.adaptive_params(passes=3)


# ------------------------------------------------------------- the sparse fold --
# mean, m2 at FAKE + 0 / 2 images; count at + 4; pixels at + 5; values from + 8 images on.
def _state(L, mean=FAKE, m2=FAKE + 2 * IMAGE, count=FAKE + 4 * IMAGE, width=W, rows=ROWS):
    return L.AdaptiveState(mean, m2, count, width, rows)


def _fold(L, pixels=FAKE + 5 * IMAGE, n_pixels=PIXELS, values=FAKE + 8 * IMAGE, n_passes=3, state="ok", **skw):
    st = _state(L, **skw)
    return L.lib().tray_adaptive_fold_async(ctypes.byref(st) if state == "ok" else None, pixels, n_pixels, values,
                                            n_passes, 0, None)


FOLD_ERRORS = {
    "null_state": (dict(state=None), "TRAY_ERR_INVALID_ARGUMENT", b"null state"),
    "null_mean": (dict(mean=None), "TRAY_ERR_INVALID_ARGUMENT", b"null mean or m2"),
    "null_m2": (dict(m2=None), "TRAY_ERR_INVALID_ARGUMENT", b"null mean or m2"),
    "null_count": (dict(count=None), "TRAY_ERR_INVALID_ARGUMENT", b"null count"),
    "null_pixels": (dict(pixels=None), "TRAY_ERR_INVALID_ARGUMENT", b"null pixels"),
    "null_values": (dict(values=None), "TRAY_ERR_INVALID_ARGUMENT", b"null values"),
    "negative_width": (dict(width=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative width or rows"),
    "negative_rows": (dict(rows=-5), "TRAY_ERR_INVALID_ARGUMENT", b"negative width or rows"),
    "negative_n_pixels": (dict(n_pixels=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative n_pixels"),
    "n_passes_0": (dict(n_passes=0), "TRAY_ERR_INVALID_ARGUMENT", b"1..65535"),
    "n_passes_65536": (dict(n_passes=65536), "TRAY_ERR_INVALID_ARGUMENT", b"1..65535"),
    "pixels_2_31": (dict(width=2 ** 16, rows=2 ** 15), "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels in one state"),
    "list_2_31": (dict(n_pixels=2 ** 31), "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels in one list"),
    "misaligned_mean": (dict(mean=FAKE + 4), "TRAY_ERR_INVALID_ARGUMENT", b"8-byte aligned"),
    "misaligned_values": (dict(values=FAKE + 8 * IMAGE + 4), "TRAY_ERR_INVALID_ARGUMENT", b"8-byte aligned"),
    "misaligned_count": (dict(count=FAKE + 4 * IMAGE + 2), "TRAY_ERR_INVALID_ARGUMENT", b"4-byte aligned"),
    "misaligned_pixels": (dict(pixels=FAKE + 5 * IMAGE + 1), "TRAY_ERR_INVALID_ARGUMENT", b"4-byte aligned"),
    "mean_is_m2": (dict(m2=FAKE), "TRAY_ERR_INVALID_ARGUMENT", b"mean overlaps m2"),
    "m2_overlaps_mean_end": (dict(m2=FAKE + IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"mean overlaps m2"),
    "count_in_m2": (dict(count=FAKE + 3 * IMAGE - 4), "TRAY_ERR_INVALID_ARGUMENT", b"m2 overlaps count"),
    "pixels_in_count": (dict(pixels=FAKE + 4 * IMAGE + 4 * PIXELS - 4), "TRAY_ERR_INVALID_ARGUMENT",
                        b"count overlaps pixels"),
    "mean_in_last_pass": (dict(mean=FAKE + 11 * IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"mean overlaps values"),
    "pixels_in_values": (dict(pixels=FAKE + 9 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"pixels overlaps values"),
}


@pytest.mark.parametrize("case", sorted(FOLD_ERRORS))
def test_fold_argument_errors_before_any_device_work(L, case):
    kw, status, word = FOLD_ERRORS[case]
    assert _fold(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_fold_of_nothing_is_ok_and_launches_nothing(L):
    for kw in (dict(width=0), dict(rows=0), dict(n_pixels=0), dict(n_pixels=0, pixels=None, values=None)):
        assert _fold(L, **kw) == L.TRAY_OK, kw


# ---------------------------------------------------------------- the selection --
# variance at + 12 images, the list at + 16, the record at + 17, the workspace at + 18.
def _select(L, variance=FAKE + 12 * IMAGE, pixels=FAKE + 16 * IMAGE, record=FAKE + 17 * IMAGE,
            workspace=FAKE + 18 * IMAGE, workspace_bytes=None, state="ok", params="ok", skw=None, **pkw):
    st = _state(L, **(skw or {}))
    p = L.adaptive_params()
    for name, value in pkw.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    need = ctypes.c_size_t(0)
    L.lib().tray_adaptive_workspace_bytes(max(st.width, 0), max(st.rows, 0), ctypes.byref(need))
    return L.lib().tray_adaptive_select_async(ctypes.byref(st) if state == "ok" else None,
                                              ctypes.byref(p) if params == "ok" else None, variance, pixels, record,
                                              workspace, need.value if workspace_bytes is None else workspace_bytes,
                                              0, None)


WORK = (PIXELS + 7) // 8 * 8 + 8  # 561 pixels: a 568-byte flag plane and one block total, padded to 8
SELECT_ERRORS = {
    "null_state": (dict(state=None), "TRAY_ERR_INVALID_ARGUMENT", b"null state"),
    "null_params": (dict(params=None), "TRAY_ERR_INVALID_ARGUMENT", b"null params"),
    "null_pixels": (dict(pixels=None), "TRAY_ERR_INVALID_ARGUMENT", b"null pixels"),
    "null_record": (dict(record=None), "TRAY_ERR_INVALID_ARGUMENT", b"null record"),
    "null_mean": (dict(skw=dict(mean=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null mean or m2"),
    "null_count": (dict(skw=dict(count=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null count"),
    "negative_width": (dict(skw=dict(width=-1)), "TRAY_ERR_INVALID_ARGUMENT", b"negative width or rows"),
    "pixels_2_31": (dict(skw=dict(width=2 ** 16, rows=2 ** 15)), "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels"),
    "tolerance_negative": (dict(tolerance=-1.0), "TRAY_ERR_INVALID_ARGUMENT", b"tolerance"),
    "tolerance_nan": (dict(tolerance=NAN), "TRAY_ERR_INVALID_ARGUMENT", b"tolerance"),
    "tolerance_inf": (dict(tolerance=INF), "TRAY_ERR_INVALID_ARGUMENT", b"tolerance"),
    "floor_zero": (dict(floor=0.0), "TRAY_ERR_INVALID_ARGUMENT", b"floor"),
    "floor_inf": (dict(floor=INF), "TRAY_ERR_INVALID_ARGUMENT", b"floor"),
    "min_passes_0": (dict(min_passes=0), "TRAY_ERR_INVALID_ARGUMENT", b"min_passes"),
    "max_below_min": (dict(min_passes=5, max_passes=4), "TRAY_ERR_INVALID_ARGUMENT", b"min_passes"),
    "max_passes_above_2_30": (dict(max_passes=2 ** 30 + 1), "TRAY_ERR_INVALID_ARGUMENT", b"2^30"),
    "dilate_2": (dict(dilate=2), "TRAY_ERR_INVALID_ARGUMENT", b"dilate"),
    "dilate_negative": (dict(dilate=-1), "TRAY_ERR_INVALID_ARGUMENT", b"dilate"),
    "reserved": (dict(reserved=1), "TRAY_ERR_INVALID_ARGUMENT", b"reserved"),
    "workspace_null": (dict(workspace=None), "TRAY_ERR_INVALID_ARGUMENT", b"workspace"),
    "workspace_one_byte_short": (dict(workspace_bytes=WORK - 1), "TRAY_ERR_INVALID_ARGUMENT", b"workspace"),
    "misaligned_variance": (dict(variance=FAKE + 12 * IMAGE + 4), "TRAY_ERR_INVALID_ARGUMENT", b"8-byte aligned"),
    "misaligned_record": (dict(record=FAKE + 17 * IMAGE + 4), "TRAY_ERR_INVALID_ARGUMENT", b"8-byte aligned"),
    "misaligned_workspace": (dict(workspace=FAKE + 18 * IMAGE + 4), "TRAY_ERR_INVALID_ARGUMENT", b"8-byte aligned"),
    "misaligned_pixels": (dict(pixels=FAKE + 16 * IMAGE + 2), "TRAY_ERR_INVALID_ARGUMENT", b"4-byte aligned"),
    "variance_is_mean": (dict(variance=FAKE), "TRAY_ERR_INVALID_ARGUMENT", b"mean overlaps variance"),
    "variance_in_m2": (dict(variance=FAKE + 3 * IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"m2 overlaps variance"),
    "pixels_in_count": (dict(pixels=FAKE + 4 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"count overlaps pixels"),
    "record_in_variance": (dict(record=FAKE + 13 * IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT",
                           b"variance overlaps the record"),
    "record_in_pixels": (dict(record=FAKE + 16 * IMAGE + 8), "TRAY_ERR_INVALID_ARGUMENT", b"pixels overlaps the record"),
    "workspace_in_mean": (dict(workspace=FAKE + IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"mean overlaps the workspace"),
    "workspace_end_in_record": (dict(record=FAKE + 18 * IMAGE + WORK - 8), "TRAY_ERR_INVALID_ARGUMENT",
                                b"the record overlaps the workspace"),
}


@pytest.mark.parametrize("case", sorted(SELECT_ERRORS))
def test_select_argument_errors_before_any_device_work(L, case):
    kw, status, word = SELECT_ERRORS[case]
    assert _select(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_select_empty_image_is_ok_and_launches_nothing(L):
    for skw in (dict(width=0), dict(rows=0), dict(width=0, rows=0)):
        assert _select(L, skw=skw) == L.TRAY_OK, skw
    assert _select(L, skw=dict(rows=0), workspace=None, workspace_bytes=0, variance=None) == L.TRAY_OK


def test_workspace_bytes_is_the_headers_formula(L):
    """A flag byte per pixel padded to 8 bytes, and a uint32 per block of 1024 pixels padded to 8."""
    for w, rows in ((1, 1), (1, 70), (33, 17), (129, 65), (1280, 720), (1024, 1), (1025, 1), (46340, 46340)):
        P = w * rows
        assert L.adaptive_workspace_bytes(w, rows) == (P + 7) // 8 * 8 + ((P + 1023) // 1024 + 1) // 2 * 8, (w, rows)
        assert L.adaptive_workspace_bytes(w, rows) <= L.adaptive_workspace_bytes(w + 1, rows)
    assert L.adaptive_workspace_bytes(0, 5) == 0 and L.adaptive_workspace_bytes(5, 0) == 0
    assert L.adaptive_workspace_bytes(33, 17) == WORK
    n = ctypes.c_size_t(0)
    lib = L.lib()
    assert lib.tray_adaptive_workspace_bytes(-1, 4, ctypes.byref(n)) == L.TRAY_ERR_INVALID_ARGUMENT
    assert lib.tray_adaptive_workspace_bytes(4, 4, None) == L.TRAY_ERR_INVALID_ARGUMENT
    assert lib.tray_adaptive_workspace_bytes(2 ** 16, 2 ** 15, ctypes.byref(n)) == L.TRAY_ERR_TOO_LARGE


# ----------------------------------------------------------- the pixel renderer --
def _pixels(L, scene=FAKE, camera="ok", params="ok", pixels=FAKE, n_pixels=10, plane=None, n_passes=1,
            out=FAKE + IMAGE, **pkw):
    kw = dict(width=W, height=ROWS, max_depth=5, rays_per_pixel=4, ray_radius=0.5, seed=1)
    kw.update(pkw)
    p = L.make_params(**kw)
    cam = L.CameraState()
    return L.lib().tray_render_pixels_async(scene, ctypes.byref(cam) if camera == "ok" else None,
                                            ctypes.byref(p) if params == "ok" else None, pixels, n_pixels, plane,
                                            n_passes, out, None, None)


PIXEL_ERRORS = {
    "null_scene": (dict(scene=None), "TRAY_ERR_INVALID_ARGUMENT", b"null scene"),
    "null_camera": (dict(camera=None), "TRAY_ERR_INVALID_ARGUMENT", b"null camera"),
    "null_params": (dict(params=None), "TRAY_ERR_INVALID_ARGUMENT", b"null params"),
    "bad_depth": (dict(max_depth=0), "TRAY_ERR_INVALID_ARGUMENT", b"max_depth"),
    "unknown_flag": (dict(flags=4), "TRAY_ERR_INVALID_ARGUMENT", b"unknown flags"),
    "output_f32": (dict(output=1), "TRAY_ERR_INVALID_ARGUMENT", b"TRAY_OUT_RGB_F64"),
    "output_rgba8": (dict(output=2), "TRAY_ERR_INVALID_ARGUMENT", b"TRAY_OUT_RGB_F64"),
    "negative_n_pixels": (dict(n_pixels=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative n_pixels"),
    "n_passes_0": (dict(n_passes=0), "TRAY_ERR_INVALID_ARGUMENT", b"n_passes"),
    "sample_word": (dict(pass_=2 ** 30 - 2, n_passes=3), "TRAY_ERR_TOO_LARGE", b"sample word"),
    "too_many_samples": (dict(n_pixels=2 ** 29, n_passes=1), "TRAY_ERR_TOO_LARGE", b"2^31 - 1"),
    "too_many_samples_by_passes": (dict(n_pixels=2 ** 20, n_passes=2 ** 9), "TRAY_ERR_TOO_LARGE", b"2^31 - 1"),
    "too_many_groups": (dict(n_pixels=2 ** 20, n_passes=2 ** 12, rays_per_pixel=1), "TRAY_ERR_TOO_LARGE", b"2^31 - 1"),
    "null_pixels": (dict(pixels=None), "TRAY_ERR_INVALID_ARGUMENT", b"null pixel list"),
    "null_out": (dict(out=None), "TRAY_ERR_INVALID_ARGUMENT", b"null result buffer"),
}


@pytest.mark.parametrize("case", sorted(PIXEL_ERRORS))
def test_render_pixels_argument_errors_before_any_device_work(L, case):
    kw, status, word = PIXEL_ERRORS[case]
    assert _pixels(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_render_pixels_of_nothing_is_ok_and_accepts_both_flags(L):
    """An empty list returns TRAY_OK before the (fake) scene is looked at, with either flag set."""
    for kw in (dict(), dict(pixels=None, out=None), dict(flags=L.FLAG_ORDERED_SUM),
               dict(flags=L.FLAG_LINEAR_SCAN | L.FLAG_ORDERED_SUM), dict(n_passes=7)):
        assert _pixels(L, n_pixels=0, **kw) == L.TRAY_OK, kw
    # n_pixels x n_passes x r = 2^31 - 1 exactly is within the limit: the next check (a null list) answers
    assert _pixels(L, n_pixels=2 ** 31 - 1, rays_per_pixel=1, pixels=None) == L.TRAY_ERR_INVALID_ARGUMENT
    assert b"null pixel list" in L.lib().tray_last_error()


def test_mirror_refuses_without_a_device(L):
    """Tracer.RenderPixels and RenderAdaptive refuse misshapen input with ValueError before any device
    work; the wrappers raise TrayError for argument errors."""
    import numpy as np

    from tray_amd import ray

    t = ray.New(8, 6)
    assert callable(t.RenderPixels) and callable(t.RenderAdaptive)
    with pytest.raises(ValueError):
        t.RenderPixels(None, np.zeros((2, 2), dtype=np.uint32))
    with pytest.raises(ValueError):
        t.RenderPixels(None, np.array([0.5, 1.0]))
    with pytest.raises(ValueError):
        t.RenderPixels(None, np.array([-1]))
    with pytest.raises(ValueError):
        t.RenderPixels(None, np.array([1, 2]), passes=0)
    with pytest.raises(ValueError):
        t.RenderAdaptive(None, 0)
    with pytest.raises(ValueError):
        t.RenderAdaptive(None, 4, batch=0)
    with pytest.raises(ValueError):
        t.RenderAdaptive(None, 4, min_passes=0)
    with pytest.raises(ValueError):
        t.RenderAdaptive(None, 4, sigma_variance=1.0)  # filter parameters without the filter
    with pytest.raises(L.TrayError) as e:
        L.adaptive_fold_async(L.AdaptiveState(FAKE, FAKE, FAKE + 4 * IMAGE, 8, 6), FAKE + 5 * IMAGE, 4,
                              FAKE + 8 * IMAGE, 1)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "overlaps" in str(e.value)
    with pytest.raises(L.TrayError) as e:
        L.adaptive_select_async(L.AdaptiveState(FAKE, FAKE + 2 * IMAGE, FAKE + 4 * IMAGE, 8, 6),
                                L.adaptive_params(dilate=3), FAKE + 16 * IMAGE, FAKE + 17 * IMAGE, FAKE + 18 * IMAGE,
                                1 << 20)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "dilate" in str(e.value)
