"""include/tray_temporal_variance.h on the CPU: the M2-carrying reprojection step and the variance of
listed pixels are declared, exported and bound, sit beside (not inside) the eight older headers, the
header is C99 and links from C, and argument errors are reported before any device work. No kernel
is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tray_temporal_variance.h")
CALLER = os.path.join(ROOT, "tests", "c", "tray_temporal_variance_caller.c")
OLDER = {"tray.h": "EXPORTS", "tray_query.h": "QUERY_EXPORTS", "tray_shade.h": "SHADE_EXPORTS",
         "tray_aov.h": "AOV_EXPORTS", "tray_denoise.h": "DENOISE_EXPORTS", "tray_progressive.h": "PROGRESSIVE_EXPORTS",
         "tray_adaptive.h": "ADAPTIVE_EXPORTS", "tray_temporal.h": "TEMPORAL_EXPORTS"}
FAKE = 0x100000  # a non-null "device pointer": validation fails before anything reads it
W, H = 33, 17
PIXELS = W * H
IMAGE = PIXELS * 24
INF, NAN = float("inf"), float("nan")


def _declared(path=HEADER):
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(path).read(), re.M))


def test_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.TEMPORAL_VARIANCE_EXPORTS) and len(declared) == len(L.TEMPORAL_VARIANCE_EXPORTS) == 3
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_temporal_var_version() == 1
    text = open(HEADER).read()
    assert "#define TRAY_TEMPORAL_VAR_VERSION 1" in text and '#include "tray_temporal.h"' in text
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in L.TEMPORAL_VARIANCE_EXPORTS:
        assert re.search(rf"\bT {name}\b", out), name


def test_older_headers_and_lists_unchanged(L):
    """The eight older headers declare nothing of the new one; their export lists hold none of its
    symbols, keep their lengths and still match their headers; versions as before."""
    for header, listname in OLDER.items():
        text = open(os.path.join(INCLUDE, header)).read()
        for word in ("tray_temporal_var", "TRAY_TEMPORAL_VAR"):
            assert word not in text, (header, word)
        assert _declared(os.path.join(INCLUDE, header)) == set(getattr(L, listname)), header
        assert not set(L.TEMPORAL_VARIANCE_EXPORTS) & set(getattr(L, listname)), header
    assert (len(L.EXPORTS), len(L.QUERY_EXPORTS), len(L.SHADE_EXPORTS), len(L.AOV_EXPORTS), len(L.DENOISE_EXPORTS),
            len(L.PROGRESSIVE_EXPORTS), len(L.ADAPTIVE_EXPORTS), len(L.TEMPORAL_EXPORTS)) == (27, 4, 4, 2, 4, 7, 6, 3)
    assert L.TEMPORAL_EXPORTS == ("tray_temporal_version", "tray_temporal_default_params", "tray_temporal_step_async")
    lib = L.lib()
    assert lib.tray_abi_version() == 6 and lib.tray_query_version() == 1 and lib.tray_shade_version() == 1
    assert lib.tray_aov_version() == 1 and lib.tray_denoise_version() == 1 and lib.tray_progressive_version() == 1
    assert lib.tray_adaptive_version() == 1 and lib.tray_temporal_version() == 1
    assert "#define TRAY_TEMPORAL_VERSION 1" in open(os.path.join(INCLUDE, "tray_temporal.h")).read()


def _struct_fields(text, name):
    body = text[text.index(f"typedef struct {name} {{"):text.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body[body.index("{") + 1:].split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip(" *") for f in decl.split(None, 1)[1].split(",")]
    return fields


def test_struct_layout(L):
    text = open(HEADER).read()
    ptr = ctypes.sizeof(ctypes.c_void_p)
    S = L.TemporalVarState
    assert _struct_fields(text, "tray_temporal_var_state") == [n for n, _ in S._fields_]
    assert ctypes.sizeof(S) == 5 * ptr + 8
    assert (S.colour.offset, S.m2.offset, S.age.offset, S.index.offset, S.depth.offset, S.width.offset,
            S.height.offset) == (0, ptr, 2 * ptr, 3 * ptr, 4 * ptr, 5 * ptr, 5 * ptr + 4)
    # the parameters and the record are tray_temporal.h's: the header defines no others
    assert set(re.findall(r"typedef struct (\w+)", text)) == {"tray_temporal_var_state"}
    # every temporal state with m2 is a tray_adaptive_state {mean = colour, m2, count = age, width, rows = height}
    s = S(1, 2, 3, 4, 5, 6, 7)
    a = s.adaptive()
    assert isinstance(a, L.AdaptiveState) and (a.mean, a.m2, a.count, a.width, a.rows) == (1, 2, 3, 6, 7)


def test_header_is_c99_and_links(tmp_path):
    """tests/c/tray_temporal_variance_caller.c includes the header and calls every entry point; it
    compiles as strict C99, links against the library, and its argument-error calls run without a
    device."""
    from tray_amd import _lib

    text = open(CALLER).read()
    for name in _lib.TEMPORAL_VARIANCE_EXPORTS:
        assert name + "(" in text, name
    exe = str(tmp_path / "tray_temporal_variance_caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, CALLER, "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)


# The frame at FAKE; out's colour, m2, depth, age, index at OUT + 0, 1, 2, 3, 4 images; the history's at
# HIST + the same; the variance at + 14 images, the record at + 16.
OUT, HIST, VARIANCE, RECORD = FAKE + 2 * IMAGE, FAKE + 8 * IMAGE, FAKE + 14 * IMAGE, FAKE + 16 * IMAGE


def _state(L, base, width=W, height=H, **absolute):
    at = dict(colour=base, m2=base + IMAGE, depth=base + 2 * IMAGE, age=base + 3 * IMAGE, index=base + 4 * IMAGE)
    assert set(absolute) <= set(at), absolute
    at.update(absolute)
    return L.TemporalVarState(at["colour"], at["m2"], at["age"], at["index"], at["depth"], width, height)


def _step(L, scene=FAKE, camera="ok", prev="ok", params="ok", frame=FAKE, history="ok", out="ok", variance=VARIANCE,
          record=RECORD, okw=None, hkw=None, **pkw):
    tp = L.temporal_params()
    for name, value in pkw.items():
        assert hasattr(tp, name), name
        setattr(tp, name, value)
    cam, pcam = L.CameraState(), L.CameraState()
    o = _state(L, OUT, **(okw or {}))
    hs = _state(L, HIST, **(hkw or {}))
    return L.lib().tray_temporal_var_step_async(
        scene, ctypes.byref(cam) if camera == "ok" else None, ctypes.byref(pcam) if prev == "ok" else None,
        ctypes.byref(tp) if params == "ok" else None, frame, ctypes.byref(hs) if history == "ok" else None,
        ctypes.byref(o) if out == "ok" else None, variance, record, None)


STEP_ERRORS = {
    "null_scene": (dict(scene=None), "TRAY_ERR_INVALID_ARGUMENT", b"null scene"),
    "null_camera": (dict(camera=None), "TRAY_ERR_INVALID_ARGUMENT", b"null camera"),
    "null_params": (dict(params=None), "TRAY_ERR_INVALID_ARGUMENT", b"null params"),
    "null_out": (dict(out=None), "TRAY_ERR_INVALID_ARGUMENT", b"null state"),
    "history_without_camera": (dict(prev=None), "TRAY_ERR_INVALID_ARGUMENT", b"both"),
    "camera_without_history": (dict(history=None), "TRAY_ERR_INVALID_ARGUMENT", b"both"),
    "negative_width": (dict(okw=dict(width=-1), hkw=dict(width=-1)), "TRAY_ERR_INVALID_ARGUMENT", b"negative width"),
    "negative_height": (dict(okw=dict(height=-1), hkw=dict(height=-1)), "TRAY_ERR_INVALID_ARGUMENT",
                        b"negative width or height"),
    "history_another_size": (dict(hkw=dict(width=W + 1)), "TRAY_ERR_INVALID_ARGUMENT", b"differ"),
    "pixels_2_31": (dict(okw=dict(width=2 ** 16, height=2 ** 15), hkw=dict(width=2 ** 16, height=2 ** 15)),
                    "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels"),
    "max_history_0": (dict(max_history=0), "TRAY_ERR_INVALID_ARGUMENT", b"max_history"),
    "max_history_above_2_30": (dict(max_history=2 ** 30 + 1), "TRAY_ERR_INVALID_ARGUMENT", b"2^30"),
    "unknown_flag": (dict(flags=2), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
    "tolerance_negative": (dict(depth_tolerance=-0.5), "TRAY_ERR_INVALID_ARGUMENT", b"depth_tolerance"),
    "tolerance_nan": (dict(depth_tolerance=NAN), "TRAY_ERR_INVALID_ARGUMENT", b"depth_tolerance"),
    "tolerance_inf": (dict(depth_tolerance=INF), "TRAY_ERR_INVALID_ARGUMENT", b"depth_tolerance"),
    "snap_half": (dict(snap=0.5), "TRAY_ERR_INVALID_ARGUMENT", b"snap"),
    "snap_negative": (dict(snap=-1e-9), "TRAY_ERR_INVALID_ARGUMENT", b"snap"),
    "snap_nan": (dict(snap=NAN), "TRAY_ERR_INVALID_ARGUMENT", b"snap"),
    "reserved": (dict(reserved=1), "TRAY_ERR_INVALID_ARGUMENT", b"reserved"),
    "null_frame": (dict(frame=None), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: the frame"),
    "null_out_m2": (dict(okw=dict(m2=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: out.m2"),
    "null_out_age": (dict(okw=dict(age=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: out.age"),
    "null_history_m2": (dict(hkw=dict(m2=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: history.m2"),
    "null_history_depth": (dict(hkw=dict(depth=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: history.depth"),
    "misaligned_frame": (dict(frame=FAKE + 4), "TRAY_ERR_INVALID_ARGUMENT", b"the frame is not 8-byte aligned"),
    "misaligned_out_m2": (dict(okw=dict(m2=OUT + IMAGE + 4)), "TRAY_ERR_INVALID_ARGUMENT",
                          b"out.m2 is not 8-byte aligned"),
    "misaligned_out_index": (dict(okw=dict(index=OUT + 4 * IMAGE + 2)), "TRAY_ERR_INVALID_ARGUMENT",
                             b"out.index is not 4-byte aligned"),
    "misaligned_history_m2": (dict(hkw=dict(m2=HIST + IMAGE + 4)), "TRAY_ERR_INVALID_ARGUMENT",
                              b"history.m2 is not 8-byte aligned"),
    "misaligned_history_age": (dict(hkw=dict(age=HIST + 3 * IMAGE + 1)), "TRAY_ERR_INVALID_ARGUMENT",
                               b"history.age is not 4-byte aligned"),
    "misaligned_variance": (dict(variance=VARIANCE + 4), "TRAY_ERR_INVALID_ARGUMENT",
                            b"the variance is not 8-byte aligned"),
    "misaligned_record": (dict(record=RECORD + 4), "TRAY_ERR_INVALID_ARGUMENT", b"the record is not 8-byte aligned"),
    "out_is_the_frame": (dict(frame=OUT), "TRAY_ERR_INVALID_ARGUMENT", b"out.colour overlaps the frame"),
    "out_m2_is_the_frame": (dict(frame=OUT + IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"out.m2 overlaps the frame"),
    "out_is_history": (dict(hkw=dict(colour=OUT)), "TRAY_ERR_INVALID_ARGUMENT", b"out.colour overlaps history.colour"),
    "out_m2_is_history_m2": (dict(hkw=dict(m2=OUT + IMAGE)), "TRAY_ERR_INVALID_ARGUMENT",
                             b"out.m2 overlaps history.m2"),
    "out_m2_end_in_history_colour": (dict(hkw=dict(colour=OUT + 2 * IMAGE - 8)), "TRAY_ERR_INVALID_ARGUMENT",
                                     b"out.m2 overlaps"),
    "out_colour_is_out_m2": (dict(okw=dict(m2=OUT + IMAGE - 8)), "TRAY_ERR_INVALID_ARGUMENT",
                             b"out.colour overlaps out.m2"),
    "out_age_in_out_depth": (dict(okw=dict(age=OUT + 2 * IMAGE + 8 * PIXELS - 4)), "TRAY_ERR_INVALID_ARGUMENT",
                             b"out.age overlaps out.depth"),
    "variance_is_out_m2": (dict(variance=OUT + IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"out.m2 overlaps the variance"),
    "variance_is_the_frame": (dict(variance=FAKE + 8), "TRAY_ERR_INVALID_ARGUMENT",
                              b"the variance overlaps the frame"),
    "variance_in_history_m2": (dict(variance=HIST + 2 * IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT",
                               b"the variance overlaps history.m2"),
    "record_in_variance": (dict(record=VARIANCE + IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT",
                           b"the variance overlaps the record"),
    "record_in_history_depth": (dict(record=HIST + 2 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT",
                                b"the record overlaps history.depth"),
}


@pytest.mark.parametrize("case", sorted(STEP_ERRORS))
def test_step_argument_errors_before_any_device_work(L, case):
    kw, status, word = STEP_ERRORS[case]
    assert _step(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def _variance(L, state="ok", pixels=FAKE, n=5, variance=VARIANCE, skw=None):
    s = _state(L, OUT, **(skw or {}))
    return L.lib().tray_temporal_var_variance_async(ctypes.byref(s) if state == "ok" else None, pixels, n, variance,
                                                    0, None)


VARIANCE_ERRORS = {
    "null_state": (dict(state=None), "TRAY_ERR_INVALID_ARGUMENT", b"null state"),
    "negative_width": (dict(skw=dict(width=-1)), "TRAY_ERR_INVALID_ARGUMENT", b"negative width"),
    "negative_n_pixels": (dict(n=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative n_pixels"),
    "pixels_2_31": (dict(skw=dict(width=2 ** 16, height=2 ** 15)), "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels"),
    "n_pixels_2_31": (dict(n=2 ** 31), "TRAY_ERR_TOO_LARGE", b"n_pixels"),
    "null_m2": (dict(skw=dict(m2=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: m2"),
    "null_age": (dict(skw=dict(age=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: age"),
    "null_variance": (dict(variance=None), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: the variance"),
    "null_variance_whole_frame": (dict(variance=None, pixels=None), "TRAY_ERR_INVALID_ARGUMENT",
                                  b"null buffer: the variance"),
    "misaligned_m2": (dict(skw=dict(m2=OUT + IMAGE + 4)), "TRAY_ERR_INVALID_ARGUMENT", b"m2 is not 8-byte aligned"),
    "misaligned_age": (dict(skw=dict(age=OUT + 3 * IMAGE + 2)), "TRAY_ERR_INVALID_ARGUMENT",
                       b"age is not 4-byte aligned"),
    "misaligned_variance": (dict(variance=VARIANCE + 4), "TRAY_ERR_INVALID_ARGUMENT",
                            b"the variance is not 8-byte aligned"),
    "misaligned_list": (dict(pixels=FAKE + 2), "TRAY_ERR_INVALID_ARGUMENT", b"the pixel list is not 4-byte aligned"),
    "variance_is_m2": (dict(variance=OUT + IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"the variance overlaps m2"),
    "variance_end_in_age": (dict(variance=OUT + 2 * IMAGE + 8), "TRAY_ERR_INVALID_ARGUMENT",
                            b"the variance overlaps age"),
    "list_in_variance": (dict(pixels=VARIANCE + IMAGE - 4), "TRAY_ERR_INVALID_ARGUMENT",
                         b"the variance overlaps the pixel list"),
}


@pytest.mark.parametrize("case", sorted(VARIANCE_ERRORS))
def test_variance_argument_errors_before_any_device_work(L, case):
    kw, status, word = VARIANCE_ERRORS[case]
    assert _variance(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_empty_image_and_empty_list_are_ok_and_launch_nothing(L):
    """TRAY_OK before the (fake) scene, the device or any plane is looked at."""
    for dims in (dict(width=0), dict(height=0), dict(width=0, height=0)):
        assert _step(L, okw=dims, hkw=dims) == L.TRAY_OK, dims
        assert _step(L, okw=dims, history=None, prev=None, frame=None, record=None, variance=None) == L.TRAY_OK, dims
        assert _variance(L, skw=dims) == L.TRAY_OK, dims
        assert _variance(L, skw=dims, pixels=None, n=0, variance=None) == L.TRAY_OK, dims
    none = dict(colour=None, m2=None, age=None, index=None, depth=None, height=0)
    assert _step(L, okw=none, hkw=none, frame=None, record=None, variance=None) == L.TRAY_OK
    assert _variance(L, n=0) == L.TRAY_OK
    assert _variance(L, n=0, variance=None, skw=dict(m2=None, age=None)) == L.TRAY_OK


def test_render_sequence_refusals_without_a_device(L):
    """ValueError before any device work for what RenderSequence's new arguments refuse; the old
    refusals hold with them; the wrappers raise TrayError for argument errors."""
    from tray_amd import ray

    t = ray.New(8, 6)
    cams = [ray.RichSceneCamera()]
    for kw in (dict(refill=-1), dict(refill=1.5), dict(refill=True), dict(refill="3"), dict(refill=1, max_history=1),
               dict(refill=3, max_history=3), dict(refill=1, refill_tolerance=-1.0),
               dict(refill=1, refill_tolerance=NAN), dict(refill=1, refill_tolerance=INF),
               dict(refill=1, refill_tolerance=1e200), dict(refill=1, refill_dilate=2),
               dict(variance=True, history=4), dict(variance=True, reserved=0), dict(refill=2, sigma_variance=1.0)):
        with pytest.raises(ValueError):
            t.RenderSequence(None, cams, **kw)
    for bad in ([], None, [cams[0], "camera"]):
        with pytest.raises(ValueError):
            t.RenderSequence(None, bad, variance=True, refill=2)
    with pytest.raises(L.TrayError) as e:
        L.temporal_var_step_async(FAKE, L.CameraState(), None, L.temporal_params(snap=0.75), FAKE, None,
                                  _state(L, OUT), VARIANCE)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "snap" in str(e.value)
    with pytest.raises(L.TrayError) as e:
        L.temporal_var_variance_async(_state(L, OUT), FAKE, 4, OUT + IMAGE)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "overlaps m2" in str(e.value)
    assert isinstance(ray.REFILL_DEFAULT, int) and 0 < ray.REFILL_DEFAULT < L.temporal_params().max_history
