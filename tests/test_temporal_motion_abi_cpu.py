"""include/tray_temporal_motion.h on the CPU: the reprojection step across scene updates is declared,
exported and bound, sits beside (not inside) the older headers, the header is C99 and links from C,
and argument errors are reported before any device work (the one check that needs a real scene, an
n_spheres other than the scene's, is in tests/test_gpu_temporal_motion.py). No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tray_temporal_motion.h")
CALLER = os.path.join(ROOT, "tests", "c", "tray_temporal_motion_caller.c")
OLDER = {"tray.h": "EXPORTS", "tray_query.h": "QUERY_EXPORTS", "tray_shade.h": "SHADE_EXPORTS",
         "tray_aov.h": "AOV_EXPORTS", "tray_denoise.h": "DENOISE_EXPORTS", "tray_progressive.h": "PROGRESSIVE_EXPORTS",
         "tray_adaptive.h": "ADAPTIVE_EXPORTS", "tray_temporal.h": "TEMPORAL_EXPORTS",
         "tray_temporal_variance.h": "TEMPORAL_VARIANCE_EXPORTS", "tray_scene_update.h": "SCENE_UPDATE_EXPORTS"}
FAKE = 0x100000  # a non-null "device pointer": validation fails before anything reads it
W, H = 33, 17
PIXELS = W * H
IMAGE = PIXELS * 24
N = 5
INF, NAN = float("inf"), float("nan")


def _declared(path=HEADER):
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(path).read(), re.M))


def test_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.TEMPORAL_MOTION_EXPORTS) and len(declared) == len(L.TEMPORAL_MOTION_EXPORTS) == 2
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_temporal_motion_version() == 1
    text = open(HEADER).read()
    assert "#define TRAY_TEMPORAL_MOTION_VERSION 1" in text and '#include "tray_temporal_variance.h"' in text
    assert not re.findall(r"typedef struct (\w+)", text)  # params, record and states are the older headers'
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in L.TEMPORAL_MOTION_EXPORTS:
        assert re.search(rf"\bT {name}\b", out), name


def test_older_headers_and_lists_unchanged(L):
    """The older headers declare nothing of the new one; their export lists hold none of its symbols,
    keep their lengths and still match their headers; versions as before. tray_scene_update.h may
    name the new header in its text (it points to it), not declare anything of it."""
    for header, listname in OLDER.items():
        text = open(os.path.join(INCLUDE, header)).read()
        assert "tray_temporal_motion_" not in text and "TRAY_TEMPORAL_MOTION" not in text, header
        assert _declared(os.path.join(INCLUDE, header)) == set(getattr(L, listname)), header
        assert not set(L.TEMPORAL_MOTION_EXPORTS) & set(getattr(L, listname)), header
    assert (len(L.EXPORTS), len(L.QUERY_EXPORTS), len(L.SHADE_EXPORTS), len(L.AOV_EXPORTS), len(L.DENOISE_EXPORTS),
            len(L.PROGRESSIVE_EXPORTS), len(L.ADAPTIVE_EXPORTS), len(L.TEMPORAL_EXPORTS),
            len(L.TEMPORAL_VARIANCE_EXPORTS), len(L.SCENE_UPDATE_EXPORTS)) == (27, 4, 4, 2, 4, 7, 6, 3, 3, 2)
    lib = L.lib()
    assert lib.tray_abi_version() == 6 and lib.tray_temporal_version() == 1 and lib.tray_temporal_var_version() == 1


def test_header_is_c99_and_links(tmp_path):
    """tests/c/tray_temporal_motion_caller.c includes the header and calls every entry point; it compiles
    as strict C99, links against the library, and its argument-error calls run without a device."""
    from tray_amd import _lib

    text = open(CALLER).read()
    for name in _lib.TEMPORAL_MOTION_EXPORTS:
        assert name + "(" in text, name
    exe = str(tmp_path / "tray_temporal_motion_caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, CALLER, "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)


# The frame at FAKE; out's colour, m2, depth, age, index at OUT + 0, 1, 2, 3, 4 images; the history's at
# HIST + the same; the variance at + 14 images, the record at + 16, the motion plane at + 17, the
# previous geometry at + 18.
OUT, HIST, VARIANCE, RECORD = FAKE + 2 * IMAGE, FAKE + 8 * IMAGE, FAKE + 14 * IMAGE, FAKE + 16 * IMAGE
MOTION, GEOMETRY = FAKE + 17 * IMAGE, FAKE + 18 * IMAGE


def _state(L, base, with_m2=True, width=W, height=H, **absolute):
    at = dict(colour=base, m2=base + IMAGE if with_m2 else None, depth=base + 2 * IMAGE, age=base + 3 * IMAGE,
              index=base + 4 * IMAGE)
    assert set(absolute) <= set(at), absolute
    at.update(absolute)
    return L.TemporalVarState(at["colour"], at["m2"], at["age"], at["index"], at["depth"], width, height)


def _step(L, scene=FAKE, camera="ok", prev="ok", geometry=GEOMETRY, n=N, params="ok", frame=FAKE, history="ok",
          out="ok", variance=VARIANCE, motion=MOTION, record=RECORD, m2=True, okw=None, hkw=None, **pkw):
    tp = L.temporal_params()
    for name, value in pkw.items():
        assert hasattr(tp, name), name
        setattr(tp, name, value)
    cam, pcam = L.CameraState(), L.CameraState()
    o = _state(L, OUT, m2, **(okw or {}))
    hs = _state(L, HIST, m2, **(hkw or {}))
    return L.lib().tray_temporal_motion_step_async(
        scene, ctypes.byref(cam) if camera == "ok" else None, ctypes.byref(pcam) if prev == "ok" else None,
        geometry, n, ctypes.byref(tp) if params == "ok" else None, frame, ctypes.byref(hs) if history == "ok" else None,
        ctypes.byref(o) if out == "ok" else None, variance if m2 or variance != VARIANCE else None, motion, record,
        None)


INVALID = "TRAY_ERR_INVALID_ARGUMENT"
# Every error of tray_temporal_step_async and tray_temporal_var_step_async, through the same checker:
SHARED_ERRORS = {
    "null_scene": (dict(scene=None), INVALID, b"null scene"),
    "null_camera": (dict(camera=None), INVALID, b"null camera"),
    "null_params": (dict(params=None), INVALID, b"null params"),
    "null_out": (dict(out=None), INVALID, b"null state"),
    "history_without_camera": (dict(prev=None), INVALID, b"both"),
    "camera_without_history": (dict(history=None), INVALID, b"both"),
    "negative_width": (dict(okw=dict(width=-1), hkw=dict(width=-1)), INVALID, b"negative width"),
    "negative_height": (dict(okw=dict(height=-1), hkw=dict(height=-1)), INVALID, b"negative width or height"),
    "history_another_size": (dict(hkw=dict(width=W + 1)), INVALID, b"differ"),
    "pixels_2_31": (dict(okw=dict(width=2 ** 16, height=2 ** 15), hkw=dict(width=2 ** 16, height=2 ** 15)),
                    "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels"),
    "max_history_0": (dict(max_history=0), INVALID, b"max_history"),
    "max_history_above_2_30": (dict(max_history=2 ** 30 + 1), INVALID, b"2^30"),
    "unknown_flag": (dict(flags=2), INVALID, b"flags"),
    "tolerance_negative": (dict(depth_tolerance=-0.5), INVALID, b"depth_tolerance"),
    "tolerance_nan": (dict(depth_tolerance=NAN), INVALID, b"depth_tolerance"),
    "tolerance_inf": (dict(depth_tolerance=INF), INVALID, b"depth_tolerance"),
    "snap_half": (dict(snap=0.5), INVALID, b"snap"),
    "snap_negative": (dict(snap=-1e-9), INVALID, b"snap"),
    "snap_nan": (dict(snap=NAN), INVALID, b"snap"),
    "reserved": (dict(reserved=1), INVALID, b"reserved"),
    "null_frame": (dict(frame=None), INVALID, b"null buffer: the frame"),
    "null_out_colour": (dict(okw=dict(colour=None)), INVALID, b"null buffer: out.colour"),
    "null_out_age": (dict(okw=dict(age=None)), INVALID, b"null buffer: out.age"),
    "null_history_depth": (dict(hkw=dict(depth=None)), INVALID, b"null buffer: history.depth"),
    "misaligned_frame": (dict(frame=FAKE + 4), INVALID, b"the frame is not 8-byte aligned"),
    "misaligned_out_m2": (dict(okw=dict(m2=OUT + IMAGE + 4)), INVALID, b"out.m2 is not 8-byte aligned"),
    "misaligned_out_index": (dict(okw=dict(index=OUT + 4 * IMAGE + 2)), INVALID, b"out.index is not 4-byte aligned"),
    "misaligned_history_m2": (dict(hkw=dict(m2=HIST + IMAGE + 4)), INVALID, b"history.m2 is not 8-byte aligned"),
    "misaligned_history_age": (dict(hkw=dict(age=HIST + 3 * IMAGE + 1)), INVALID,
                               b"history.age is not 4-byte aligned"),
    "misaligned_variance": (dict(variance=VARIANCE + 4), INVALID, b"the variance is not 8-byte aligned"),
    "misaligned_record": (dict(record=RECORD + 4), INVALID, b"the record is not 8-byte aligned"),
    "out_is_the_frame": (dict(frame=OUT), INVALID, b"out.colour overlaps the frame"),
    "out_m2_is_the_frame": (dict(frame=OUT + IMAGE), INVALID, b"out.m2 overlaps the frame"),
    "out_is_history": (dict(hkw=dict(colour=OUT)), INVALID, b"out.colour overlaps history.colour"),
    "out_m2_is_history_m2": (dict(hkw=dict(m2=OUT + IMAGE)), INVALID, b"out.m2 overlaps history.m2"),
    "out_colour_is_out_m2": (dict(okw=dict(m2=OUT + IMAGE - 8)), INVALID, b"out.colour overlaps out.m2"),
    "out_age_in_out_depth": (dict(okw=dict(age=OUT + 2 * IMAGE + 8 * PIXELS - 4)), INVALID,
                             b"out.age overlaps out.depth"),
    "variance_is_out_m2": (dict(variance=OUT + IMAGE), INVALID, b"out.m2 overlaps the variance"),
    "variance_is_the_frame": (dict(variance=FAKE + 8), INVALID, b"the variance overlaps the frame"),
    "variance_in_history_m2": (dict(variance=HIST + 2 * IMAGE - 8), INVALID, b"the variance overlaps history.m2"),
    "record_in_variance": (dict(record=VARIANCE + IMAGE - 8), INVALID, b"the variance overlaps the record"),
    "record_in_history_depth": (dict(record=HIST + 2 * IMAGE), INVALID, b"the record overlaps history.depth"),
    # without m2: the plain step's
    "plain_null_out_depth": (dict(m2=False, okw=dict(depth=None)), INVALID, b"null buffer: out.depth"),
    "plain_out_is_history": (dict(m2=False, hkw=dict(colour=OUT)), INVALID, b"out.colour overlaps history.colour"),
    "plain_misaligned_history_age": (dict(m2=False, hkw=dict(age=HIST + 3 * IMAGE + 1)), INVALID,
                                     b"history.age is not 4-byte aligned"),
}
# What the header adds:
MOTION_ERRORS = {
    "null_geometry_with_history": (dict(geometry=None), INVALID, b"null buffer: the previous geometry"),
    "plain_null_geometry_with_history": (dict(geometry=None, m2=False), INVALID,
                                         b"null buffer: the previous geometry"),
    "misaligned_geometry": (dict(geometry=GEOMETRY + 4), INVALID, b"the previous geometry is not 8-byte aligned"),
    "misaligned_motion": (dict(motion=MOTION + 4), INVALID, b"the motion plane is not 8-byte aligned"),
    "motion_is_the_frame": (dict(motion=FAKE + IMAGE - 8), INVALID, b"the motion plane overlaps the frame"),
    "motion_in_history_colour": (dict(motion=HIST + 8), INVALID, b"the motion plane overlaps history.colour"),
    "motion_is_out_colour": (dict(motion=OUT), INVALID, b"out.colour overlaps the motion plane"),
    "motion_in_variance": (dict(motion=VARIANCE + IMAGE - 8), INVALID, b"the variance overlaps the motion plane"),
    "record_in_motion": (dict(record=MOTION + 16 * PIXELS - 8), INVALID, b"the record overlaps the motion plane"),
    "motion_over_the_geometry": (dict(motion=GEOMETRY - 16 * PIXELS + 8), INVALID,
                                 b"the motion plane overlaps the previous geometry"),
    "out_depth_over_the_geometry": (dict(geometry=OUT + 2 * IMAGE + 8), INVALID,
                                    b"out.depth overlaps the previous geometry"),
    "variance_without_m2": (dict(m2=False, variance=VARIANCE + 8), INVALID, b"variance plane needs the m2"),
    "m2_of_out_alone": (dict(hkw=dict(m2=None)), INVALID, b"all be given or all be null"),
    "m2_of_history_alone": (dict(okw=dict(m2=None)), INVALID, b"all be given or all be null"),
}


@pytest.mark.parametrize("case", sorted(SHARED_ERRORS))
def test_the_older_steps_argument_errors_before_any_device_work(L, case):
    kw, status, word = SHARED_ERRORS[case]
    assert _step(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


@pytest.mark.parametrize("case", sorted(MOTION_ERRORS))
def test_the_new_argument_errors_before_any_device_work(L, case):
    kw, status, word = MOTION_ERRORS[case]
    assert _step(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_empty_image_is_ok_and_launches_nothing(L):
    """TRAY_OK before the (fake) scene or any plane is looked at, with or without m2 and a history."""
    for dims in (dict(width=0), dict(height=0), dict(width=0, height=0)):
        for m2 in (True, False):
            assert _step(L, m2=m2, okw=dims, hkw=dims) == L.TRAY_OK, dims
            assert _step(L, m2=m2, okw=dims, history=None, prev=None, frame=None, record=None, motion=None,
                         geometry=None, variance=None) == L.TRAY_OK, dims


def test_render_animation_refusals_without_a_device(L):
    """ValueError before any device work for what RenderAnimation's new arguments refuse; the wrapper
    raises TrayError for argument errors."""
    from tray_amd import ray

    t = ray.New(8, 6)
    scene = ray.DefaultScene()
    n = len(scene.Objects)
    geo = np.zeros((2, n, 4))
    cams = [ray.RichSceneCamera() for _ in range(2)]
    for kw in (dict(variance=True), dict(refill=2), dict(max_history=4), dict(refill_tolerance=0.5),
               dict(refill_dilate=0),                                                 # need temporal=True
               dict(temporal=True, refill=-1), dict(temporal=True, refill=1.5), dict(temporal=True, refill=True),
               dict(temporal=True, refill=1, max_history=1), dict(temporal=True, refill=1, refill_tolerance=NAN),
               dict(temporal=True, refill=1, refill_dilate=2), dict(temporal=True, history=4),
               dict(temporal=True, reserved=0), dict(temporal=True, cameras=cams[:1]),
               dict(temporal=True, cameras=cams + cams[:1]), dict(cameras=cams[:1]),
               dict(temporal=True, cameras=[cams[0], "camera"])):
        with pytest.raises(ValueError):
            t.RenderAnimation(scene, geo, **kw)
    with pytest.raises(L.TrayError) as e:
        L.temporal_motion_step_async(FAKE, L.CameraState(), None, None, n, L.temporal_params(snap=0.75), FAKE, None,
                                     _state(L, OUT), VARIANCE, MOTION)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "snap" in str(e.value)
    with pytest.raises(L.TrayError) as e:
        L.temporal_motion_step_async(FAKE, L.CameraState(), L.CameraState(), None, n, L.temporal_params(), FAKE,
                                     _state(L, HIST), _state(L, OUT), VARIANCE, MOTION)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "previous geometry" in str(e.value)
