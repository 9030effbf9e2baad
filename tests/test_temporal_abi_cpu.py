"""include/tray_temporal.h on the CPU: the reprojection step is declared, exported and bound, sits
beside (not inside) the seven older headers, the header is C99 and links from C, and argument errors
are reported before any device work. No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tray_temporal.h")
CALLER = os.path.join(ROOT, "tests", "c", "tray_temporal_caller.c")
OLDER = {"tray.h": "EXPORTS", "tray_query.h": "QUERY_EXPORTS", "tray_shade.h": "SHADE_EXPORTS",
         "tray_aov.h": "AOV_EXPORTS", "tray_denoise.h": "DENOISE_EXPORTS", "tray_progressive.h": "PROGRESSIVE_EXPORTS",
         "tray_adaptive.h": "ADAPTIVE_EXPORTS"}
FAKE = 0x100000  # a non-null "device pointer": validation fails before anything reads it
W, H = 33, 17
PIXELS = W * H
IMAGE = PIXELS * 24
INF, NAN = float("inf"), float("nan")


def _declared(path=HEADER):
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(path).read(), re.M))


def test_temporal_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.TEMPORAL_EXPORTS) and len(declared) == len(L.TEMPORAL_EXPORTS) == 3
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_temporal_version() == 1
    text = open(HEADER).read()
    assert "#define TRAY_TEMPORAL_VERSION 1" in text and '#include "tray.h"' in text
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in L.TEMPORAL_EXPORTS:
        assert re.search(rf"\bT {name}\b", out), name


def test_older_headers_and_lists_unchanged_by_temporal(L):
    """The seven older headers declare nothing of the new one; their export lists hold none of its
    symbols, keep their lengths and still match their headers; versions as before."""
    for header, listname in OLDER.items():
        text = open(os.path.join(INCLUDE, header)).read()
        for word in ("tray_temporal", "TRAY_TEMPORAL"):
            assert word not in text, (header, word)
        assert _declared(os.path.join(INCLUDE, header)) == set(getattr(L, listname)), header
        assert not set(L.TEMPORAL_EXPORTS) & set(getattr(L, listname)), header
    assert (len(L.EXPORTS), len(L.QUERY_EXPORTS), len(L.SHADE_EXPORTS), len(L.AOV_EXPORTS), len(L.DENOISE_EXPORTS),
            len(L.PROGRESSIVE_EXPORTS), len(L.ADAPTIVE_EXPORTS)) == (27, 4, 4, 2, 4, 7, 6)
    lib = L.lib()
    assert lib.tray_abi_version() == 6 and lib.tray_query_version() == 1 and lib.tray_shade_version() == 1
    assert lib.tray_aov_version() == 1 and lib.tray_denoise_version() == 1 and lib.tray_progressive_version() == 1
    assert lib.tray_adaptive_version() == 1


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
    for name, cls, size in (("tray_temporal_state", L.TemporalState, 4 * ptr + 8),
                            ("tray_temporal_params", L.TemporalParams, 32),
                            ("tray_temporal_record", L.TemporalRecord, 16)):
        assert _struct_fields(text, name) == [n for n, _ in cls._fields_], name
        assert ctypes.sizeof(cls) == size, name
    assert L.TemporalState.depth.offset == 3 * ptr and L.TemporalState.width.offset == 4 * ptr
    assert (L.TemporalParams.flags.offset, L.TemporalParams.depth_tolerance.offset, L.TemporalParams.snap.offset,
            L.TemporalParams.reserved.offset) == (4, 8, 16, 24)
    assert [L.TEMPORAL_RECORD_DTYPE.fields[n][1] for n in ("fresh", "age_sum")] == [0, 8] == \
        [getattr(L.TemporalRecord, n).offset for n, _ in L.TemporalRecord._fields_]


def test_header_is_c99_and_links(tmp_path):
    """tests/c/tray_temporal_caller.c includes the header and calls every entry point; it compiles as
    strict C99, links against the library, and its argument-error calls run without a device."""
    from tray_amd import _lib

    text = open(CALLER).read()
    for name in _lib.TEMPORAL_EXPORTS:
        assert name + "(" in text, name
    exe = str(tmp_path / "tray_temporal_caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, CALLER, "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)


def test_default_params(L):
    p = L.temporal_params()
    assert p.max_history in (8, 16, 32, 64) and p.depth_tolerance in (0.02, 0.1, 0.5)  # a row of the sweep
    assert (p.snap, p.flags, p.reserved) == (2.0 ** -20, 0, 0)
    assert L.temporal_params(max_history=3).max_history == 3
    assert L.lib().tray_temporal_default_params(None) == L.TRAY_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        L.temporal_params(history=3)


# The frame at FAKE; out's colour, depth, age, index at + 2, 4, 5, 6 images; the history's at + 8, 10, 11, 12;
# the record at + 14.
def _state(L, base, width=W, height=H, **absolute):
    at = dict(colour=base, depth=base + 2 * IMAGE, age=base + 3 * IMAGE, index=base + 4 * IMAGE)
    assert set(absolute) <= set(at), absolute
    at.update(absolute)
    return L.TemporalState(at["colour"], at["age"], at["index"], at["depth"], width, height)


def _step(L, scene=FAKE, camera="ok", prev="ok", params="ok", frame=FAKE, history="ok", out="ok",
          record=FAKE + 14 * IMAGE, okw=None, hkw=None, **pkw):
    tp = L.temporal_params()
    for name, value in pkw.items():
        assert hasattr(tp, name), name
        setattr(tp, name, value)
    cam, pcam = L.CameraState(), L.CameraState()
    o = _state(L, FAKE + 2 * IMAGE, **(okw or {}))
    hs = _state(L, FAKE + 8 * IMAGE, **(hkw or {}))
    return L.lib().tray_temporal_step_async(
        scene, ctypes.byref(cam) if camera == "ok" else None, ctypes.byref(pcam) if prev == "ok" else None,
        ctypes.byref(tp) if params == "ok" else None, frame, ctypes.byref(hs) if history == "ok" else None,
        ctypes.byref(o) if out == "ok" else None, record, None)


OUT = FAKE + 2 * IMAGE
STEP_ERRORS = {
    "null_scene": (dict(scene=None), "TRAY_ERR_INVALID_ARGUMENT", b"null scene"),
    "null_camera": (dict(camera=None), "TRAY_ERR_INVALID_ARGUMENT", b"null camera"),
    "null_params": (dict(params=None), "TRAY_ERR_INVALID_ARGUMENT", b"null params"),
    "null_out": (dict(out=None), "TRAY_ERR_INVALID_ARGUMENT", b"null state"),
    "history_without_camera": (dict(prev=None), "TRAY_ERR_INVALID_ARGUMENT", b"both"),
    "camera_without_history": (dict(history=None), "TRAY_ERR_INVALID_ARGUMENT", b"both"),
    "negative_width": (dict(okw=dict(width=-1), hkw=dict(width=-1)), "TRAY_ERR_INVALID_ARGUMENT", b"negative width"),
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
    "null_out_age": (dict(okw=dict(age=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: out.age"),
    "null_history_depth": (dict(hkw=dict(depth=None)), "TRAY_ERR_INVALID_ARGUMENT", b"null buffer: history.depth"),
    "misaligned_frame": (dict(frame=FAKE + 4), "TRAY_ERR_INVALID_ARGUMENT", b"the frame is not 8-byte aligned"),
    "misaligned_out_depth": (dict(okw=dict(depth=OUT + 2 * IMAGE + 4)), "TRAY_ERR_INVALID_ARGUMENT",
                             b"out.depth is not 8-byte aligned"),
    "misaligned_out_index": (dict(okw=dict(index=OUT + 4 * IMAGE + 2)), "TRAY_ERR_INVALID_ARGUMENT",
                             b"out.index is not 4-byte aligned"),
    "misaligned_history_age": (dict(hkw=dict(age=FAKE + 11 * IMAGE + 1)), "TRAY_ERR_INVALID_ARGUMENT",
                               b"history.age is not 4-byte aligned"),
    "misaligned_record": (dict(record=FAKE + 14 * IMAGE + 4), "TRAY_ERR_INVALID_ARGUMENT",
                          b"the record is not 8-byte aligned"),
    "out_is_the_frame": (dict(frame=OUT), "TRAY_ERR_INVALID_ARGUMENT", b"out.colour overlaps the frame"),
    "out_is_history": (dict(hkw=dict(colour=OUT)), "TRAY_ERR_INVALID_ARGUMENT", b"out.colour overlaps history.colour"),
    "out_colour_end_in_history": (dict(hkw=dict(colour=OUT + IMAGE - 8)), "TRAY_ERR_INVALID_ARGUMENT",
                                  b"out.colour overlaps history.colour"),
    "out_age_in_out_depth": (dict(okw=dict(age=OUT + 2 * IMAGE + 8 * PIXELS - 4)), "TRAY_ERR_INVALID_ARGUMENT",
                             b"out.age overlaps out.depth"),
    "out_index_in_history_age": (dict(okw=dict(index=FAKE + 11 * IMAGE)), "TRAY_ERR_INVALID_ARGUMENT",
                                 b"out.index overlaps history.age"),
    "record_in_out_colour": (dict(record=OUT + IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT",
                             b"out.colour overlaps the record"),
    "record_in_history_depth": (dict(record=FAKE + 10 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT",
                                b"the record overlaps history.depth"),
}


@pytest.mark.parametrize("case", sorted(STEP_ERRORS))
def test_step_argument_errors_before_any_device_work(L, case):
    kw, status, word = STEP_ERRORS[case]
    assert _step(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_empty_image_is_ok_and_launches_nothing(L):
    """TRAY_OK before the (fake) scene or any plane is looked at, with and without a history."""
    for dims in (dict(width=0), dict(height=0), dict(width=0, height=0)):
        assert _step(L, okw=dims, hkw=dims) == L.TRAY_OK, dims
        assert _step(L, okw=dims, history=None, prev=None, frame=None, record=None) == L.TRAY_OK, dims
    none = dict(colour=None, age=None, index=None, depth=None, height=0)
    assert _step(L, okw=none, hkw=none, frame=None, record=None) == L.TRAY_OK


def test_render_sequence_refuses_bad_input_without_a_device(L):
    """ValueError for an empty sequence, an entry that is no Camera and unknown or misshapen overrides,
    before any device work; the wrapper raises TrayError for argument errors."""
    from tray_amd import ray

    t = ray.New(8, 6)
    assert callable(t.RenderSequence)
    cams = [ray.RichSceneCamera()]
    for bad in ([], None, [cams[0], "camera"], [(13.0, 2.0, 3.0)]):
        with pytest.raises(ValueError):
            t.RenderSequence(None, bad)
    for kw in (dict(history=4), dict(reserved=0), dict(sigma_color=1.0)):
        with pytest.raises(ValueError):
            t.RenderSequence(None, cams, **kw)
    with pytest.raises(L.TrayError) as e:
        L.temporal_step_async(FAKE, L.CameraState(), None, L.temporal_params(snap=0.75), FAKE, None,
                              _state(L, OUT))
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "snap" in str(e.value)
    step = ray.ORBIT_STEP_DEGREES
    assert step > 0
    a = ray.Orbit(ray.RichSceneCamera(), 0.0)
    b = ray.Orbit(ray.RichSceneCamera(), 360.0)
    assert a.Position == ray.RichSceneCamera().Position and max(abs(p - q) for p, q in zip(a.Position, b.Position)) < 1e-12
    c = ray.Orbit(ray.RichSceneCamera(), 90.0)  # about +y from (13, 2, 3): (3, 2, -13)
    assert max(abs(p - q) for p, q in zip(c.Position, (3.0, 2.0, -13.0))) < 1e-12
