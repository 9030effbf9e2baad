"""include/tray_denoise.h on the CPU: the denoiser is declared, exported and bound,
sits beside (not inside) the four older headers, the header is C99 and links from
C, argument errors are reported before any device work, and the workspace size is
monotone and sufficient. No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tray_denoise.h")
CALLER = os.path.join(ROOT, "tests", "c", "tray_denoise_caller.c")
OLDER = {"tray.h": "EXPORTS", "tray_query.h": "QUERY_EXPORTS", "tray_shade.h": "SHADE_EXPORTS",
         "tray_aov.h": "AOV_EXPORTS"}
FAKE = 0x100000  # a non-null "device pointer": validation fails before anything reads it
W, ROWS = 33, 17
IMAGE = W * ROWS * 24


def _declared(path=HEADER):
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(path).read(), re.M))


def test_denoise_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.DENOISE_EXPORTS) and len(declared) == 4
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_denoise_version() == 1
    text = open(HEADER).read()
    assert "#define TRAY_DENOISE_VERSION 1" in text and '#include "tray.h"' in text
    assert "#define TRAY_DENOISE_DEMODULATE 1" in text and L.DENOISE_DEMODULATE == 1


def test_older_headers_and_lists_unchanged_by_denoise(L):
    """The four older headers declare nothing of the new one; their export lists hold none of
    its symbols, keep their lengths and still match their headers; versions as before."""
    for header, listname in OLDER.items():
        text = open(os.path.join(INCLUDE, header)).read()
        assert "tray_denoise" not in text and "TRAY_DENOISE" not in text, header
        assert _declared(os.path.join(INCLUDE, header)) == set(getattr(L, listname)), header
        assert not set(L.DENOISE_EXPORTS) & set(getattr(L, listname)), header
    assert (len(L.EXPORTS), len(L.QUERY_EXPORTS), len(L.SHADE_EXPORTS), len(L.AOV_EXPORTS)) == (27, 4, 4, 2)
    lib = L.lib()
    assert lib.tray_abi_version() == 6 and lib.tray_query_version() == 1 and lib.tray_shade_version() == 1
    assert lib.tray_aov_version() == 1


def test_struct_layouts(L):
    assert ctypes.sizeof(L.DenoiseGuides) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in L.DenoiseGuides._fields_] == ["albedo", "normal", "depth"]
    assert [n for n, _ in L.DenoiseParams._fields_] == ["width", "rows", "iterations", "flags", "sigma_color",
                                                         "sigma_normal", "sigma_depth"]
    assert ctypes.sizeof(L.DenoiseParams) == 40 and L.DenoiseParams.sigma_color.offset == 16
    # the order of the fields in the header's structs
    text = open(HEADER).read()
    g = text[text.index("typedef struct tray_denoise_guides"):text.index("} tray_denoise_guides;")]
    assert re.findall(r"const double \*(\w+);", g) == ["albedo", "normal", "depth"]
    p = text[text.index("typedef struct tray_denoise_params"):text.index("} tray_denoise_params;")]
    assert re.findall(r"\b(width|rows|iterations|flags|sigma_color|sigma_normal|sigma_depth)\b[,;]", p) == \
        ["width", "rows", "iterations", "flags", "sigma_color", "sigma_normal", "sigma_depth"]


def test_header_is_c99_and_links(tmp_path):
    """tests/c/tray_denoise_caller.c includes the header and calls every entry point; it compiles
    as strict C99, links against the library, and its argument-error calls run without a device."""
    text = open(CALLER).read()
    for name in ("tray_denoise_version", "tray_denoise_default_params", "tray_denoise_workspace_bytes",
                 "tray_denoise_async"):
        assert name + "(" in text, name
    exe = str(tmp_path / "tray_denoise_caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, CALLER, "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)


def test_default_params(L):
    p = L.denoise_params(1280, 720)
    assert (p.width, p.rows, p.iterations, p.flags) == (1280, 720, 5, L.DENOISE_DEMODULATE)
    for s in (p.sigma_color, p.sigma_normal, p.sigma_depth):
        assert 0 < s < float("inf")
    assert L.lib().tray_denoise_default_params(4, 4, None) == L.TRAY_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        L.denoise_params(4, 4, sigma_colour=1.0)


def _call(L, colour=FAKE, guides="all", params="ok", out=FAKE + 4 * IMAGE, workspace=FAKE + 8 * IMAGE,
          workspace_bytes=None, **pkw):
    p = L.denoise_params(W, ROWS)
    for name, value in pkw.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    need = ctypes.c_size_t(0)
    L.lib().tray_denoise_workspace_bytes(ctypes.byref(p), ctypes.byref(need))
    g = {"all": L.DenoiseGuides(FAKE + 16 * IMAGE, FAKE + 20 * IMAGE, FAKE + 24 * IMAGE), None: None,
         "no_albedo": L.DenoiseGuides(None, FAKE + 20 * IMAGE, FAKE + 24 * IMAGE)}[guides]
    return L.lib().tray_denoise_async(colour, ctypes.byref(g) if g is not None else None,
                                      ctypes.byref(p) if params == "ok" else None, out, workspace,
                                      need.value if workspace_bytes is None else workspace_bytes, 0, None)


INF, NAN = float("inf"), float("nan")
ERRORS = {
    "null_colour": (dict(colour=None), "TRAY_ERR_INVALID_ARGUMENT", b"null colour"),
    "null_guides": (dict(guides=None), "TRAY_ERR_INVALID_ARGUMENT", b"null guides"),
    "null_params": (dict(params=None), "TRAY_ERR_INVALID_ARGUMENT", b"null params"),
    "null_out": (dict(out=None), "TRAY_ERR_INVALID_ARGUMENT", b"null out"),
    "workspace_one_byte_short": (dict(workspace_bytes=2 * IMAGE - 1), "TRAY_ERR_INVALID_ARGUMENT", b"workspace"),
    "workspace_null": (dict(workspace=None), "TRAY_ERR_INVALID_ARGUMENT", b"workspace"),
    "iterations_0": (dict(iterations=0), "TRAY_ERR_INVALID_ARGUMENT", b"iterations"),
    "iterations_9": (dict(iterations=9), "TRAY_ERR_INVALID_ARGUMENT", b"iterations"),
    "unknown_flag": (dict(flags=3), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
    "sigma_color_zero": (dict(sigma_color=0.0), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_color"),
    "sigma_color_nan": (dict(sigma_color=NAN), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_color"),
    "sigma_normal_negative": (dict(sigma_normal=-1.0), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_normal"),
    "sigma_normal_inf": (dict(sigma_normal=INF), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_normal"),
    "sigma_depth_zero": (dict(sigma_depth=-0.0), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_depth"),
    "sigma_depth_inf": (dict(sigma_depth=INF), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_depth"),
    "demodulate_without_albedo": (dict(guides="no_albedo"), "TRAY_ERR_INVALID_ARGUMENT", b"albedo"),
    "out_is_colour": (dict(out=FAKE), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps colour"),
    "out_overlaps_colour_end": (dict(out=FAKE + IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps colour"),
    "out_overlaps_colour_start": (dict(out=FAKE - IMAGE + 8), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps colour"),
    "out_is_workspace": (dict(out=FAKE + 8 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps the workspace"),
    "out_in_workspace_second_image": (dict(out=FAKE + 10 * IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT",
                                      b"overlaps the workspace"),
    "negative_width": (dict(width=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative"),
    "pixels_2_31": (dict(width=2 ** 16, rows=2 ** 15), "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels"),
    # the header's rule: level 7 (s = 128) of 33 x 2^25 needs 1 * 32768 * 33 * 128 workgroups > 2^24 - 1
    "workgroups_2_24": (dict(width=33, rows=2 ** 25, iterations=8, out=FAKE + 2 ** 40), "TRAY_ERR_TOO_LARGE",
                        b"2^24 - 1 workgroups"),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_argument_errors_before_any_device_work(L, case):
    kw, status, word = ERRORS[case]
    assert _call(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_workgroup_limit_is_the_headers_formula(L):
    """Any level above the limit refuses the call: 33 x 2^25 stays below it at s = 1 and 2
    (2^23 workgroups each) and passes it at s = 4 (1 * 2^20 * 4 * 4 = 2^24), so 3 iterations are
    refused. (2 iterations would pass validation and go on to the device: not tried with fake
    pointers.)"""
    from math import ceil

    def blocks(w, r, s):
        return ceil(ceil(w / s) / 32) * ceil(ceil(r / s) / 8) * min(s, w) * min(s, r)

    assert blocks(33, 2 ** 25, 128) > 2 ** 24 - 1 and blocks(33, 2 ** 25, 64) > 2 ** 24 - 1
    assert max(blocks(33, 2 ** 25, 1 << i) for i in range(2)) <= 2 ** 24 - 1 < blocks(33, 2 ** 25, 4)
    far = FAKE + 2 ** 40
    assert _call(L, width=33, rows=2 ** 25, iterations=3, out=far, workspace=far + 2 ** 40) == L.TRAY_ERR_TOO_LARGE
    assert b"2^24 - 1 workgroups" in L.lib().tray_last_error()
    assert max(blocks(1280, 720, 1 << i) for i in range(8)) == 16384


def test_empty_image_is_ok_and_launches_nothing(L):
    """With no pixels the call returns TRAY_OK before any (fake) buffer or device is looked at."""
    for kw in (dict(width=0), dict(rows=0), dict(width=0, rows=0), dict(rows=0, iterations=1, flags=0)):
        assert _call(L, **kw) == L.TRAY_OK, kw
    assert _call(L, rows=0, workspace=None, workspace_bytes=0) == L.TRAY_OK


def test_workspace_bytes_is_monotone_and_sufficient(L):
    """Sufficient: what the launches need is an image per ping-pong buffer in use, which is
    min(iterations - 1, 2) images of rows x width x 3 doubles (the last level writes `out`).
    Monotone in width, rows and iterations. Errors as for the call."""
    def need(w, rows, it):
        return L.denoise_workspace_bytes(L.denoise_params(w, rows, iterations=it))

    for w, rows in ((1, 1), (37, 23), (1280, 720), (46340, 46340)):
        for it in range(1, 9):
            assert need(w, rows, it) == min(it - 1, 2) * w * rows * 24, (w, rows, it)
            assert need(w, rows, it) <= need(w + 1, rows, it) and need(w, rows, it) <= need(w, rows + 1, it)
            assert it == 8 or need(w, rows, it) <= need(w, rows, it + 1)
    assert need(0, 5, 5) == 0 and need(5, 0, 5) == 0
    n = ctypes.c_size_t(0)
    bad = L.denoise_params(4, 4, iterations=0)
    assert L.lib().tray_denoise_workspace_bytes(ctypes.byref(bad), ctypes.byref(n)) == L.TRAY_ERR_INVALID_ARGUMENT
    assert L.lib().tray_denoise_workspace_bytes(None, ctypes.byref(n)) == L.TRAY_ERR_INVALID_ARGUMENT
    assert L.lib().tray_denoise_workspace_bytes(ctypes.byref(L.denoise_params(4, 4)), None) == \
        L.TRAY_ERR_INVALID_ARGUMENT
    big = L.denoise_params(2 ** 16, 2 ** 15)
    assert L.lib().tray_denoise_workspace_bytes(ctypes.byref(big), ctypes.byref(n)) == L.TRAY_ERR_TOO_LARGE


def test_mirror_refuses_without_a_device(L):
    """Tracer.Denoise refuses interleaved row sets and partial or misshapen frames with
    ValueError before any device work; the wrapper raises TrayError for argument errors."""
    import numpy as np

    from tray_amd import ray

    t = ray.New(8, 6)
    assert callable(t.Denoise) and callable(t.RenderDenoised)
    frame = np.zeros((6, 8, 3))
    with pytest.raises(ValueError, match="contiguous"):
        t.Denoise(frame, {}, tile_rows=2)
    with pytest.raises(ValueError):
        t.Denoise(frame[:4], {})  # rows [0, 6) asked for, 4 given
    with pytest.raises(ValueError):
        t.Denoise(frame[:, :7], {})
    with pytest.raises(ValueError):
        t.Denoise(frame, {"depth": np.zeros((6, 7))}, flags=0)
    with pytest.raises(ValueError):
        t.Denoise(frame, {}, yStart=2, yEnd=7)
    with pytest.raises(L.TrayError) as e:
        L.denoise_async(FAKE, L.denoise_params(8, 6, iterations=9), FAKE + 4 * IMAGE, None, 0)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "iterations" in str(e.value)
