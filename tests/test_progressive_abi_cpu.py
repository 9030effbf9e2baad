"""include/tray_progressive.h on the CPU: the accumulator, its metric and the
variance-guided filter are declared, exported and bound, sit beside (not inside) the five
older headers, the header is C99 and links from C, argument errors are reported before any
device work, and the workspace size follows its formula. No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tray_progressive.h")
CALLER = os.path.join(ROOT, "tests", "c", "tray_progressive_caller.c")
OLDER = {"tray.h": "EXPORTS", "tray_query.h": "QUERY_EXPORTS", "tray_shade.h": "SHADE_EXPORTS",
         "tray_aov.h": "AOV_EXPORTS", "tray_denoise.h": "DENOISE_EXPORTS"}
FAKE = 0x100000  # a non-null "device pointer": validation fails before anything reads it
W, ROWS = 33, 17
IMAGE = W * ROWS * 24
INF, NAN = float("inf"), float("nan")


def _declared(path=HEADER):
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(path).read(), re.M))


def test_progressive_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.PROGRESSIVE_EXPORTS) and len(declared) == len(L.PROGRESSIVE_EXPORTS) == 7
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.tray_progressive_version() == 1
    text = open(HEADER).read()
    assert "#define TRAY_PROGRESSIVE_VERSION 1" in text
    assert '#include "tray.h"' in text and '#include "tray_denoise.h"' in text
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in L.PROGRESSIVE_EXPORTS:
        assert re.search(rf"\bT {name}\b", out), name


def test_older_headers_and_lists_unchanged_by_progressive(L):
    """The five older headers declare nothing of the new one; their export lists hold none of its
    symbols, keep their lengths and still match their headers; versions as before."""
    for header, listname in OLDER.items():
        text = open(os.path.join(INCLUDE, header)).read()
        for word in ("tray_progressive", "TRAY_PROGRESSIVE", "tray_accum", "tray_denoise_variance"):
            assert word not in text, (header, word)
        assert _declared(os.path.join(INCLUDE, header)) == set(getattr(L, listname)), header
        assert not set(L.PROGRESSIVE_EXPORTS) & set(getattr(L, listname)), header
    assert (len(L.EXPORTS), len(L.QUERY_EXPORTS), len(L.SHADE_EXPORTS), len(L.AOV_EXPORTS),
            len(L.DENOISE_EXPORTS)) == (27, 4, 4, 2, 4)
    lib = L.lib()
    assert lib.tray_abi_version() == 6 and lib.tray_query_version() == 1 and lib.tray_shade_version() == 1
    assert lib.tray_aov_version() == 1 and lib.tray_denoise_version() == 1


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
    for name, cls, size in (("tray_accum", L.Accum, 2 * ptr + 16),
                            ("tray_accum_metric_params", L.AccumMetricParams, 16),
                            ("tray_accum_metric", L.AccumMetric, 16),
                            ("tray_denoise_variance_params", L.DenoiseVarianceParams, 48)):
        assert _struct_fields(text, name) == [n for n, _ in cls._fields_], name
        assert ctypes.sizeof(cls) == size, name
    assert L.Accum.width.offset == 2 * ptr and L.Accum.count.offset == 2 * ptr + 8
    assert L.AccumMetric.max_ratio.offset == 8 and L.ACCUM_METRIC_DTYPE.fields["max_ratio"][1] == 8
    assert L.DenoiseVarianceParams.sigma_variance.offset == 16 and L.DenoiseVarianceParams.epsilon.offset == 40


def test_header_is_c99_and_links(tmp_path):
    """tests/c/tray_progressive_caller.c includes the header and calls every entry point; it
    compiles as strict C99, links against the library, and its argument-error calls run without
    a device."""
    from tray_amd import _lib

    text = open(CALLER).read()
    for name in _lib.PROGRESSIVE_EXPORTS:
        assert name + "(" in text, name
    exe = str(tmp_path / "tray_progressive_caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, CALLER, "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)


def test_default_params(L):
    mp = L.accum_metric_params()
    assert mp.tolerance == 0.05 and mp.floor == 2.0 ** -10
    assert L.accum_metric_params(tolerance=0.5).tolerance == 0.5
    assert L.lib().tray_accum_metric_default_params(None) == L.TRAY_ERR_INVALID_ARGUMENT
    p = L.denoise_variance_params(1280, 720)
    assert (p.width, p.rows, p.iterations, p.flags) == (1280, 720, 5, L.DENOISE_DEMODULATE)
    d = L.denoise_params(1280, 720)
    assert (p.sigma_normal, p.sigma_depth) == (d.sigma_normal, d.sigma_depth)  # the guides' terms are the same filter
    assert 0 < p.sigma_variance < INF and 0 < p.epsilon < 1e-6
    assert L.lib().tray_denoise_variance_default_params(4, 4, None) == L.TRAY_ERR_INVALID_ARGUMENT
    assert L.lib().tray_denoise_variance_default_params(-1, 4, ctypes.byref(p)) == L.TRAY_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        L.denoise_variance_params(4, 4, sigma_color=1.0)
    with pytest.raises(ValueError):
        L.accum_metric_params(tol=1.0)


# ------------------------------------------------------------- the accumulator --
def _fold(L, mean=FAKE, m2=FAKE + 2 * IMAGE, frames=FAKE + 8 * IMAGE, n_frames=3, width=W, rows=ROWS, count=0,
          reserved=0, acc="ok", metric=False, mp="ok", variance=None, record=None, **mpkw):
    a = L.Accum(mean, m2, width, rows, count, reserved)
    ref = ctypes.byref(a) if acc == "ok" else None
    if not metric:
        rc = L.lib().tray_accum_fold_async(ref, frames, n_frames, 0, None)
    else:
        p = L.accum_metric_params(**mpkw)
        rc = L.lib().tray_accum_fold_metric_async(ref, frames, n_frames, ctypes.byref(p) if mp == "ok" else None,
                                                  variance, record, 0, None)
    return rc, a.count


FOLD_ERRORS = {
    "null_acc": (dict(acc=None), "TRAY_ERR_INVALID_ARGUMENT", b"null acc"),
    "null_mean": (dict(mean=None), "TRAY_ERR_INVALID_ARGUMENT", b"null mean or m2"),
    "null_m2": (dict(m2=None), "TRAY_ERR_INVALID_ARGUMENT", b"null mean or m2"),
    "null_frames": (dict(frames=None), "TRAY_ERR_INVALID_ARGUMENT", b"null frames"),
    "negative_width": (dict(width=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative width or rows"),
    "negative_rows": (dict(rows=-5), "TRAY_ERR_INVALID_ARGUMENT", b"negative width or rows"),
    "negative_count": (dict(count=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative count"),
    "negative_n_frames": (dict(n_frames=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative n_frames"),
    "reserved": (dict(reserved=1), "TRAY_ERR_INVALID_ARGUMENT", b"reserved"),
    "count_overflow": (dict(count=2 ** 31 - 2, n_frames=2), "TRAY_ERR_INVALID_ARGUMENT", b"overflows int32"),
    "pixels_2_31": (dict(width=2 ** 16, rows=2 ** 15), "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels"),
    "misaligned_mean": (dict(mean=FAKE + 4), "TRAY_ERR_INVALID_ARGUMENT", b"8-byte aligned"),
    "misaligned_frames": (dict(frames=FAKE + 8 * IMAGE + 2), "TRAY_ERR_INVALID_ARGUMENT", b"8-byte aligned"),
    "mean_is_m2": (dict(m2=FAKE), "TRAY_ERR_INVALID_ARGUMENT", b"mean overlaps m2"),
    "m2_overlaps_mean_end": (dict(m2=FAKE + IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"mean overlaps m2"),
    "mean_in_last_frame": (dict(mean=FAKE + 11 * IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps the frames"),
    "m2_before_first_frame": (dict(m2=FAKE + 7 * IMAGE + 8), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps the frames"),
    "null_metric_params": (dict(metric=True, mp=None), "TRAY_ERR_INVALID_ARGUMENT", b"null metric params"),
    "tolerance_negative": (dict(metric=True, tolerance=-1.0), "TRAY_ERR_INVALID_ARGUMENT", b"tolerance"),
    "tolerance_nan": (dict(metric=True, tolerance=NAN), "TRAY_ERR_INVALID_ARGUMENT", b"tolerance"),
    "tolerance_inf": (dict(metric=True, tolerance=INF), "TRAY_ERR_INVALID_ARGUMENT", b"tolerance"),
    "floor_zero": (dict(metric=True, floor=0.0), "TRAY_ERR_INVALID_ARGUMENT", b"floor"),
    "floor_inf": (dict(metric=True, floor=INF), "TRAY_ERR_INVALID_ARGUMENT", b"floor"),
    "nothing_to_evaluate": (dict(metric=True, n_frames=0, record=FAKE + 20 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT",
                            b"nothing to evaluate"),
    "variance_is_mean": (dict(metric=True, variance=FAKE), "TRAY_ERR_INVALID_ARGUMENT", b"variance overlaps"),
    "variance_in_frames": (dict(metric=True, variance=FAKE + 9 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT",
                           b"variance overlaps"),
    "record_in_m2": (dict(metric=True, record=FAKE + 2 * IMAGE + 8), "TRAY_ERR_INVALID_ARGUMENT", b"metric record"),
    "record_in_variance": (dict(metric=True, variance=FAKE + 20 * IMAGE, record=FAKE + 21 * IMAGE - 8),
                           "TRAY_ERR_INVALID_ARGUMENT", b"metric record"),
    "misaligned_record": (dict(metric=True, record=FAKE + 30 * IMAGE + 4), "TRAY_ERR_INVALID_ARGUMENT",
                          b"8-byte aligned"),
}


@pytest.mark.parametrize("case", sorted(FOLD_ERRORS))
def test_fold_argument_errors_before_any_device_work(L, case):
    kw, status, word = FOLD_ERRORS[case]
    rc, count = _fold(L, **kw)
    assert rc == getattr(L, status) and count == kw.get("count", 0)  # and the count is left alone
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_fold_of_nothing_is_ok_and_launches_nothing(L):
    """An empty image, or no frames, returns TRAY_OK before any (fake) buffer or device is looked
    at, and leaves the count alone."""
    for kw in (dict(width=0), dict(rows=0), dict(n_frames=0), dict(n_frames=0, frames=None),
               dict(width=0, metric=True, variance=FAKE + 20 * IMAGE, record=FAKE + 30 * IMAGE),
               dict(n_frames=0, count=3, metric=True)):  # no outputs asked for, nothing to fold
        assert _fold(L, **kw) == (L.TRAY_OK, kw.get("count", 0)), kw


# ------------------------------------------------------------------ the filter --
def _call(L, colour=FAKE, variance=FAKE + 2 * IMAGE, guides="all", params="ok", out=FAKE + 4 * IMAGE,
          variance_out=None, workspace=FAKE + 8 * IMAGE, workspace_bytes=None, **pkw):
    p = L.denoise_variance_params(W, ROWS)
    for name, value in pkw.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    need = ctypes.c_size_t(0)
    L.lib().tray_denoise_variance_workspace_bytes(ctypes.byref(p), ctypes.byref(need))
    g = {"all": L.DenoiseGuides(FAKE + 16 * IMAGE, FAKE + 20 * IMAGE, FAKE + 24 * IMAGE), None: None,
         "no_albedo": L.DenoiseGuides(None, FAKE + 20 * IMAGE, FAKE + 24 * IMAGE)}[guides]
    return L.lib().tray_denoise_variance_async(colour, variance, ctypes.byref(g) if g is not None else None,
                                               ctypes.byref(p) if params == "ok" else None, out, variance_out,
                                               workspace, need.value if workspace_bytes is None else workspace_bytes,
                                               0, None)


WORK = 2 * W * ROWS * 32  # two images and two planes
ERRORS = {
    "null_colour": (dict(colour=None), "TRAY_ERR_INVALID_ARGUMENT", b"null colour"),
    "null_variance": (dict(variance=None), "TRAY_ERR_INVALID_ARGUMENT", b"null variance"),
    "null_guides": (dict(guides=None), "TRAY_ERR_INVALID_ARGUMENT", b"null guides"),
    "null_params": (dict(params=None), "TRAY_ERR_INVALID_ARGUMENT", b"null params"),
    "null_out": (dict(out=None), "TRAY_ERR_INVALID_ARGUMENT", b"null out"),
    "workspace_one_byte_short": (dict(workspace_bytes=WORK - 1), "TRAY_ERR_INVALID_ARGUMENT", b"workspace"),
    "workspace_null": (dict(workspace=None), "TRAY_ERR_INVALID_ARGUMENT", b"workspace"),
    "iterations_0": (dict(iterations=0), "TRAY_ERR_INVALID_ARGUMENT", b"iterations"),
    "iterations_9": (dict(iterations=9), "TRAY_ERR_INVALID_ARGUMENT", b"iterations"),
    "unknown_flag": (dict(flags=3), "TRAY_ERR_INVALID_ARGUMENT", b"flags"),
    "sigma_variance_zero": (dict(sigma_variance=0.0), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_variance"),
    "sigma_variance_nan": (dict(sigma_variance=NAN), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_variance"),
    "sigma_variance_inf": (dict(sigma_variance=INF), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_variance"),
    "epsilon_zero": (dict(epsilon=0.0), "TRAY_ERR_INVALID_ARGUMENT", b"epsilon"),
    "epsilon_negative": (dict(epsilon=-1e-12), "TRAY_ERR_INVALID_ARGUMENT", b"epsilon"),
    "epsilon_inf": (dict(epsilon=INF), "TRAY_ERR_INVALID_ARGUMENT", b"epsilon"),
    "sigma_normal_negative": (dict(sigma_normal=-1.0), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_normal"),
    "sigma_depth_inf": (dict(sigma_depth=INF), "TRAY_ERR_INVALID_ARGUMENT", b"sigma_depth"),
    "demodulate_without_albedo": (dict(guides="no_albedo"), "TRAY_ERR_INVALID_ARGUMENT", b"albedo"),
    "out_is_colour": (dict(out=FAKE), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps colour"),
    "out_overlaps_colour_end": (dict(out=FAKE + IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps colour"),
    "out_is_variance": (dict(out=FAKE + 2 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps variance"),
    "out_is_workspace": (dict(out=FAKE + 8 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"overlaps the workspace"),
    "out_in_workspace_planes": (dict(out=FAKE + 8 * IMAGE + WORK - 8), "TRAY_ERR_INVALID_ARGUMENT",
                                b"overlaps the workspace"),
    "variance_out_in_out": (dict(variance_out=FAKE + 5 * IMAGE - 8), "TRAY_ERR_INVALID_ARGUMENT", b"variance_out"),
    "variance_out_in_colour": (dict(variance_out=FAKE + 8), "TRAY_ERR_INVALID_ARGUMENT", b"variance_out"),
    "variance_out_in_variance": (dict(variance_out=FAKE + 2 * IMAGE), "TRAY_ERR_INVALID_ARGUMENT", b"variance_out"),
    "variance_out_in_workspace": (dict(variance_out=FAKE + 8 * IMAGE + WORK - 8), "TRAY_ERR_INVALID_ARGUMENT",
                                  b"variance_out"),
    "negative_width": (dict(width=-1), "TRAY_ERR_INVALID_ARGUMENT", b"negative"),
    "pixels_2_31": (dict(width=2 ** 16, rows=2 ** 15), "TRAY_ERR_TOO_LARGE", b"2^31 - 1 pixels"),
    # the rule of tray_denoise.h: level 7 (s = 128) of 33 x 2^25 needs 1 * 32768 * 33 * 128 workgroups > 2^24 - 1
    "workgroups_2_24": (dict(width=33, rows=2 ** 25, iterations=8, out=FAKE + 2 ** 40, variance=FAKE + 2 ** 41,
                             workspace=FAKE + 2 ** 42), "TRAY_ERR_TOO_LARGE", b"2^24 - 1 workgroups"),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_filter_argument_errors_before_any_device_work(L, case):
    kw, status, word = ERRORS[case]
    assert _call(L, **kw) == getattr(L, status)
    msg = L.lib().tray_last_error()
    assert msg and word in msg, msg


def test_filter_empty_image_is_ok_and_launches_nothing(L):
    for kw in (dict(width=0), dict(rows=0), dict(width=0, rows=0), dict(rows=0, iterations=1, flags=0)):
        assert _call(L, **kw) == L.TRAY_OK, kw
    assert _call(L, rows=0, workspace=None, workspace_bytes=0) == L.TRAY_OK


def test_workspace_bytes_is_the_headers_formula(L):
    """Per intermediate ping-pong buffer (min(iterations - 1, 2) of them) an image of rows x
    width x 3 doubles and a noise plane of rows x width doubles: a third more than
    tray_denoise_workspace_bytes. Monotone in width, rows and iterations; errors as for the call."""
    def need(w, rows, it):
        return L.denoise_variance_workspace_bytes(L.denoise_variance_params(w, rows, iterations=it))

    for w, rows in ((1, 1), (37, 23), (1280, 720), (46340, 46340)):
        for it in range(1, 9):
            assert need(w, rows, it) == min(it - 1, 2) * w * rows * 32, (w, rows, it)
            assert 3 * need(w, rows, it) == 4 * L.denoise_workspace_bytes(L.denoise_params(w, rows, iterations=it))
            assert need(w, rows, it) <= need(w + 1, rows, it) and need(w, rows, it) <= need(w, rows + 1, it)
            assert it == 8 or need(w, rows, it) <= need(w, rows, it + 1)
    assert need(0, 5, 5) == 0 and need(5, 0, 5) == 0
    n = ctypes.c_size_t(0)
    lib = L.lib()
    bad = L.denoise_variance_params(4, 4, iterations=0)
    assert lib.tray_denoise_variance_workspace_bytes(ctypes.byref(bad), ctypes.byref(n)) == L.TRAY_ERR_INVALID_ARGUMENT
    bad = L.denoise_variance_params(4, 4, epsilon=0.0)
    assert lib.tray_denoise_variance_workspace_bytes(ctypes.byref(bad), ctypes.byref(n)) == L.TRAY_ERR_INVALID_ARGUMENT
    assert lib.tray_denoise_variance_workspace_bytes(None, ctypes.byref(n)) == L.TRAY_ERR_INVALID_ARGUMENT
    assert lib.tray_denoise_variance_workspace_bytes(ctypes.byref(L.denoise_variance_params(4, 4)), None) == \
        L.TRAY_ERR_INVALID_ARGUMENT
    big = L.denoise_variance_params(2 ** 16, 2 ** 15)
    assert lib.tray_denoise_variance_workspace_bytes(ctypes.byref(big), ctypes.byref(n)) == L.TRAY_ERR_TOO_LARGE


def test_mirror_refuses_without_a_device(L):
    """Tracer.Accumulate and RenderProgressive refuse misshapen input with ValueError before any
    device work; the wrappers raise TrayError for argument errors."""
    import numpy as np

    from tray_amd import ray

    t = ray.New(8, 6)
    assert callable(t.Accumulate) and callable(t.RenderProgressive)
    with pytest.raises(ValueError):
        t.Accumulate(np.zeros((6, 8, 3)))  # one frame, not a stack
    with pytest.raises(ValueError):
        t.Accumulate(np.zeros((2, 6, 7, 3)))
    with pytest.raises(ValueError):
        t.Accumulate(np.zeros((0, 6, 8, 3)))
    with pytest.raises(ValueError):
        t.RenderProgressive(None, 0)
    with pytest.raises(ValueError):
        t.RenderProgressive(None, 4, batch=0)
    with pytest.raises(ValueError):
        t.RenderProgressive(None, 4, sigma_variance=1.0)  # filter parameters without the filter
    with pytest.raises(L.TrayError) as e:
        L.accum_fold_async(L.Accum(FAKE, FAKE, 8, 6, 0, 0), FAKE + 4 * IMAGE, 1)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "overlaps" in str(e.value)
    with pytest.raises(L.TrayError) as e:
        L.denoise_variance_async(FAKE, FAKE + 2 * IMAGE, L.denoise_variance_params(8, 6, iterations=9),
                                 FAKE + 4 * IMAGE, None, 0)
    assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "iterations" in str(e.value)
