"""include/tray_scene_update.h on the CPU: the two entry points and the node hook of tray_debug.h
are declared, exported and bound, sit beside (not inside) the older headers, the header is C99 and
links from C, the record is 32 bytes, and the null-argument errors are reported before any device
work. No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "tray_scene_update.h")
CALLER = os.path.join(ROOT, "tests", "c", "tray_scene_update_caller.c")
OLDER = {"tray.h": "EXPORTS", "tray_query.h": "QUERY_EXPORTS", "tray_shade.h": "SHADE_EXPORTS",
         "tray_aov.h": "AOV_EXPORTS", "tray_denoise.h": "DENOISE_EXPORTS", "tray_progressive.h": "PROGRESSIVE_EXPORTS",
         "tray_adaptive.h": "ADAPTIVE_EXPORTS", "tray_temporal.h": "TEMPORAL_EXPORTS",
         "tray_temporal_variance.h": "TEMPORAL_VARIANCE_EXPORTS"}
FAKE = 0x100000  # a non-null "pointer": validation fails before anything reads it


def _declared(path=HEADER):
    return set(re.findall(r"^(?:int|int32_t|const char \*)\s*\**\s*(tray_\w+)\(", open(path).read(), re.M))


def test_exports_match_header(L):
    declared = _declared()
    assert declared == set(L.SCENE_UPDATE_EXPORTS) and len(declared) == len(L.SCENE_UPDATE_EXPORTS) == 2
    lib = L.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in L.SCENE_UPDATE_EXPORTS + ("tray_debug_scene_nodes",):
        assert hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", out), name
    assert "tray_debug_scene_nodes" in L.DEBUG_EXPORTS
    assert "tray_debug_scene_nodes" in _declared(os.path.join(INCLUDE, "tray_debug.h"))
    assert lib.tray_abi_version() == 6  # the addition bumps nothing


def test_older_headers_and_lists_unchanged(L):
    for header, listname in OLDER.items():
        text = open(os.path.join(INCLUDE, header)).read()
        assert "tray_scene_update" not in text, header
        assert _declared(os.path.join(INCLUDE, header)) == set(getattr(L, listname)), header
        assert not set(L.SCENE_UPDATE_EXPORTS) & set(getattr(L, listname)), header
    assert not set(L.SCENE_UPDATE_EXPORTS) & set(L.DEBUG_EXPORTS)


def test_record_layout(L):
    text = open(HEADER).read()
    body = text[text.index("typedef struct tray_scene_update_record {"):text.index("} tray_scene_update_record;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.split()[-1] for d in body[body.index("{") + 1:].split(";") if d.strip()]
    R = L.SceneUpdateRecord
    assert fields == [n for n, _ in R._fields_] == list(L.SCENE_UPDATE_RECORD_DTYPE.names)
    assert ctypes.sizeof(R) == L.SCENE_UPDATE_RECORD_DTYPE.itemsize == 32
    assert (R.applied.offset, R.n_refused.offset, R.first_refused.offset, R.reserved.offset, R.extent.offset,
            R.bound.offset) == (0, 4, 8, 12, 16, 24)
    assert [L.SCENE_UPDATE_RECORD_DTYPE.fields[n][1] for n in L.SCENE_UPDATE_RECORD_DTYPE.names] == [0, 4, 8, 12, 16, 24]
    N = L.NODE_DTYPE
    assert N.itemsize == 128 and N["box"].shape == (3, 2, 4) and N["box"].base == np.dtype("<f4")
    assert (N.fields["box"][1], N.fields["ref"][1], N.fields["pad"][1]) == (0, 96, 112)


def test_header_is_c99_and_links(tmp_path):
    from tray_amd import _lib

    text = open(CALLER).read()
    for name in _lib.SCENE_UPDATE_EXPORTS:
        assert name + "(" in text, name
    exe = str(tmp_path / "tray_scene_update_caller")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, CALLER, "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    # tray_debug.h too: it now includes tray.h for tray_scene_t
    src = tmp_path / "debug_header.c"
    src.write_text('#include "tray_debug.h"\nint main(void) { return tray_debug_scene_nodes(NULL, NULL, 0, NULL) == '
                   'TRAY_ERR_INVALID_ARGUMENT ? 0 : 1; }\n')
    exe = str(tmp_path / "debug_header")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, str(src), "-L",
                        os.path.join(ROOT, "tray_amd"), "-ltray_amd", "-Wl,-rpath," + os.path.join(ROOT, "tray_amd"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe], timeout=120).returncode == 0


def test_null_arguments_before_any_device_work(L):
    lib = L.lib()
    rec = L.SceneUpdateRecord()
    cases = {"scene": (None, FAKE, ctypes.byref(rec)), "geometry": (FAKE, None, ctypes.byref(rec)),
             "record": (FAKE, FAKE, None)}
    for what, (scene, geometry, record) in cases.items():
        assert lib.tray_scene_update(scene, geometry, 3, record) == L.TRAY_ERR_INVALID_ARGUMENT, what
        assert f"null {what}".encode() in lib.tray_last_error(), what
        record_device = FAKE if record is not None else None
        assert lib.tray_scene_update_async(scene, geometry, 3, record_device, None) == L.TRAY_ERR_INVALID_ARGUMENT, what
        assert f"null {what}".encode() in lib.tray_last_error(), what
    size = ctypes.c_size_t(7)
    assert lib.tray_debug_scene_nodes(None, None, 0, ctypes.byref(size)) == L.TRAY_ERR_INVALID_ARGUMENT
    assert lib.tray_debug_scene_nodes(FAKE, None, 0, None) == L.TRAY_ERR_INVALID_ARGUMENT


def test_python_surface_checks_shapes():
    """Scene.Move and Tracer.RenderAnimation refuse a wrong shape before any device work."""
    import pytest

    from tray_amd import ray

    scene = ray.DefaultScene()
    n = len(scene.Objects)
    with pytest.raises(ValueError):
        scene.Move(np.zeros((n + 1, 3)))
    with pytest.raises(ValueError):
        scene.Move(np.zeros((n, 3)), radii=np.zeros(n + 1))
    centers = np.array([o.Center for o in scene.Objects]) + 1.0
    assert scene.Move(centers) is False  # no uploaded copy: nothing to move in place
    assert [o.Center for o in scene.Objects] == [tuple(c) for c in centers.tolist()]
    t = ray.New(8, 4)
    t.Camera = ray.RichSceneCamera()
    for bad in (np.zeros((0, n, 4)), np.zeros((2, n + 1, 4)), np.zeros((n, 4))):
        with pytest.raises(ValueError):
            t.RenderAnimation(scene, bad)
    g = ray.Bounce(ray.RichScene(2), 3)
    assert g.shape == (3, 486, 4) and (g[0, :, 3] == g[2, :, 3]).all() and (g[0, :, 1] != g[2, :, 1]).any()
    small = g[0, :, 3] < 0.5
    assert small.sum() > 400 and (g[:, small, 1] >= g[:, small, 3]).all()  # they hop on or above the ground
    assert (g[:, ~small] == g[0, ~small]).all()
