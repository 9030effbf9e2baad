"""The megakernel's plain-frame instance (tray_kernel.hip `plain_frame_launch`, `PlainFrame` in
tray_device.hpp): render_kernel with the launch's options compiled in. It removes
tests whose answers are fixed for a whole launch and the arms behind them, never a decision a path
takes, so its frames must equal the generic instance's bit for bit (the "plain_instance" knob forces
the generic one in the same process), and pass 0 the oracle's pixels within the suite's bar.

The scene is the book cover at half extent 3: one out-of-tree sphere (the ground), one sphere per
leaf, a tree of more than one level. The frame is 20 x 12 (column and row padding chunks), r = 64,
depth 8, with 1 and 3 passes per launch, launched twice with one key: the first launch of a key
counts the tiles' costs (generic), the second carries the work order (plain). Every launch that must
not take the plain instance is checked to take none and to render the forced-generic bits."""
import numpy as np
import pytest

from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_begin_step import oracle
from test_gpu_parity import TIGHT, bg_struct, camera

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, RADIUS, SEED = 20, 12, 64, 8, 0.5, 5
_scene = {}


def scene(O):
    if "s" not in _scene:
        sc = O.rich_scene(2, 3)
        sc.setflags(write=False)
        _scene["s"] = sc
    return _scene["s"]


def two_launches(L, sc, p, n, segments=False, w=W, h=H):
    """Two launches of n passes with one key on a fresh scene handle: their frames (and Scene.Hit
    counts when asked for) and how many launches each sent through the plain instance."""
    import torch

    st = camera(L, RICH_SETUP, w, h)
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    frames, segs, took = [], [], []
    try:
        for _ in range(2):
            out = torch.zeros((n, L.params_rows(p), w, 3), dtype=torch.float64, device="cuda")
            seg = torch.zeros((L.params_rows(p), w), dtype=torch.int32, device="cuda") if segments else None
            s = torch.cuda.current_stream().cuda_stream
            before = L.plain_launches()
            if n == 1:
                dev.render_async(st, p, out.data_ptr(), seg.data_ptr() if segments else None, s)
            else:
                dev.render_passes_async(st, p, n, out.data_ptr(), s)
            torch.cuda.synchronize()
            took.append(L.plain_launches() - before)
            frames.append(out.cpu().numpy())
            segs.append(seg.cpu().numpy() if segments else None)
    finally:
        dev.release()
    return frames, segs, took


def forced_generic(L, knobs, sc, p, n, segments=False, w=W, h=H, **kw):
    knobs(plain_instance=0, **kw)
    try:
        frames, segs, took = two_launches(L, sc, p, n, segments, w, h)
    finally:
        L.clear_debug_knobs()
    assert took == [0, 0]
    return frames, segs


def test_scene_qualifies(L, O):
    dev = L.DeviceScene(scene(O), bg_struct(L, DEFAULT_BG), 0)
    try:
        info = dev.info()
        p = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64)
        plan = dev.plan(camera(L, RICH_SETUP, W, H), p).as_dict()
    finally:
        dev.release()
    assert info.has_bvh == 1 and info.n_global == 1 and info.leaf_max == 1
    assert info.n_nodes > 1 and info.n_leaves > 4  # a 4-wide tree of more than one level
    assert plan["bvh"] == 1 and plan["acc_slots"] > 0 and plan["lds_layout"] == 1


@pytest.mark.parametrize("passes", [1, 3])
def test_plain_equals_generic_and_oracle(L, O, knobs, passes):
    sc = scene(O)
    p = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64)
    generic, _ = forced_generic(L, knobs, sc, p, passes)
    frames, _, took = two_launches(L, sc, p, passes)
    assert took == [0, 1]  # the counting launch, then the launch with its work order (one band)
    for f in (generic[1], frames[0], frames[1]):
        assert np.array_equal(f, generic[0])
    ref, _ = oracle(O, "plain3", sc, camera(L, RICH_SETUP, W, H), W, H, SPP, DEPTH, RADIUS, SEED)
    err = float(np.max(np.abs(frames[1][0] - ref)))
    assert err <= TIGHT, err


def test_plain_second_layout_and_deep_instance(L, O, knobs):
    """The nodes-only layout and the 6-step twin, forced by their knobs: plain again, same bits."""
    sc = scene(O)
    p = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64)
    generic, _ = forced_generic(L, knobs, sc, p, 1)
    for kw in (dict(bvh_lds_mode=2), dict(node_deep=1), dict(bvh_lds_mode=2, node_deep=1)):
        knobs(**kw)
        try:
            frames, _, took = two_launches(L, sc, p, 1)
        finally:
            L.clear_debug_knobs()
        assert took == [0, 1], kw
        assert np.array_equal(frames[0], generic[0]) and np.array_equal(frames[1], generic[0]), kw


def falls_back(L, knobs, sc, p, n=1, segments=False, w=W, h=H, **kw):
    """No launch takes the plain instance, and the bits are the forced-generic render's."""
    generic, gseg = forced_generic(L, knobs, sc, p, n, segments, w, h, **kw)
    if kw:
        knobs(**kw)
    try:
        frames, segs, took = two_launches(L, sc, p, n, segments, w, h)
    finally:
        L.clear_debug_knobs()
    assert took == [0, 0]
    for k in range(2):
        assert np.array_equal(frames[k], generic[0])
        if segments:
            assert np.array_equal(segs[k], gseg[0]) and int(segs[k].sum()) > 0
    return frames[1]


def test_fallback_segment_counts(L, O, knobs):
    p = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64)
    falls_back(L, knobs, scene(O), p, segments=True)


def test_fallback_row_tiles(L, O, knobs):
    for index in (0, 1):
        p = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64, tile_rows=1, tile_count=2,
                          tile_index=index)
        assert L.params_rows(p) == H // 2
        falls_back(L, knobs, scene(O), p, 3)


@pytest.mark.parametrize("spp", [16, 1])
def test_fallback_rays_per_pixel(L, O, knobs, spp):
    """r = 16: sums per pixel-pass of a chunk; r = 1: no on-chip sums, no anti-aliasing disc."""
    p = L.make_params(W, H, DEPTH, spp, RADIUS, SEED, output=L.OUT_RGB_F64)
    falls_back(L, knobs, scene(O), p, 3)


def test_fallback_linear_scan(L, O, knobs):
    p = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64, flags=L.FLAG_LINEAR_SCAN)
    lin = falls_back(L, knobs, scene(O), p)
    q = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64)
    assert np.array_equal(lin, two_launches(L, scene(O), q, 1)[0][1])  # the plain instance's bits


def test_fallback_no_out_of_tree_sphere(L, O, knobs):
    sc = scene(O)
    sc = sc[np.abs(sc["radius"]) < 100.0].copy()  # the ground removed
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    info = dev.info()
    dev.release()
    assert info.has_bvh == 1 and info.n_global == 0
    p = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64)
    falls_back(L, knobs, sc, p, 3)


def test_fallback_leaves_of_several_spheres(L, O, knobs):
    knobs(bvh_leaf=2)
    dev = L.DeviceScene(scene(O), bg_struct(L, DEFAULT_BG), 0)
    info = dev.info()
    dev.release()
    L.clear_debug_knobs()
    assert info.has_bvh == 1 and info.leaf_max == 2 and info.n_global == 1
    p = L.make_params(W, H, DEPTH, SPP, RADIUS, SEED, output=L.OUT_RGB_F64)
    two = falls_back(L, knobs, scene(O), p, 3, bvh_leaf=2)
    assert np.array_equal(two, two_launches(L, scene(O), p, 3)[0][1])  # one sphere per leaf, plain: the same bits
