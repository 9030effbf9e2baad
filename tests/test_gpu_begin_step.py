"""The begin step of the BVH megakernel (DESIGN.md §5 "The begin step"; lane state
kTravReady in tray_device.hpp): the shade phase and the refill's camera-hit shading
only mark a scattered ray's lane; one step per loop iteration then sets up the new
segments of both (|dir|^2, the out-of-tree spheres, the FP32 traversal state). It
changes when that arithmetic runs, never what it computes, so every frame and every
per-pixel Scene.Hit count must still equal the oracle's: with no scattered ray at all
(depth 1), through each accumulation instance (r = 64, 16, 1), several passes per
launch, scenes with one sphere, with no out-of-tree sphere and with overflowing
candidate lists, the nodes-only and stack-spill instances, and an interleaved row tile."""
import numpy as np
import pytest

from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_parity import WORKERS, bg_struct, camera, check, gpu_render

pytestmark = pytest.mark.gpu

W, H = 40, 24
_oracle = {}


def oracle(O, key, sc, st, w, h, spp, depth, radius, seed, pass_=0, rows=None):
    """The oracle's frame and segment counts, rendered once per case and shared."""
    k = (key, w, h, spp, depth, radius, seed, pass_, None if rows is None else tuple(rows))
    if k not in _oracle:
        if rows is None:
            ref = O.render(sc, DEFAULT_BG, st.as_array(), w, h, spp, depth, radius, seed, workers=WORKERS, pass_=pass_)
        else:
            ref = O.render_rows(sc, DEFAULT_BG, st.as_array(), w, h, spp, depth, radius, seed, list(rows),
                                workers=WORKERS, pass_=pass_)
        for a in ref:
            a.setflags(write=False)
        _oracle[k] = ref
    return _oracle[k]


@pytest.mark.parametrize("spp", [64, 16, 1])
@pytest.mark.parametrize("depth", [1, 2, 50])
def test_begin_step_depths_and_accumulators(L, O, spp, depth):
    """Depth 1: no ray ever scatters, so no lane is ever marked; depth 2: every scattered
    ray ends at its first hit; depth 50: the whole state machine."""
    sc = O.rich_scene(2)
    st = camera(L, RICH_SETUP, W, H)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, spp, depth, 0.5, 4)
    check(rgb, seg, *oracle(O, "rich2", sc, st, W, H, spp, depth, 0.5, 4))


@pytest.mark.parametrize("spp,depth", [(64, 50), (16, 2)])
def test_begin_step_passes_in_one_launch(L, O, spp, depth):
    """Three progressive passes in one persistent launch: each frame equals the single-pass
    render of that pass, which equals the oracle's (colours and Scene.Hit counts)."""
    import torch

    sc = O.rich_scene(2)
    st = camera(L, RICH_SETUP, W, H)
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        out = torch.zeros((3, H, W, 3), dtype=torch.float64, device="cuda")
        p = L.make_params(W, H, depth, spp, 0.5, 4, output=L.OUT_RGB_F64)
        dev.render_passes_async(st, p, 3, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        frames = out.cpu().numpy()
    finally:
        dev.release()
    for k in range(3):
        one, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, spp, depth, 0.5, 4, pass_=k)
        check(one, seg, *oracle(O, "rich2", sc, st, W, H, spp, depth, 0.5, 4, pass_=k))
        assert np.array_equal(frames[k], one), k


def test_begin_step_one_sphere(L, O):
    sc = O.rich_scene(2)
    sc = sc[sc["radius"] == 1.0][:1].copy()  # one of the three big spheres in view
    assert len(sc) == 1
    st = camera(L, RICH_SETUP, W, H)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, 16, 50, 0.5, 6)
    check(rgb, seg, *oracle(O, "one", sc, st, W, H, 16, 50, 0.5, 6))


def test_begin_step_no_out_of_tree_sphere(L, O):
    """Small spheres only (the ground removed): the begin step tests no sphere itself."""
    sc = O.rich_scene(2)
    sc = sc[np.abs(sc["radius"]) < 100.0].copy()
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    info = dev.info()
    dev.release()
    assert info.has_bvh == 1 and info.n_global == 0
    st = camera(L, RICH_SETUP, W, H)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, 16, 50, 0.5, 7)
    check(rgb, seg, *oracle(O, "noground", sc, st, W, H, 16, 50, 0.5, 7))


def test_begin_step_overflowing_candidate_lists(L, O):
    """A dense scene under a wide anti-aliasing disc: some pixels' candidate lists overflow
    and their camera rays traverse the tree (box tests at depth 1 come from nothing else),
    beside lanes whose camera hit was shaded in the refill."""
    import torch

    sc = O.rich_scene(7, 22)
    w, h, spp, radius = 48, 27, 8, 2.0
    st = camera(L, RICH_SETUP, w, h)
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        stats = torch.zeros(3, dtype=torch.int64, device="cuda")
        dev.render_stats_async(st, L.make_params(w, h, 1, spp, radius, 7), out.data_ptr(), stats.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n_seg, _, n_box = stats.tolist()
    finally:
        dev.release()
    assert n_seg == w * h * spp and n_box > 0
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, w, h, spp, 50, radius, 7)
    check(rgb, seg, *oracle(O, "dense7", sc, st, w, h, spp, 50, radius, 7))


@pytest.mark.parametrize("knob", [dict(bvh_lds_mode=2), dict(stack_lds_slots=8), dict(bvh_lds_mode=2, stack_lds_slots=8)])
def test_begin_step_nodes_only_and_stack_spill_instances(L, O, knobs, knob):
    sc = O.rich_scene(2)
    st = camera(L, RICH_SETUP, W, H)
    knobs(**knob)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, 16, 50, 0.5, 4)
    check(rgb, seg, *oracle(O, "rich2", sc, st, W, H, 16, 50, 0.5, 4))


def test_begin_step_interleaved_row_tile(L, O):
    from tray_amd import shard

    sc = O.rich_scene(2)
    w, h = 96, 54
    st = camera(L, RICH_SETUP, w, h)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, w, h, 64, 50, 0.5, 9, tile_rows=1, tile_count=8, tile_index=3)
    rows = [int(y) for y in shard.rows_for(h, 1, 8, 3)]
    assert len(rows) == rgb.shape[0]
    check(rgb, seg, *oracle(O, "rich2", sc, st, w, h, 64, 50, 0.5, 9, rows=rows))
