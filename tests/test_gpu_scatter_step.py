"""The scatter step of the BVH megakernel (DESIGN.md §5 "The scatter step"; lane states
kTravHit / kTravHitCam in tray_device.hpp): the shade phase and the refill's camera-hit
shading run only the end half of a shading (sky, last level) and mark every other hit;
one step per loop iteration then scatters the marked lanes of both and sets up their new
segments. It changes when that arithmetic runs, never what it computes, so every frame
must equal the oracle's to the suite's bar and every per-pixel Scene.Hit count exactly:
with no marked lane at all (depth 1), with marked lanes that all end at their next
shading (depth 2), through each accumulation instance (r = 64, 16, 1), with paths that
end inside the step (rays absorbed by fuzzed Metal, also through the live-progress
instance), with one material class only, several passes per launch, the nodes-only and
stack-spill instances, an interleaved row tile, no out-of-tree sphere, overflowing
candidate lists, and the stats instance's segment total."""
import numpy as np
import pytest

from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_begin_step import oracle
from test_gpu_fuzz import random_scene, random_setup
from test_gpu_parity import WORKERS, bg_struct, camera, check, gpu_render

pytestmark = pytest.mark.gpu

W, H = 40, 24


@pytest.mark.parametrize("spp", [64, 16, 1])
@pytest.mark.parametrize("depth", [1, 2, 50])
def test_scatter_step_depths_and_accumulators(L, O, spp, depth):
    """Depth 1: no lane is ever marked and every camera hit ends in the refill's end half;
    depth 2: every marked lane's ray ends at its next shading; depth 50: the whole state
    machine. r = 64, 16, 1: the three accumulation instances."""
    sc = O.rich_scene(2)
    st = camera(L, RICH_SETUP, W, H)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, spp, depth, 0.5, 4)
    check(rgb, seg, *oracle(O, "rich2", sc, st, W, H, spp, depth, 0.5, 4))


def fuzz_case(O, k):
    """Scene and camera of tests/test_gpu_fuzz.py's case k."""
    rng = np.random.default_rng(1000 + k)
    sc = random_scene(O, rng, [1, 3, 24, 160, 600][k % 5], ground=k % 3 != 2)
    return sc, random_setup(rng, sc, inside=k % 4 == 3)


@pytest.mark.parametrize("k", [19, 3])  # 600 spheres seen from outside; 160 seen from inside one
def test_scatter_step_absorbed_rays(L, O, k):
    """Metal spheres with fuzz above 1 absorb rays (dot(scattered, normal) <= 0): those
    paths end inside the scatter step. Frames and counts against the oracle; the same
    render through tray_render_progress gives the same bits, and the device's progress
    counters, read back after the launch (tray_debug_progress_counts: the callback's rows
    would add up to the height whatever the kernel counted, since the host reports the
    rest when the launch ends), hold every sample of their tile row, the absorbed ones
    included: rows x width x r each, height x width x r together."""
    sc, setup = fuzz_case(O, k)
    assert ((sc["material"] == O.METAL) & (sc["param"] > 1.0)).any()
    depth, spp, seed = 50, 16, 5
    st = camera(L, setup, W, H)
    # The case exercises the step only if a path ends by absorption at bounce >= 1. At one
    # sample per pixel the oracle shows it: a black pixel whose path made at least two
    # Scene.Hit calls and fewer than the depth allows neither reached the sky (its colour
    # would be the background times albedos of 0.05 at least) nor ran out of depth.
    one, one_seg = oracle(O, ("fuzz", k), sc, st, W, H, 1, depth, 0.5, seed)
    absorbed = (one_seg >= 2) & (one_seg < depth) & (one == 0.0).all(-1)
    assert absorbed.sum() >= 1
    ref = oracle(O, ("fuzz", k), sc, st, W, H, spp, depth, 0.5, seed)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, spp, depth, 0.5, seed)
    check(rgb, seg, *ref)
    rgb1, seg1 = gpu_render(L, sc, DEFAULT_BG, st, W, H, 1, depth, 0.5, seed)
    check(rgb1, seg1, one, one_seg)
    rows = []
    p = L.make_params(W, H, depth, spp, 0.5, seed)
    live, live_seg = L.render(sc, bg_struct(L, DEFAULT_BG), st, p, 0, segments=True, progress=rows.append)
    assert sum(rows) == H, rows
    counts = L.progress_counts(0)
    want = [min(8, H - 8 * t) * W * spp for t in range((H + 7) // 8)]
    assert counts.tolist() == want, (counts.tolist(), want)
    assert int(counts.sum()) == H * W * spp
    assert np.array_equal(live, rgb) and np.array_equal(live_seg, seg)


@pytest.mark.parametrize("material,param", [("DIELECTRIC", 1.5), ("LAMBERTIAN", 0.0)])
@pytest.mark.parametrize("spp", [64, 4])
def test_scatter_step_one_material_class(L, O, material, param, spp):
    """Every sphere Dielectric, or every sphere Lambertian: a merged pass holds one class
    from both of its sources, and the lazy Unit(dir) is always taken or always skipped."""
    sc = O.rich_scene(2).copy()
    sc["material"] = getattr(O, material)
    sc["param"] = param
    st = camera(L, RICH_SETUP, W, H)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, spp, 50, 0.5, 8)
    check(rgb, seg, *oracle(O, material, sc, st, W, H, spp, 50, 0.5, 8))


def test_scatter_step_passes_in_one_launch(L, O):
    """Three progressive passes in one persistent launch equal three single-pass renders,
    which equal the oracle's."""
    import torch

    sc = O.rich_scene(2)
    st = camera(L, RICH_SETUP, W, H)
    spp, depth = 64, 50
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


def test_scatter_step_interleaved_row_tile(L, O):
    from tray_amd import shard

    sc = O.rich_scene(2)
    w, h = 40, 24
    st = camera(L, RICH_SETUP, w, h)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, w, h, 64, 50, 0.5, 9, tile_rows=1, tile_count=4, tile_index=3)
    rows = [int(y) for y in shard.rows_for(h, 1, 4, 3)]
    assert len(rows) == rgb.shape[0] == 6
    check(rgb, seg, *oracle(O, "rich2", sc, st, w, h, 64, 50, 0.5, 9, rows=rows))


@pytest.mark.parametrize("knob", [dict(bvh_lds_mode=2), dict(stack_lds_slots=8), dict(bvh_lds_mode=2, stack_lds_slots=8)])
def test_scatter_step_nodes_only_and_stack_spill_instances(L, O, knobs, knob):
    sc = O.rich_scene(2)
    st = camera(L, RICH_SETUP, W, H)
    knobs(**knob)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, 16, 50, 0.5, 4)
    check(rgb, seg, *oracle(O, "rich2", sc, st, W, H, 16, 50, 0.5, 4))


def test_scatter_step_no_out_of_tree_sphere(L, O):
    """Small spheres only (the ground removed): the step's begin part tests no sphere itself."""
    sc = O.rich_scene(2)
    sc = sc[np.abs(sc["radius"]) < 100.0].copy()
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    info = dev.info()
    dev.release()
    assert info.has_bvh == 1 and info.n_global == 0
    st = camera(L, RICH_SETUP, W, H)
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, W, H, 16, 50, 0.5, 7)
    check(rgb, seg, *oracle(O, "noground", sc, st, W, H, 16, 50, 0.5, 7))


def _stats(L, sc, st, w, h, spp, depth, radius, seed):
    """(segments, sphere tests, box tests) of one frame through tray_render_stats_async."""
    import torch

    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        stats = torch.zeros(3, dtype=torch.int64, device="cuda")
        dev.render_stats_async(st, L.make_params(w, h, depth, spp, radius, seed), out.data_ptr(), stats.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return stats.tolist()
    finally:
        dev.release()


def test_scatter_step_overflowing_candidate_lists(L, O):
    """A dense scene under a wide anti-aliasing disc: some pixels' candidate lists overflow
    and their camera rays traverse the tree (box tests at depth 1 come from nothing else),
    so their hits are marked by the shade phase, beside lanes marked by the refill."""
    sc = O.rich_scene(7, 22)
    w, h, spp, radius = 40, 24, 8, 2.0
    st = camera(L, RICH_SETUP, w, h)
    n_seg, _, n_box = _stats(L, sc, st, w, h, spp, 1, radius, 7)
    assert n_seg == w * h * spp and n_box > 0
    rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, w, h, spp, 50, radius, 7)
    check(rgb, seg, *oracle(O, "dense7", sc, st, w, h, spp, 50, radius, 7))


@pytest.mark.parametrize("spp", [64, 16])
def test_scatter_step_stats_instance_segment_total(L, O, spp):
    sc = O.rich_scene(2)
    st = camera(L, RICH_SETUP, W, H)
    _, ref_seg = oracle(O, "rich2", sc, st, W, H, spp, 50, 0.5, 4)
    assert _stats(L, sc, st, W, H, spp, 50, 0.5, 4)[0] == int(ref_seg.sum(dtype=np.int64))
