"""The megakernel's per-chunk pixel decode (tray_kernel.hip, `kChunkPixel`). With
on-chip sums and 64 | r a 64-item chunk is 64 samples of one pixel in one pass, so the wave that
takes a chunk decodes its pixel once and the refill's lanes copy it, where every lane used to
decode its own item. The change moves integer arithmetic and no decision, so every frame of a
passes launch must equal the single-pass render of the same pass bit for bit, and that render the
oracle's pixels: Scene.Hit counts exactly, colours within the suite's 1e-12 bar.

Tiny frames whose width and height are no multiples of 8 (padding chunks in both directions), a
small scene, depth 8; r = 64, 128, 192 with 1, 3 and 16 passes per launch, a first pass other
than 0, row tiles, the work order on and off, several launch bands, the stats and live-progress
entry points, and r = 1, 16, 32, 48, whose instances keep the per-lane decode.
tests/test_chunk_decode_cpu.py shows the index identity itself."""
import numpy as np
import pytest

from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_begin_step import oracle
from test_gpu_parity import bg_struct, camera, check, gpu_render

pytestmark = pytest.mark.gpu

DEPTH, RADIUS, SEED = 8, 0.5, 6
SIZES = [(24, 20), (20, 13)]
_scene = {}
_single = {}


def scene(O):
    """RichScene with half extent 2: 16 spheres or more, so the device builds its tree."""
    if "s" not in _scene:
        sc = O.rich_scene(2, 2)
        sc.setflags(write=False)
        _scene["s"] = sc
    return _scene["s"]


def single(L, O, w, h, spp, pass_=0, **tiles):
    """One single-pass render (frame, Scene.Hit counts) per case, checked against the oracle once."""
    key = (w, h, spp, pass_, tuple(sorted(tiles.items())))
    if key not in _single:
        from tray_amd import shard

        sc = scene(O)
        st = camera(L, RICH_SETUP, w, h)
        rgb, seg = gpu_render(L, sc, DEFAULT_BG, st, w, h, spp, DEPTH, RADIUS, SEED, pass_=pass_, **tiles)
        rows = None
        if tiles:
            rows = [int(y) for y in shard.rows_for(h, tiles["tile_rows"], tiles["tile_count"], tiles["tile_index"])]
        check(rgb, seg, *oracle(O, "rich2x2", sc, st, w, h, spp, DEPTH, RADIUS, SEED, pass_=pass_, rows=rows))
        rgb.setflags(write=False)
        seg.setflags(write=False)
        _single[key] = (rgb, seg)
    return _single[key]


def passes_launch(L, dev, st, p, n):
    """Frames of one launch of n passes (FP64), through render_async for n = 1."""
    import torch

    out = torch.zeros((n, L.params_rows(p), p.width, 3), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if n == 1:
        dev.render_async(st, p, out.data_ptr(), None, s)
    else:
        dev.render_passes_async(st, p, n, out.data_ptr(), s)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def launch_equals_singles(L, O, w, h, spp, n, pass0=0, launches=1, on_chip=True, **tiles):
    """`launches` launches of n passes from pass0 on one scene handle (the second launch of a key
    runs in the counted work order): every frame equals its single-pass render."""
    sc = scene(O)
    st = camera(L, RICH_SETUP, w, h)
    want = [single(L, O, w, h, spp, pass0 + k, **tiles)[0] for k in range(n)]  # before any knob applies
    p = L.make_params(w, h, DEPTH, spp, RADIUS, SEED, output=L.OUT_RGB_F64, pass_=pass0, **tiles)
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        plan = dev.plan(st, p, n).as_dict()
        assert plan["bvh"] == 1
        assert (plan["acc_slots"] > 0) == on_chip, plan
        for launch in range(launches):
            frames = passes_launch(L, dev, st, p, n)
            for k in range(n):
                assert np.array_equal(frames[k], want[k]), (launch, k)
    finally:
        dev.release()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("passes", [1, 3, 16])
@pytest.mark.parametrize("spp", [64, 128, 192])
def test_chunk_decode_passes_and_rays_per_pixel(L, O, spp, passes, w, h):
    launch_equals_singles(L, O, w, h, spp, passes)


@pytest.mark.parametrize("w,h", SIZES)
def test_chunk_decode_first_pass_7(L, O, w, h):
    launch_equals_singles(L, O, w, h, 64, 3, pass0=7)
    assert not np.array_equal(single(L, O, w, h, 64, 7)[0], single(L, O, w, h, 64, 0)[0])


@pytest.mark.parametrize("rank", [0, 1, 2])
@pytest.mark.parametrize("tile_rows", [1, 3])
def test_chunk_decode_row_tiles(L, O, tile_rows, rank):
    from tray_amd import shard

    for (w, h), spp in zip(SIZES, (64, 128)):
        p = shard.shard_params(L.make_params(w, h, DEPTH, spp, RADIUS, SEED), tile_rows, 3, rank)
        tiles = dict(tile_rows=p.tile_rows, tile_count=p.tile_count, tile_index=p.tile_index)
        assert tiles == dict(tile_rows=tile_rows, tile_count=3, tile_index=rank)
        assert single(L, O, w, h, spp, **tiles)[0].shape[0] == len(shard.rows_for(h, tile_rows, 3, rank))
        launch_equals_singles(L, O, w, h, spp, 3, pass0=1, **tiles)


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("passes", [1, 3])
def test_chunk_decode_work_order_on_and_off(L, O, knobs, passes, order):
    """The first launch of a key counts each tile's Scene.Hit calls, the second hands the tiles out
    most expensive first (a permuted tile order); with the knob off both run in band order."""
    w, h = SIZES[0]
    if not order:
        knobs(work_order=0)
    launch_equals_singles(L, O, w, h, 64, passes, launches=3)


@pytest.mark.parametrize("w,h", SIZES)
def test_chunk_decode_several_bands(L, O, knobs, w, h):
    """One 8-row tile row per launch band: 3 bands of 24 x 20, 2 of 20 x 13 (j0 = 0, 8, 16; the
    last band's rows are padded)."""
    for spp, passes in ((64, 1), (128, 3)):
        for k in range(passes):  # the references, in one band
            single(L, O, w, h, spp, k)
        knobs(band_samples=((w + 7) // 8) * 64 * spp * passes)
        launch_equals_singles(L, O, w, h, spp, passes, launches=2)
        L.clear_debug_knobs()


def test_chunk_decode_stats_entry_point(L, O):
    """tray_render_stats_async: the frame (FP32) and the Scene.Hit total of the plain render."""
    import torch

    w, h, spp = SIZES[1] + (64,)
    sc = scene(O)
    st = camera(L, RICH_SETUP, w, h)
    _, seg = single(L, O, w, h, spp)
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        stats = torch.zeros(3, dtype=torch.int64, device="cuda")
        p = L.make_params(w, h, DEPTH, spp, RADIUS, SEED)
        dev.render_stats_async(st, p, out.data_ptr(), stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n_seg, n_sphere, n_box = stats.tolist()
    finally:
        dev.release()
    assert n_seg == int(seg.sum(dtype=np.int64))
    assert n_sphere > 0
    f32, _ = L.render(sc, bg_struct(L, DEFAULT_BG), st,
                      L.make_params(w, h, DEPTH, spp, RADIUS, SEED, output=L.OUT_RGB_F32), 0)
    assert np.array_equal(out.cpu().numpy(), f32)


def test_chunk_decode_live_progress_entry_point(L, O):
    """tray_render_progress: the same bits, every row reported, every sample counted."""
    w, h, spp = SIZES[0] + (128,)
    rgb, seg = single(L, O, w, h, spp)
    rows = []
    p = L.make_params(w, h, DEPTH, spp, RADIUS, SEED)
    live, live_seg = L.render(scene(O), bg_struct(L, DEFAULT_BG), camera(L, RICH_SETUP, w, h), p, 0, segments=True,
                              progress=rows.append)
    assert sum(rows) == h, rows
    counts = L.progress_counts(0)
    assert counts.tolist() == [min(8, h - 8 * t) * w * spp for t in range((h + 7) // 8)]
    assert np.array_equal(live, rgb) and np.array_equal(live_seg, seg)


@pytest.mark.parametrize("spp", [1, 16, 32, 48])
def test_chunk_decode_untouched_paths(L, O, spp):
    """r = 16, 32: on-chip sums with several pixel-passes per chunk; r = 1, 48: FP64 sums in
    sample order. All keep the per-lane decode."""
    w, h = SIZES[spp % 3 == 0]
    launch_equals_singles(L, O, w, h, spp, 3, on_chip=spp in (16, 32))
