"""The front of the megakernel's refill (tray_kernel.hip): the straight-line item
assignment (the current chunk's rest, one take at most, the next chunk's first items) and, with
on-chip sums and 64 | r, the decode kept for a pixel's run of chunks. Both move integer work and
no decision: which lane gets which item in which refill is what it was, so every frame of a passes
launch must equal the single-pass render of the same pass bit for bit, and that render the oracle's
pixels (Scene.Hit counts exactly, colours within the suite's 1e-12 bar; checked once per case by
test_gpu_chunk_decode.single, whose frames this file shares).

The shapes, beside those of tests/test_gpu_chunk_decode.py: the wave's reservation forced to 1, 3,
8 and 64 chunks (takes inside a reservation, across its end - 3 and 8 divide no run of 16 or 48
chunks evenly - and, with single chunks, a wave's takes scattered over the pixels' runs); 1 and 2
accumulator slots per wave (the retire inside the take, and refills where no slot frees, so only
the lanes of the current chunk's rest start); and r = 1, 16, 32, 48, which keep their decode at
every take. tests/test_refill_assign_cpu.py shows the two identities themselves."""
import numpy as np
import pytest

from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_chunk_decode import DEPTH, RADIUS, SEED, SIZES, launch_equals_singles, scene, single
from test_gpu_parity import bg_struct, camera

pytestmark = pytest.mark.gpu


def knobbed(L, O, knobs, w, h, spp, n, pass0=0, launches=1, on_chip=True, tiles=None, **kw):
    """launch_equals_singles under the debug knobs `kw`; the references render before they apply."""
    tiles = tiles or {}
    for k in range(n):
        single(L, O, w, h, spp, pass0 + k, **tiles)
    knobs(**kw)
    try:
        launch_equals_singles(L, O, w, h, spp, n, pass0=pass0, launches=launches, on_chip=on_chip, **tiles)
    finally:
        L.clear_debug_knobs()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("passes", [1, 3, 16])
@pytest.mark.parametrize("spp", [64, 128, 192])
def test_refill_assign_passes_and_rays_per_pixel(L, O, spp, passes, w, h):
    launch_equals_singles(L, O, w, h, spp, passes)


@pytest.mark.parametrize("w,h", SIZES)
def test_refill_assign_first_pass_7(L, O, w, h):
    launch_equals_singles(L, O, w, h, 128, 3, pass0=7)
    assert not np.array_equal(single(L, O, w, h, 128, 7)[0], single(L, O, w, h, 128, 0)[0])


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("spp,passes", [(64, 1), (64, 16), (128, 3), (192, 16)])
@pytest.mark.parametrize("wave_chunks", [1, 3, 8, 64])
def test_refill_assign_reservation_sizes(L, O, knobs, wave_chunks, spp, passes, w, h):
    """Runs of 1, 16, 6 and 48 chunks against reservations of 1, 3, 8 and 64."""
    knobbed(L, O, knobs, w, h, spp, passes, wave_chunks=wave_chunks)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("spp,passes,wave_chunks", [(64, 3, 0), (128, 16, 0), (64, 16, 1), (192, 1, 3)])
@pytest.mark.parametrize("slots", [1, 2])
def test_refill_assign_few_accumulator_slots(L, O, knobs, slots, spp, passes, wave_chunks, w, h):
    """One slot: a refill that uses the current chunk up finds no free slot (its own lanes hold it),
    so only those lanes start. Two: the take's retire frees the chunk before."""
    kw = dict(acc_slots=slots)
    if wave_chunks:
        kw["wave_chunks"] = wave_chunks
    knobbed(L, O, knobs, w, h, spp, passes, **kw)
    knobs(**kw)
    dev = L.DeviceScene(scene(O), bg_struct(L, DEFAULT_BG), 0)
    try:
        p = L.make_params(w, h, DEPTH, spp, RADIUS, SEED, output=L.OUT_RGB_F64)
        assert dev.plan(camera(L, RICH_SETUP, w, h), p, passes).as_dict()["acc_slots"] == slots
    finally:
        dev.release()


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("spp,passes,wave_chunks", [(64, 1, 0), (64, 3, 0), (128, 3, 1), (64, 16, 3)])
def test_refill_assign_work_order_on_and_off(L, O, knobs, spp, passes, wave_chunks, order):
    """Three launches of one key: the second and third hand the tiles out in the counted order, in
    which a pixel's run still is passes x r / 64 consecutive chunks."""
    w, h = SIZES[0]
    kw = {} if order else dict(work_order=0)
    if wave_chunks:
        kw["wave_chunks"] = wave_chunks
    knobbed(L, O, knobs, w, h, spp, passes, launches=3, **kw)


@pytest.mark.parametrize("w,h", SIZES)
def test_refill_assign_several_bands(L, O, knobs, w, h):
    """One 8-row tile row per launch band; each band's kernel starts with no run kept."""
    for spp, passes in ((64, 1), (128, 3), (64, 16)):
        knobbed(L, O, knobs, w, h, spp, passes, launches=2, band_samples=((w + 7) // 8) * 64 * spp * passes)


@pytest.mark.parametrize("rank", [0, 1, 2])
@pytest.mark.parametrize("tile_rows", [1, 3])
def test_refill_assign_row_tiles(L, O, knobs, tile_rows, rank):
    from tray_amd import shard

    for (w, h), spp in zip(SIZES, (64, 128)):
        p = shard.shard_params(L.make_params(w, h, DEPTH, spp, RADIUS, SEED), tile_rows, 3, rank)
        tiles = dict(tile_rows=p.tile_rows, tile_count=p.tile_count, tile_index=p.tile_index)
        assert tiles == dict(tile_rows=tile_rows, tile_count=3, tile_index=rank)
        knobbed(L, O, knobs, w, h, spp, 3, pass0=1, tiles=tiles, wave_chunks=3)


def test_refill_assign_stats_entry_point(L, O):
    """tray_render_stats_async: the frame (FP32) and the Scene.Hit total of the plain render."""
    import torch

    w, h, spp = SIZES[0] + (128,)
    st = camera(L, RICH_SETUP, w, h)
    _, seg = single(L, O, w, h, spp)
    dev = L.DeviceScene(scene(O), bg_struct(L, DEFAULT_BG), 0)
    try:
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        stats = torch.zeros(3, dtype=torch.int64, device="cuda")
        p = L.make_params(w, h, DEPTH, spp, RADIUS, SEED)
        dev.render_stats_async(st, p, out.data_ptr(), stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n_seg, n_sphere, _ = stats.tolist()
    finally:
        dev.release()
    assert n_seg == int(seg.sum(dtype=np.int64))
    assert n_sphere > 0
    f32, _ = L.render(scene(O), bg_struct(L, DEFAULT_BG), st,
                      L.make_params(w, h, DEPTH, spp, RADIUS, SEED, output=L.OUT_RGB_F32), 0)
    assert np.array_equal(out.cpu().numpy(), f32)


def test_refill_assign_live_progress_entry_point(L, O):
    """tray_render_progress: the same bits, every row reported, every sample counted."""
    w, h, spp = SIZES[1] + (192,)
    rgb, seg = single(L, O, w, h, spp)
    rows = []
    p = L.make_params(w, h, DEPTH, spp, RADIUS, SEED)
    live, live_seg = L.render(scene(O), bg_struct(L, DEFAULT_BG), camera(L, RICH_SETUP, w, h), p, 0, segments=True,
                              progress=rows.append)
    assert sum(rows) == h, rows
    counts = L.progress_counts(0)
    assert counts.tolist() == [min(8, h - 8 * t) * w * spp for t in range((h + 7) // 8)]
    assert np.array_equal(live, rgb) and np.array_equal(live_seg, seg)


@pytest.mark.parametrize("wave_chunks", [0, 3])
@pytest.mark.parametrize("spp", [1, 16, 32, 48])
def test_refill_assign_paths_that_decode_every_take(L, O, knobs, spp, wave_chunks):
    """r = 16, 32: on-chip sums with several pixel-passes per chunk; r = 1, 48: FP64 sums in sample
    order (no on-chip sums in the plan). They get the straight-line assignment alone."""
    w, h = SIZES[spp % 3 == 0]
    kw = dict(wave_chunks=wave_chunks) if wave_chunks else {}
    knobbed(L, O, knobs, w, h, spp, 3, on_chip=spp in (16, 32), **kw)
