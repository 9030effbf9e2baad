"""The shapes of tests/frame_shapes.py against the sources: the constants the launch model stands on
are read out of the .hip and .hpp files, and every shape must still cross the threshold it is named
for when the model runs on them ("the case proves what it says"). A later change that raises a cap
or resizes a tile fails here, instead of tests/test_gpu_frame_sizes.py quietly no longer reaching the
second pass, the carry or the skipped workgroups."""
import os
import re

import pytest

import frame_shapes as F
from conftest import ROOT

CSRC = os.path.join(ROOT, "tray_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constants(text):
    """Every `constexpr <integer type> kName = <expression>[, kName = <expression>];` of a source
    file, evaluated in order: the expressions are sums, products and quotients of integers and of
    earlier names."""
    values = {}
    for decl in re.findall(r"constexpr\s+(?:int|int32_t|int64_t|uint32_t|size_t)\s+(k\w+\s*=[^;]+);", text):
        for name, expr in re.findall(r"(k\w+)\s*=\s*([^,;]+)", decl):
            expr = re.sub(r"\(\s*(?:u?int\d+_t|int|size_t)\s*\)", "", expr)  # casts
            expr = re.sub(r"(\d+)(?:ull|ll|u)\b", r"\1", expr)                # integer suffixes
            if not re.fullmatch(r"[\w\s*/+\-()<]+", expr):
                continue
            try:
                values[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(values)))
            except (NameError, SyntaxError, TypeError):
                continue  # stands on something that is not a plain integer constant
    return values


@pytest.fixture(scope="module")
def sources():
    stream = constants(source("tray_stream.hpp"))
    srgb = re.search(r"std::min<size_t>\(\(n_pixels \+ (\d+)\) / (\d+), (\d+)\);\s*"
                     r"hipLaunchKernelGGL\(to_srgba_kernel, dim3\(\(uint32_t\)blocks\), dim3\((\d+)\)",
                     source("tray_kernel.hip"))
    assert srgb, "launch_to_srgba no longer sizes its grid as min(ceil(n / threads), cap)"
    round_up, per_block, cap, threads = (int(v) for v in srgb.groups())
    assert round_up + 1 == per_block == threads
    stride = re.search(r"i \+= \(size_t\)gridDim\.x \* (\d+)u\)", source("tray_kernel.hip"))
    assert stride and int(stride.group(1)) == threads  # to_srgba_kernel's grid-stride loop
    return dict(stream=stream, progressive=constants(source("tray_progressive.hip")),
                adaptive=constants(source("tray_adaptive.hip")), denoise=constants(source("tray_denoise.hip")),
                srgb_threads=threads, srgb_max_blocks=cap)


def test_the_models_constants_are_the_sources(sources):
    s = sources["stream"]
    # kBlockElems from its factors: four waves of three rows of 128 doubles
    assert s["kBlockElems"] == (s["kThreads"] // s["kWave"]) * s["kSlots"] * 2 * s["kWave"]
    assert (s["kWave"], s["kWaveElems"], s["kBlockElems"], s["kMaxGrid"]) == \
        (F.WAVE, F.WAVE_ELEMS, F.BLOCK_ELEMS, F.MAX_GRID)
    assert s["kBlockElems"] % 3 == 0  # a chunk holds whole pixels: SECOND_PASS_PIXEL is a pixel index
    assert sources["progressive"]["kFramesAhead"] == F.FRAMES_AHEAD
    assert sources["adaptive"]["kScanPixels"] == F.SCAN_PIXELS
    assert (sources["denoise"]["kTileX"], sources["denoise"]["kTileY"]) == (F.TILE_X, F.TILE_Y)
    assert (sources["srgb_threads"], sources["srgb_max_blocks"]) == (F.SRGB_THREADS, F.SRGB_MAX_BLOCKS)


@pytest.mark.parametrize("name", ["tray_progressive.hip", "tray_adaptive.hip", "tray_temporal.hip"])
def test_the_streaming_launches_cap_their_grid_at_kMaxGrid(name):
    text = source(name)
    assert re.search(r"chunks < kMaxGrid \? \(int64_t\)\w+\.chunks : kMaxGrid", text), name
    assert re.search(r"for \(size_t chunk = blockIdx\.x; chunk < A\.chunks; chunk \+= gridDim\.x\)", text), name
    assert re.search(r"chunks = \(\w+\.elems \+ kBlockElems - 1\) / kBlockElems", text), name


def model(sources):
    s = sources["stream"]
    return dict(stream=dict(block_elems=s["kBlockElems"], max_grid=s["kMaxGrid"], wave_elems=s["kWaveElems"]),
                srgb=dict(threads=sources["srgb_threads"], max_blocks=sources["srgb_max_blocks"]),
                scan=dict(scan_pixels=sources["adaptive"]["kScanPixels"], wave=s["kWave"]),
                tile=dict(tile_x=sources["denoise"]["kTileX"], tile_y=sources["denoise"]["kTileY"]))


@pytest.mark.parametrize("shape", F.CAP_SHAPES, ids=repr)
def test_cap_shapes(sources, shape):
    m = model(sources)
    got = dict(F.streaming(shape.pixels, **m["stream"]), **F.srgb(shape.pixels, **m["srgb"]))
    assert {k: got[k] for k in shape.facts} == shape.facts, (shape, got)
    first = m["stream"]["max_grid"] * m["stream"]["block_elems"] // 3
    assert first == F.SECOND_PASS_PIXEL == m["srgb"]["threads"] * m["srgb"]["max_blocks"]
    # what the names say, whatever the numbers: the old regime's last size, then the wrap
    if shape.pixels <= first:
        assert shape.pixels == first and got["passes"] == 1 and got["blocks"] == got["srgb_grid"] and got["chunks"] == got["grid"]
    else:
        assert got["passes"] == 2 and got["tail_in_second_pass"] and got["wrapped"] >= 1
        assert got["second_pass_pixels"] == got["wrapped_threads"] == shape.pixels - first > 0


def test_the_odd_cap_shape_is_odd():
    """1031 x 1019: an odd number of doubles per frame (frames after the first start 8 bytes off a
    16-byte boundary), several wrapped workgroups, and the tail inside the last wave of its chunk."""
    got = F.streaming(F.by_name(F.CAP_SHAPES)["1031x1019"].pixels)
    assert got["elems"] == 3151767 and got["elems"] % 2 == 1
    assert got["wrapped"] == 4 and got["tail"] % F.WAVE_ELEMS != 0
    assert got["tail_wave"] == F.BLOCK_ELEMS // F.WAVE_ELEMS - 1
    assert F.FRAMES_AHEAD < 5  # the five frames of the fold tests take a second round of the fetch-ahead loop


@pytest.mark.parametrize("shape", F.SCAN_SHAPES, ids=repr)
def test_scan_shapes(sources, shape):
    got = F.scan(shape.pixels, **model(sources)["scan"])
    assert {k: got[k] for k in shape.facts} == shape.facts, (shape, got)


def test_the_scan_shapes_stand_on_both_sides_of_one_load(sources):
    wave = sources["stream"]["kWave"]
    totals = sorted(F.scan(s.pixels, **model(sources)["scan"])["totals"] for s in F.SCAN_SHAPES)
    assert totals[:3] == [wave, wave, wave + 1] and totals[3] > 2 * wave and totals[4] > 16 * wave


@pytest.mark.parametrize("shape", F.FILTER_SHAPES, ids=repr)
def test_filter_shapes(sources, shape):
    for s, want in zip(F.FILTER_SPACINGS, shape.facts["levels"]):
        got = F.filter_level(shape.rows, shape.width, s, **model(sources)["tile"])
        assert (got["tiles_x"], got["tiles_y"], got["blocks"], got["skipped"]) == want, (shape, s, got)
        assert got["filtered"] == shape.pixels, (shape, s, got)  # the model itself: every pixel once


def test_the_filter_shapes_reach_what_the_older_ones_do_not(sources):
    """More than one tile across at every spacing up to 16 and workgroups that return early. No shape
    of tests/test_gpu_denoise.py's CASES, nor 64 x 36 or 160 x 90, has a workgroup that returns early,
    and those compared bit for bit (all but 160 x 90) have one tile across from spacing 4 on."""
    tile = model(sources)["tile"]
    levels = {repr(s): [F.filter_level(s.rows, s.width, sp, **tile) for sp in F.FILTER_SPACINGS]
              for s in F.FILTER_SHAPES}
    assert all(lv["tiles_x"] >= 2 for name in levels for lv in levels[name])
    assert all(lv["skipped"] > 0 for lv in levels["129x513"][1:])
    assert all(lv["tiles_y"] >= 2 for lv in levels["129x513"])
    assert [lv["skipped"] > 0 for lv in levels["137x523"]] == [False, False, False, False, True]
    assert all(lv["tiles_y"] == 1 and lv["skipped"] > 0 for lv in levels["9x513"][1:])
    older = [(23, 37), (1, 1), (1, 40), (40, 1), (45, 70), (40, 100), (36, 64), (90, 160)]
    for rows, width in older:
        for sp in F.FILTER_SPACINGS + (32, 64, 128):
            lv = F.filter_level(rows, width, sp, **tile)
            assert lv["skipped"] == 0 and lv["filtered"] == rows * width, (rows, width, sp, lv)
            assert sp < 4 or lv["tiles_x"] == 1 or (rows, width) == (90, 160), (rows, width, sp, lv)
