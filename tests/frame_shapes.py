"""The shapes of tests/test_gpu_frame_sizes.py: the image sizes at which the post-processing kernels
change their launch structure, with a small model of that structure and, per shape, what the model
must show. tests/test_frame_shapes_cpu.py reads the constants below out of the sources and asserts
every shape against the model, so that a change of a cap or of a tile cannot move a case off the
threshold it stands for without a test saying so.

The structures (rows x width throughout):
  * the streaming kernels (accum_fold_kernel, adaptive_metric_kernel,
    temporal_variance_frame_kernel; tray_stream.hpp): an image is cut into chunks of BLOCK_ELEMS
    doubles, one per workgroup, and the grid is capped at MAX_GRID: above MAX_GRID chunks workgroup g
    takes chunk g + MAX_GRID in a second pass of its loop;
  * the sRGB encoder (launch_to_srgba): SRGB_THREADS pixels per block, at most SRGB_MAX_BLOCKS
    blocks, a grid-stride loop;
  * the selection's scan (adaptive_scan_kernel): one total per SCAN_PIXELS pixels, scanned by one
    wave WAVE totals at a time with a carry between loads;
  * the a-trous filters (plan_level and denoise_level's block decode, tray_denoise.hip): at spacing
    s the image is s x s sub-images, each cut into TILE_X x TILE_Y tiles; every sub-image gets the
    tiles of the largest one, and a workgroup whose tile starts outside its own, shorter sub-image
    returns early.
"""
import numpy as np

# tray_stream.hpp
WAVE = 64
WAVE_ELEMS = 384       # kWaveElems: doubles one wave owns
BLOCK_ELEMS = 1536     # kBlockElems: doubles per chunk (512 pixels)
MAX_GRID = 2048        # kMaxGrid
FRAMES_AHEAD = 4       # kFramesAhead, tray_progressive.hip
# launch_to_srgba, tray_kernel.hip
SRGB_THREADS, SRGB_MAX_BLOCKS = 256, 4096
# tray_adaptive.hip
SCAN_PIXELS = 1024     # kScanPixels
# tray_denoise.hip
TILE_X, TILE_Y = 32, 8

# The first pixel that only a second pass reaches, of the streaming kernels and of the encoder alike.
SECOND_PASS_PIXEL = MAX_GRID * BLOCK_ELEMS // 3
assert SECOND_PASS_PIXEL == SRGB_MAX_BLOCKS * SRGB_THREADS == 1 << 20


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the model --
def streaming(pixels, block_elems=BLOCK_ELEMS, max_grid=MAX_GRID, wave_elems=WAVE_ELEMS):
    """The launch of a streaming kernel over `pixels` pixels of three doubles."""
    elems = 3 * pixels
    chunks = ceil_div(elems, block_elems)
    grid = min(chunks, max_grid)
    tail = elems - (chunks - 1) * block_elems  # doubles in the last chunk
    return dict(elems=elems, chunks=chunks, grid=grid,
                passes=ceil_div(chunks, grid),            # the most chunks one workgroup takes
                wrapped=min(max(chunks - grid, 0), grid),  # workgroups 0 .. wrapped - 1 take a second chunk
                tail=tail, tail_wave=(tail - 1) // wave_elems,
                tail_in_second_pass=chunks > grid,
                second_pass_pixels=max(pixels - grid * block_elems // 3, 0))


def srgb(pixels, threads=SRGB_THREADS, max_blocks=SRGB_MAX_BLOCKS):
    """launch_to_srgba: the blocks the image asks for, the grid, the threads that go round again."""
    blocks = ceil_div(pixels, threads)
    grid = min(blocks, max_blocks)
    return dict(blocks=blocks, srgb_grid=grid, wrapped_threads=max(pixels - grid * threads, 0))


def scan(pixels, scan_pixels=SCAN_PIXELS, wave=WAVE):
    """adaptive_scan_kernel: block totals, loads of one wave, the pixels of the last block, and the
    totals that are added to a carry from an earlier load."""
    totals = ceil_div(pixels, scan_pixels)
    return dict(totals=totals, loads=ceil_div(totals, wave), last=pixels - (totals - 1) * scan_pixels,
                carried=max(totals - wave, 0))


def filter_level(rows, width, s, tile_x=TILE_X, tile_y=TILE_Y):
    """plan_level and the block decode of denoise_level at spacing s: tiles per sub-image, workgroups,
    those that return early, and the pixels the others filter (each in-image point of a tile)."""
    sub_w, sub_h = ceil_div(width, s), ceil_div(rows, s)
    tiles_x, tiles_y = ceil_div(sub_w, tile_x), ceil_div(sub_h, tile_y)
    lattices_x, lattices_y = min(s, width), min(s, rows)
    blocks = tiles_x * tiles_y * lattices_x * lattices_y
    b = np.arange(blocks, dtype=np.int64)
    tx, b = b % tiles_x, b // tiles_x
    ty, b = b % tiles_y, b // tiles_y
    off_x, off_y = b % lattices_x, b // lattices_x
    x0, y0 = off_x + tx * tile_x * s, off_y + ty * tile_y * s  # the tile's first pixel
    skipped = (x0 >= width) | (y0 >= rows)
    nx = np.clip(-(-(width - x0) // s), 0, tile_x)
    ny = np.clip(-(-(rows - y0) // s), 0, tile_y)
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, blocks=blocks, skipped=int(skipped.sum()),
                filtered=int((nx * ny)[~skipped].sum()))


# ------------------------------------------------------------------ the shapes --
class Shape:
    def __init__(self, rows, width, **facts):
        self.rows, self.width, self.pixels, self.facts = rows, width, rows * width, facts

    def __repr__(self):
        return f"{self.rows}x{self.width}"


# The four streaming kernels and the encoder around their caps. Facts: of streaming() and srgb().
CAP_SHAPES = [
    # the last size of the old regime: exactly MAX_GRID chunks and SRGB_MAX_BLOCKS blocks
    Shape(1024, 1024, chunks=2048, passes=1, wrapped=0, tail=1536, tail_wave=3, second_pass_pixels=0,
          blocks=4096, wrapped_threads=0),
    # one pixel more: one workgroup wraps for 3 doubles, one encoder thread wraps
    Shape(1, 1048577, chunks=2049, passes=2, wrapped=1, tail=3, tail_wave=0, second_pass_pixels=1,
          blocks=4097, wrapped_threads=1),
    # 1,050,589 pixels, 3,151,767 doubles (odd: every frame after the first starts 8 bytes off a
    # 16-byte boundary); workgroups 0-3 wrap, the partial last chunk's tail lies in wave 3
    Shape(1031, 1019, chunks=2052, passes=2, wrapped=4, tail=1431, tail_wave=3, second_pass_pixels=2013,
          blocks=4104, wrapped_threads=2013),
]

# The scan of the block totals. Facts: of scan().
SCAN_SHAPES = [
    Shape(64, 1024, totals=64, loads=1, last=1024, carried=0),   # one full load, no carry
    Shape(257, 255, totals=64, loads=1, last=1023, carried=0),   # the last total short by one pixel
    Shape(65, 1009, totals=65, loads=2, last=49, carried=1),     # the carry reaches one block of 49 pixels
    Shape(129, 1024, totals=129, loads=3, last=1024, carried=65),
    Shape(1031, 1019, totals=1026, loads=17, last=989, carried=962),
]

# The filters. Facts per spacing 1, 2, 4, 8, 16: (tiles across, tiles down, workgroups, skipped).
FILTER_SPACINGS = (1, 2, 4, 8, 16)
FILTER_SHAPES = [
    # skipped workgroups at every spacing from 2 on, in x and in y
    Shape(129, 513, levels=[(17, 17, 289, 0), (9, 9, 324, 35), (5, 5, 400, 111), (3, 3, 576, 287), (2, 2, 1024, 735)]),
    # several tiles at every level, skipped workgroups at spacing 16 alone
    Shape(137, 523, levels=[(17, 18, 306, 0), (9, 9, 324, 0), (5, 5, 400, 0), (3, 3, 576, 0), (2, 2, 1024, 349)]),
    # the first one, one tile high from spacing 2 on: skipped in x alone
    Shape(9, 513, levels=[(17, 2, 34, 0), (9, 1, 36, 2), (5, 1, 80, 12), (3, 1, 192, 56), (2, 1, 288, 135)]),
]


def by_name(shapes):
    return {repr(s): s for s in shapes}
