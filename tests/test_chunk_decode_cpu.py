"""The megakernel's per-chunk pixel decode (tray_kernel.hip, `kChunkPixel`), restated in numpy.

A band's work item i = (q x passes + k) x r + s is sample s of pass k of pixel q (8x8-tile order
of the band's compact rows; `decode_item`). With 64 | r a 64-item chunk lies within one pixel and
one pass, so the kernel decodes a chunk's first item once, where a wave takes the chunk, and every
lane of the refill copies it: column, compact row, image row (`row_of`), the RNG pixel index
y x width + x, the pass and the validity are the chunk's, and the RNG sample word is the first
item's + (i & 63). This file shows that identity for every item of a band against the per-item
decode - over r, passes, padding columns and rows, a first pass other than 0, row tiles and a
permuted tile order - and that it fails for r = 16, 32 and 48, which therefore keep the per-lane
decode (the kernel's guard is `kAcc == 1`: on-chip sums with one record per chunk, i.e. 64 | r)."""
import numpy as np
import pytest


def row_of(j, y_start, tile_rows, tile_count, tile_index):
    """Compact output row j -> image row (row_of in tray_device.hpp)."""
    if tile_rows <= 0:
        return y_start + j
    t, within = np.divmod(j, tile_rows)
    return y_start + (t * tile_count + tile_index) * tile_rows + within


def decode_items(i, band):
    """decode_item, row_of and start_sample's index arithmetic for the items `i` of a band:
    (x, j, y, pixel index, pass, sample word, valid), each an int64 array."""
    r, passes, width = band["r"], band["passes"], band["width"]
    s = i % r
    q = i // r
    k = np.zeros_like(i)
    if passes > 1:
        k = q % passes
        q = q // passes
    within = q & 63
    tile = q >> 6
    if band["order"] is not None:  # chunk_tile: the t-th tile of items renders band tile order[t]
        tile = band["order"][tile]
    ty, tx = np.divmod(tile, band["tiles_x"])
    x = tx * 8 + (within & 7)
    jb = ty * 8 + (within >> 3)
    j = band["j0"] + jb
    y = row_of(j, band["y_start"], band["tile_rows"], band["tile_count"], band["tile_index"])
    pixel = y * width + x
    word = (band["pass0"] + k) * r + s
    valid = (x < width) & (jb < band["band_rows"])
    return x, j, y, pixel, k, word, valid


def make_band(r, passes, width, band_rows, j0=0, pass0=0, y_start=0, tile_rows=0, tile_count=1, tile_index=0,
              permute=False):
    tiles_x = (width + 7) // 8
    n_tiles = tiles_x * ((band_rows + 7) // 8)
    order = np.random.default_rng(n_tiles).permutation(n_tiles).astype(np.int64) if permute else None
    return dict(r=r, passes=passes, width=width, band_rows=band_rows, j0=j0, pass0=pass0, y_start=y_start,
                tile_rows=tile_rows, tile_count=tile_count, tile_index=tile_index, tiles_x=tiles_x, order=order,
                items=n_tiles * 64 * r * passes)


def per_item_and_per_chunk(band):
    i = np.arange(band["items"], dtype=np.int64)
    assert band["items"] % 64 == 0  # a band's pixels are whole 8x8 tiles: no partial chunk
    item = decode_items(i, band)
    first = decode_items(i & ~np.int64(63), band)  # the decode the chunk's take keeps
    x, j, y, pixel, k, word0, valid = first
    # the kernel keeps `word0 - first item` and adds the item, in 32-bit wrapping arithmetic
    kept = (word0 - (i & ~np.int64(63))).astype(np.uint32)
    word = (kept + i.astype(np.uint32)).astype(np.int64)
    assert np.array_equal(word, word0 + (i & 63))
    return item, (x, j, y, pixel, k, word, valid)


SHAPES = [(24, 16, 0), (24, 20, 0), (20, 13, 8), (17, 5, 24), (8, 8, 0), (1, 1, 0)]  # width, band rows, j0


@pytest.mark.parametrize("width,band_rows,j0", SHAPES)
@pytest.mark.parametrize("passes", [1, 3, 16])
@pytest.mark.parametrize("r", [64, 128, 192])
def test_chunk_decode_equals_item_decode(r, passes, width, band_rows, j0):
    for pass0 in (0, 7):
        for permute in (False, True):
            band = make_band(r, passes, width, band_rows, j0=j0, pass0=pass0, permute=permute)
            item, chunk = per_item_and_per_chunk(band)
            for name, a, b in zip(("x", "j", "y", "pixel", "pass", "word", "valid"), item, chunk):
                assert np.array_equal(a, b), (name, pass0, permute)
            valid = item[6]
            pad_w, pad_h = width % 8 != 0, band_rows % 8 != 0
            assert (not valid.all()) == (pad_w or pad_h)  # padding occurs exactly where expected
            assert int(valid.sum()) == width * band_rows * r * passes


@pytest.mark.parametrize("tile_rows", [1, 3])
@pytest.mark.parametrize("tile_index", [0, 1, 2])
@pytest.mark.parametrize("r,passes", [(64, 1), (128, 3), (192, 16)])
def test_chunk_decode_with_row_tiles(r, passes, tile_rows, tile_index):
    # a 20 x 13 image cut into row tiles for 3 devices: this device's compact rows, in two bands
    width, height, y_start = 20, 13, 2
    rows = [y for y in range(y_start, height) if ((y - y_start) // tile_rows) % 3 == tile_index]
    seen = []
    for j0 in range(0, len(rows), 8):
        band = make_band(r, passes, width, min(8, len(rows) - j0), j0=j0, pass0=5, y_start=y_start,
                         tile_rows=tile_rows, tile_count=3, tile_index=tile_index, permute=True)
        item, chunk = per_item_and_per_chunk(band)
        for name, a, b in zip(("x", "j", "y", "pixel", "pass", "word", "valid"), item, chunk):
            assert np.array_equal(a, b), name
        valid = item[6]
        seen += sorted(set(item[2][valid].tolist()))
        assert np.array_equal(item[3][valid], item[2][valid] * width + item[0][valid])
    assert seen == rows  # row_of maps the compact rows onto this device's image rows


@pytest.mark.parametrize("r", [16, 32, 48])
def test_chunk_decode_fails_where_a_chunk_holds_several_pixel_passes(r):
    """r = 16, 32: a chunk is 64 / r whole pixel-passes; r = 48: chunks straddle pixels. The first
    item's pixel, pass or sample word is then not every item's, with one pass and with several."""
    for passes in (1, 3):
        band = make_band(r, passes, 24, 20, pass0=7)
        item, chunk = per_item_and_per_chunk(band)
        x, j, y, pixel, k, word, valid = (np.array_equal(a, b) for a, b in zip(item, chunk))
        assert not word
        assert not (pixel and k)  # another pixel (one pass) or another pass of the pixel
    band = make_band(r, 1, 24, 20)
    item, chunk = per_item_and_per_chunk(band)
    assert not np.array_equal(item[3], chunk[3])  # one pass: the chunk's items are several pixels'
