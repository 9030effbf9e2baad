"""The front of the megakernel's refill (tray_kernel.hip), restated in numpy.

Item assignment. A refill hands the wave's idle lanes the next work items: the rest of the current
64-item chunk, then the items of the next chunk, which the wave takes when the current one is
used up. The kernel did this in a loop, one trip per chunk, each trip ranking the lanes that were
still idle. At most 64 lanes are idle and a chunk has 64 items, so the loop never made more than
two trips or more than one take: the kernel now ranks the idle lanes once, gives ranks below
`rest` the current chunk, takes once, and gives rank - rest of the next chunk to the others. Both
forms are restated here and must hand every lane the same item, chunk values and slot, leave the
same pool and call the take in the same state - for every idle count, every chunk remainder,
random idle masks, and with a take that yields a chunk, finds no free slot, or finds the queue dry.

Pixel runs. Item i = (q x passes + k) x r + s: with 64 | r a pixel's items are a run of
passes x r / 64 whole chunks, and all that a take decodes is the pixel's: column, compact row,
padding verdict, and the RNG sample word less the item index, pass0 x r - q x passes x r. So a take
inside the run of the last decode keeps them (`run_first`). For r = 16, 32, 48 a pixel's items are
no whole chunks (with 1 or 3 passes), which is why those instances decode at every take."""
import numpy as np
import pytest

from test_chunk_decode_cpu import decode_items, make_band

NONE = -1  # fresh_item == ~0u


def ranks(mask):
    """mbcnt: set lanes below each lane."""
    return np.cumsum(mask) - mask


class Queue:
    """The take block: a chunk per call (its index, a token for its decoded values, a slot) or
    nothing (no free slot / queue dry: `dry` then sets `exhausted`). Records what each call saw."""

    def __init__(self, first_chunk, outcome):
        self.next, self.outcome, self.calls = first_chunk, outcome, []
        self.exhausted = False

    def take(self, fresh_item):
        self.calls.append(fresh_item.copy())  # `held` of the retire: the lanes assigned so far
        if self.outcome == "no_slot":
            return None
        if self.outcome == "dry":
            self.exhausted = True
            return None
        c = self.next
        self.next += 7  # a wave's takes need not be consecutive
        return dict(first=c * 64, end=c * 64 + 64, values=1000 + c, slot=c % 5)


def assign_loop(idle, pool, queue):
    """The loop the kernel had: a trip per chunk, the still-idle lanes ranked in each."""
    idle = idle.copy()
    item = np.full(64, NONE, np.int64)
    values = np.full(64, NONE, np.int64)
    slot = np.full(64, NONE, np.int64)
    pool = dict(pool)
    while idle.any() and not queue.exhausted:
        if pool["first"] == pool["end"]:
            got = queue.take(item)
            if got is None:
                break
            pool = got
        take = min(int(idle.sum()), pool["end"] - pool["first"])
        lanes = idle & (ranks(idle) < take)
        item[lanes] = pool["first"] + ranks(idle)[lanes]
        values[lanes] = pool["values"]
        slot[lanes] = pool["slot"]
        pool["first"] += take
        idle = idle & (item == NONE)
    return item, values, slot, pool


def assign_two_stage(idle, pool, queue):
    """The kernel's form: one rank, the current chunk's rest, one take at most, the next chunk."""
    item = np.full(64, NONE, np.int64)
    values = np.full(64, NONE, np.int64)
    slot = np.full(64, NONE, np.int64)
    pool = dict(pool)
    if idle.any() and not queue.exhausted:
        n_idle, rank = int(idle.sum()), ranks(idle)

        def stage(first, n):
            lanes = idle & ((rank - first).astype(np.uint32) < n)  # unsigned, as the kernel compares
            item[lanes] = pool["first"] + (rank - first)[lanes]
            values[lanes] = pool["values"]
            slot[lanes] = pool["slot"]
            pool["first"] += n

        rest = min(n_idle, pool["end"] - pool["first"])
        stage(0, rest)
        if n_idle > rest:
            got = queue.take(item)
            if got is not None:
                pool = got
                stage(rest, n_idle - rest)
    return item, values, slot, pool


def both_agree(idle, remainder, outcome, exhausted=False):
    pool = dict(first=640 - remainder, end=640, values=77, slot=3)  # chunk 9 with `remainder` items left
    qa, qb = Queue(20, outcome), Queue(20, outcome)
    qa.exhausted = qb.exhausted = exhausted
    a = assign_loop(idle, pool, qa)
    b = assign_two_stage(idle, pool, qb)
    for name, u, v in zip(("item", "values", "slot"), a, b):
        assert np.array_equal(u, v), (name, remainder, outcome)
    assert a[3] == b[3], (remainder, outcome)
    assert qa.exhausted == qb.exhausted and qa.next == qb.next
    assert len(qa.calls) == len(qb.calls) <= 1
    for u, v in zip(qa.calls, qb.calls):
        assert np.array_equal(u, v)
    return a, len(qa.calls)


@pytest.mark.parametrize("outcome", ["chunk", "no_slot", "dry"])
def test_two_stage_equals_loop_for_every_idle_count_and_remainder(outcome):
    rng = np.random.default_rng(14)
    for n_idle in range(1, 65):
        masks = [np.arange(64) < n_idle, np.arange(64) >= 64 - n_idle]
        masks += [np.isin(np.arange(64), rng.choice(64, n_idle, replace=False)) for _ in range(2)]
        for remainder in range(0, 65):
            for idle in masks:
                (item, values, slot, pool), takes = both_agree(idle, remainder, outcome)
                assert takes == (n_idle > remainder)
                got = item != NONE
                assert not got[~idle].any()
                if outcome == "chunk" or n_idle <= remainder:
                    assert got[idle].all()
                    # items in lane order: the current chunk's rest, then the new chunk's first
                    want = np.r_[np.arange(640 - remainder, 640), np.arange(20 * 64, 21 * 64)][:n_idle]
                    assert np.array_equal(item[idle], want)
                    assert np.array_equal(values[idle] == 77, want < 640)
                    assert np.array_equal(slot[idle], np.where(want < 640, 3, 20 % 5))
                else:  # the lanes of the current chunk's rest go on alone
                    assert int(got.sum()) == remainder and pool["first"] == pool["end"]


def test_two_stage_equals_loop_on_random_masks():
    rng = np.random.default_rng(15)
    for _ in range(2000):
        idle = rng.random(64) < rng.random()
        both_agree(idle, int(rng.integers(0, 65)), ["chunk", "no_slot", "dry"][int(rng.integers(0, 3))])


def test_no_lane_idle_or_queue_dry_assigns_nothing():
    none = np.zeros(64, bool)
    (item, _, _, pool), takes = both_agree(none, 10, "chunk")
    assert takes == 0 and (item == NONE).all() and pool["first"] == 630
    # `exhausted` is set by a take, which runs only with the chunk used up: nothing is left to assign
    (item, _, _, _), takes = both_agree(~none, 0, "chunk", exhausted=True)
    assert takes == 0 and (item == NONE).all()


# --- pixel runs -------------------------------------------------------------------------------------

NO_RUN = 0x80000000  # kNoRun: no chunk of a band (< 2^25) is within a run's length (<= 2^25) of it
SHAPES = [(24, 20, 0), (20, 13, 8), (17, 5, 24), (1, 1, 0)]  # width, band rows, j0: no multiples of 8


def chunk_decodes(band):
    """What a take's full decode keeps of every chunk: (x, j, word - item as the kernel's 32-bit
    value, valid), and the run's first chunk computed from the decode's (pass, sample)."""
    r, passes = band["r"], band["passes"]
    first = np.arange(band["items"] // 64, dtype=np.int64) * 64
    x, j, _, _, k, word, valid = decode_items(first, band)
    s = word - (band["pass0"] + k) * r
    assert np.array_equal(s, first % r)
    kept = (word - first).astype(np.uint32)
    run_first = first // 64 - (k * (r // 64) + s // 64)
    return x, j, kept, valid, run_first


@pytest.mark.parametrize("width,band_rows,j0", SHAPES)
@pytest.mark.parametrize("passes", [1, 3, 16])
@pytest.mark.parametrize("r", [64, 128, 192, 256])
def test_every_chunk_of_a_pixels_run_decodes_alike(r, passes, width, band_rows, j0):
    per_pixel = passes * r // 64
    for pass0, permute in ((0, False), (7, True)):
        band = make_band(r, passes, width, band_rows, j0=j0, pass0=pass0, permute=permute)
        x, j, kept, valid, run_first = chunk_decodes(band)
        c = np.arange(x.size, dtype=np.int64)
        assert np.array_equal(run_first, c // per_pixel * per_pixel)  # (cp, cs) give the run's first chunk
        for name, a in (("x", x), ("j", j), ("word - item", kept), ("padding", valid)):
            assert np.array_equal(a, a[run_first]), (name, pass0, permute)
        q = c // per_pixel
        assert np.array_equal(kept, ((pass0 - q * passes) * r).astype(np.uint32))
        assert (not valid.all()) == (width % 8 != 0 or band_rows % 8 != 0)  # padding runs occur
        # The kernel's test over takes in any order (single-chunk late takes, pool ends): a take
        # reuses the last decode iff its chunk lies in that decode's run, and then gets its own values.
        rng = np.random.default_rng(r + passes)
        state, reused = None, 0
        kept_first = NO_RUN
        order = np.r_[0, rng.integers(0, c.size, 300), np.arange(min(c.size, 3 * per_pixel))[::-1]]
        for t in order:
            if (int(t) - kept_first) % 2**32 < per_pixel:  # unsigned 32-bit, as the kernel compares
                reused += 1
            else:
                state, kept_first = (x[t], j[t], kept[t], valid[t]), int(run_first[t])
            assert state == (x[t], j[t], kept[t], valid[t])
        assert passes * r == 64 or reused > 0


@pytest.mark.parametrize("r", [16, 32, 48])
def test_a_pixels_items_are_no_run_of_chunks_below_64_rays(r):
    """r = 16, 32, 48 with 1 or 3 passes: passes x r is no multiple of 64, so chunks hold several
    pixels or straddle two, and what a chunk's first item decodes to is not every item's of the chunk.
    (With 16 passes a pixel's items happen to be whole chunks again; the kernel picks its instance by r.)"""
    for passes in (1, 3):
        assert passes * r % 64 != 0
        band = make_band(r, passes, 24, 20, pass0=7)
        i = np.arange(band["items"], dtype=np.int64)
        x, j, _, _, _, word, _ = decode_items(i, band)
        x0, j0, _, _, _, word0, _ = decode_items(i & ~np.int64(63), band)
        assert not (np.array_equal(x, x0) and np.array_equal(j, j0))  # another pixel in the chunk
        assert not np.array_equal(word - i, word0 - (i & ~np.int64(63)))  # and another word - item
