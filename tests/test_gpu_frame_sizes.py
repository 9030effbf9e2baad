"""The post-processing kernels at the image sizes where their launch structure changes
(tests/frame_shapes.py; tests/test_frame_shapes_cpu.py holds the shapes to the sources): the capped
grid's second pass of the fold, the selection's metric pass, the whole-frame variance and the sRGB
encoder; the carry of the selection's scan; several tiles per sub-image and the workgroups without a
tile of both a-trous filters. The product reaches some of this only at 4K frames.

Every comparison is of bit patterns against the numpy restatements the small-shape tests use
(progressive_ref, adaptive_ref, denoise_ref, the oracle's encoder), through those tests' helpers:
every output lies between guard words and is pre-filled.
"""
import numpy as np
import pytest

import adaptive_ref as A
import denoise_ref as DR
import frame_shapes as F
import progressive_ref as R
from test_gpu_adaptive import State, random_state
from test_gpu_denoise import assert_same_bits, device_denoise, synthetic
from test_gpu_parity import srgb_thresholds
from test_gpu_progressive import GUARD, Fold, Guarded, assert_state, device_filter, stack_of, synthetic_variance
from test_gpu_query import bits, torch  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
FIRST = F.SECOND_PASS_PIXEL  # the first pixel only a second pass reaches: 1,048,576


def same_record(got, count, most, what):
    assert got[0] == count and bits(np.float64(got[1])) == bits(np.float64(most)), (what, got, count, most)


# --------------------------------------------------------- a. the fold at the cap --
@pytest.fixture(scope="module", params=F.CAP_SHAPES, ids=repr)
def cap(request):
    """Five frames with the header's special values at a cap shape, and the restatement's states
    after two and after all five, computed once."""
    s = request.param
    frames = stack_of(s.rows, s.width, 5)
    two = R.fold(None, frames[:2])
    return dict(shape=s, frames=frames, two=two, five=R.fold(two, frames[2:]))


def test_fold_at_the_cap(L, torch, cap):
    """tray_accum_fold_async, five frames in one call (a second round of the four-frame fetch-ahead)
    and as 2 + 3 (the second call reads a state with count > 0 in the wrapped chunks)."""
    s, frames = cap["shape"], cap["frames"]
    f = Fold(L, torch, s.rows, s.width, variance=False, metric=False)
    back = f.fold(frames)
    assert np.array_equal(bits(back), bits(frames)), "the input frames changed"
    assert_state(f.state(), cap["five"], f"{s}, 5 frames over garbage")
    del f, back
    f = Fold(L, torch, s.rows, s.width, variance=False, metric=False)
    f.fold(frames[:2])
    assert_state(f.state(), cap["two"], f"{s}, first 2")
    f.fold(frames[2:])
    assert_state(f.state(), cap["five"], f"{s}, 2 + 3")
    mean, m2, _ = cap["five"]
    assert np.isnan(mean).any() and np.isinf(m2).any() and np.isfinite(mean).any()  # the special samples are in


def test_fold_with_the_metric_at_the_cap(L, torch, cap):
    """tray_accum_fold_metric_async with the variance and the record: 5 frames at once, 2 + 3, and
    evaluate-only (n_frames = 0) on the folded state, which it must leave alone."""
    s, frames = cap["shape"], cap["frames"]
    shape3 = (s.rows, s.width, 3)
    for parts in ((5,), (2, 3)):
        f = Fold(L, torch, s.rows, s.width)
        done = 0
        for k in parts:
            f.fold(frames[done:done + k])
            done += k
            mean, m2, n = cap["two"] if done == 2 else cap["five"]
            what = f"{s}, {parts}, after {done}"
            assert_state(f.state(), (mean, m2, n), what)
            assert_same_bits(f.variance.get(shape3), R.variance_of_mean(m2, n), what + ": variance")
            count, most, _ = R.metric(mean, m2, n)
            same_record(f.metric(), count, most, what)
            assert 0 < count < s.pixels and most > 0
        del f
    mean, m2, n = cap["five"]
    for mp in ({}, dict(tolerance=0.2, floor=0.25)):
        f = Fold(L, torch, s.rows, s.width, variance=False, metric=False)
        f.fold(frames)
        f.variance, f.record = Guarded(torch, s.pixels * 3), Guarded(torch, 2)
        f.fold(None, **mp)
        assert_state(f.state(), cap["five"], f"{s}, evaluate only {mp}")
        assert_same_bits(f.variance.get(shape3), R.variance_of_mean(m2, n), f"{s}, evaluate only {mp}: variance")
        count, most, _ = R.metric(mean, m2, n, **mp)
        same_record(f.metric(), count, most, f"{s}, evaluate only {mp}")
        del f


@pytest.fixture(scope="module")
def second_pass():
    """1031 x 1019, five frames made for the record: every pixel below FIRST is constant over the
    frames (variance 0: converged, ratio 0), the 2013 pixels from FIRST on are noisy, with one NaN
    sample among them. What the record then counts, it counts through the second pass alone."""
    s = F.by_name(F.CAP_SHAPES)["1031x1019"]
    rng = np.random.default_rng(41)
    level = rng.random((s.pixels, 3))
    frames = np.broadcast_to(level, (5, s.pixels, 3)).copy()
    noisy = s.pixels - FIRST
    frames[:, FIRST:] += 0.2 * rng.random((noisy, 1)) * rng.normal(size=(5, noisy, 3))
    frames[2, FIRST + 100, 1] = NAN
    frames = frames.reshape(5, s.rows, s.width, 3)
    mean, m2, n = R.fold(None, frames)
    count, most, converged = R.metric(mean, m2, n)
    # on the restatement alone: what the stack is meant to produce
    flat = converged.reshape(-1)
    unconverged = np.flatnonzero(~flat)
    assert flat[:FIRST].all() and (m2.reshape(-1, 3)[:FIRST] == 0).all()
    assert 0 < len(unconverged) == count and unconverged.min() >= FIRST and not flat[FIRST + 100]
    assert np.isfinite(most) and most > 0
    return dict(shape=s, frames=frames, state=(mean, m2, n), count=count, most=most)


def test_the_record_counts_what_only_the_second_pass_reaches(L, torch, second_pass):
    s, frames = second_pass["shape"], second_pass["frames"]
    for parts in ((5,), (2, 3)):
        f = Fold(L, torch, s.rows, s.width)
        done = 0
        for k in parts:
            f.fold(frames[done:done + k])
            done += k
        same_record(f.metric(), second_pass["count"], second_pass["most"], f"{s}, {parts}")
        assert_same_bits(f.variance.get((s.rows, s.width, 3)), R.variance_of_mean(*second_pass["state"][1:]),
                         f"{s}, {parts}: variance")
        del f
    f = Fold(L, torch, s.rows, s.width)
    f.fold(frames, tolerance=1e6)  # everything but the NaN pixel converges: the count is 1, from the second pass
    assert f.metric()[0] == 1 == R.metric(*second_pass["state"], tolerance=1e6)[0]


# ------------------------------------------------------------- b. the selection --
SELECT_SHAPES = list({repr(s): s for s in F.CAP_SHAPES + F.SCAN_SHAPES}.values())
BAND_RUNS = (1, 2, 63)  # blocks of SCAN_PIXELS pixels, all active and all inactive in turn
BAND_SHIFT = 500        # the band that starts at block 3 starts this many pixels late


def quiet(rows, width):
    """A state every pixel of which has converged: 5 passes, no spread."""
    return np.full((rows, width, 3), 0.5), np.zeros((rows, width, 3)), np.full((rows, width), 5, np.int32)


def state_random(s):
    kw = dict(min_passes=3, max_passes=8)

    def expect(want):
        assert 0 < want[0]["n_active"] < want[1]["n_active"] < s.pixels
        assert want[0]["unconverged"] > want[0]["n_active"]  # some pixels that need passes have had max_passes

    return random_state(s.rows, s.width, seed=7 * s.rows + s.width), kw, (0, 1), expect


def state_none_active(s):
    """Every pixel at max_passes, half of them converged and the others noisy: unconverged > 0, nothing
    listed with or without dilation."""
    rng = np.random.default_rng(s.pixels)
    mean, m2, count = quiet(s.rows, s.width)
    spent = rng.random((s.rows, s.width)) < 0.5
    m2[spent] = 1.0 + rng.random((int(spent.sum()), 3))
    count[:] = 8

    def expect(want):
        for d in (0, 1):
            assert want[d]["n_active"] == 0 and len(want[d]["pixels"]) == 0
            assert want[d]["unconverged"] == int(spent.sum()) > 0

    return (mean, m2, count), dict(min_passes=3, max_passes=8), (0, 1), expect


def state_all_active(s):
    """Every count below min_passes, max_passes = 2^30: the list is every pixel in order."""
    state = random_state(s.rows, s.width, seed=s.pixels % 1000, max_count=2)

    def expect(want):
        for d in (0, 1):
            assert want[d]["n_active"] == want[d]["unconverged"] == s.pixels
            assert np.array_equal(want[d]["pixels"], np.arange(s.pixels, dtype=np.uint32))

    return state, dict(min_passes=3, max_passes=2 ** 30), (0, 1), expect


def band_mask(pixels):
    blocks = F.ceil_div(pixels, F.SCAN_PIXELS)
    on_block = np.zeros(blocks, dtype=bool)
    b, k = 0, 0
    while b < blocks:
        on_block[b:b + BAND_RUNS[k % 3]] = k % 2 == 0
        b, k = b + BAND_RUNS[k % 3], k + 1
    on = np.repeat(on_block, F.SCAN_PIXELS)[:pixels]
    on[3 * F.SCAN_PIXELS:3 * F.SCAN_PIXELS + BAND_SHIFT] = False  # one boundary in the middle of a block
    return on


def state_banded(s):
    """dilate = 0: whole blocks all active (count 1, below min_passes) or all inactive (converged) in
    runs of 1, 2 and 63 blocks, so the totals are 0 and 1024 and a block's offset is its carry."""
    mean, m2, count = quiet(s.rows, s.width)
    on = band_mask(s.pixels)
    count.reshape(-1)[on] = 1

    def expect(want):
        w = want[0]
        assert np.array_equal(w["active"].reshape(-1), on) and np.array_equal(w["pixels"], np.flatnonzero(on))
        totals = np.add.reduceat(on.astype(np.int64), np.arange(0, s.pixels, F.SCAN_PIXELS))
        assert len(totals) == F.scan(s.pixels)["totals"] and totals[3] == F.SCAN_PIXELS - BAND_SHIFT
        assert set(np.delete(totals[:-1], 3)) == {0, F.SCAN_PIXELS}
        if len(totals) > F.WAVE:  # a total of a later load lands behind what the earlier loads hold
            assert totals[:F.WAVE].sum() > 0 and (totals[F.WAVE:] > 0).any()

    return (mean, m2, count), dict(min_passes=3, max_passes=8), (0,), expect


STATES = dict(random=state_random, none_active=state_none_active, all_active=state_all_active, banded=state_banded)


def check_select(L, torch, s, state, kw, dilates, expect):
    mean, m2, count = state
    want = {d: A.select(mean, m2, count, dilate=d, **kw) for d in dilates}
    expect(want)  # on the restatement: the state produces what it is meant to
    st = State(L, torch, mean, m2, count)
    for d in dilates:
        what = f"{s} dilate {d} {kw}"
        got = st.select(dilate=d, **kw)
        assert_same_bits(got["variance"], want[d]["variance"], what + ": variance")
        assert np.array_equal(got["pixels"], want[d]["pixels"]), what
        assert (got["n_active"], got["unconverged"], got["pixel_passes"]) == \
            (want[d]["n_active"], want[d]["unconverged"], want[d]["pixel_passes"]), what
        assert bits(np.float64(got["max_ratio"])) == bits(np.float64(want[d]["max_ratio"])), what
        again = st.select(dilate=d, **kw)
        assert again["raw"] == got["raw"] and np.array_equal(again["pixels"], got["pixels"]), what + ": a second run"
        assert_same_bits(again["variance"], want[d]["variance"], what + ": a second run: variance")
        none = st.select(variance=False, dilate=d, **kw)
        assert none["raw"] == got["raw"] and np.array_equal(none["pixels"], got["pixels"]), what + ": no variance"
    after = st.get()
    assert np.array_equal(bits(after[0]), bits(mean)) and np.array_equal(bits(after[1]), bits(m2))
    assert np.array_equal(after[2], count)


@pytest.mark.parametrize("which", sorted(STATES))
@pytest.mark.parametrize("shape", SELECT_SHAPES, ids=repr)
def test_select_at_the_cap_and_scan_shapes(L, torch, shape, which):
    state, kw, dilates, expect = STATES[which](shape)
    check_select(L, torch, shape, state, kw, dilates, expect)


def test_select_lists_what_only_the_second_pass_flags(L, torch, second_pass):
    """The state of the record test with 5 passes everywhere: only pixels from FIRST on need passes,
    so without dilation the whole list comes from flags the metric pass wrote in its second pass."""
    s = second_pass["shape"]
    mean, m2, n = second_pass["state"]

    def expect(want):
        assert want[0]["unconverged"] == second_pass["count"] == want[0]["n_active"] > 0
        assert want[0]["pixels"].min() >= FIRST and want[1]["pixels"].min() < FIRST  # dilation reaches a row up
        assert want[0]["max_ratio"] == second_pass["most"]

    check_select(L, torch, s, (mean, m2, np.full((s.rows, s.width), n, np.int32)), dict(min_passes=2, max_passes=64),
                 (0, 1), expect)


# ------------------------------------------------- c. the whole-frame variance --
@pytest.mark.parametrize("shape", F.CAP_SHAPES, ids=repr)
def test_whole_frame_variance_equals_the_formula(L, torch, shape):
    """tray_temporal_var_variance_async with a null list against tray_temporal_variance.h's 2e,
    m2 / (n (n - 1)) with the pixel's own age and +inf below two frames, on planes of its own making:
    the call reads m2 and age and nothing else of the state."""
    s = shape
    rng = np.random.default_rng(s.pixels)
    m2 = rng.random((s.rows, s.width, 3)) * 0.1
    age = rng.choice(np.array([0, 1, 2, 3, 7, 1000, 2 ** 31 - 1], dtype=np.int32), size=(s.rows, s.width))
    flat, ages = m2.reshape(-1, 3), age.reshape(-1)
    for at in (5, FIRST - 3, s.pixels - 1):  # the first pixels, the last of the first pass, the image's last
        flat[at - 5] = (NAN, -1.0, INF)
        flat[at - 4] = (-INF, 0.0, -0.0)
        flat[at - 3, 1] = 1e300
        ages[at - 5:at - 2] = (2, 3, 2 ** 31 - 1)  # the special values are divided, not replaced by +inf
        ages[at - 2:at + 1] = (0, 1, 2)
    want = A.variance(m2, age)
    assert np.isposinf(want).any() and np.isnan(want).any() and np.isneginf(want).any() and (want < 0).any()
    if s.pixels > FIRST:
        assert np.isfinite(want.reshape(-1, 3)[FIRST:]).any()
    dm2 = Guarded(torch, s.pixels * 3)
    dm2.t[GUARD:GUARD + dm2.n] = torch.from_numpy(m2.reshape(-1)).cuda()
    dage = torch.full((s.pixels + 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dage[16:16 + s.pixels] = torch.from_numpy(age.reshape(-1)).cuda()
    out = Guarded(torch, s.pixels * 3)
    st = L.TemporalVarState(None, dm2.ptr, dage.data_ptr() + 64, None, None, s.width, s.rows)
    for run in range(2):
        L.temporal_var_variance_async(st, None, 0, out.ptr, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert_same_bits(out.get((s.rows, s.width, 3)), want, f"{s} run {run}")
    assert np.array_equal(bits(dm2.get((s.rows, s.width, 3))), bits(m2)), "m2 was written"
    back = dage.cpu().numpy()
    assert (back[:16] == 0x5A5A5A5A).all() and (back[16 + s.pixels:] == 0x5A5A5A5A).all()
    assert np.array_equal(back[16:16 + s.pixels], age.reshape(-1)), "age was written"


# -------------------------------------------------------- d. the sRGB encoder --
@pytest.fixture(scope="module")
def srgb_edges(O):
    """test_device_srgb_encoder_bit_exact's values: every byte threshold with its +-3 ulp neighbours,
    then 0, -0, 1, 0.0031308 with their neighbours, clamps, denormals, infinities and NaN."""
    t = srgb_thresholds(O)
    near = (t.view(np.int64)[:, None] + np.arange(-3, 4)[None, :]).reshape(-1).view(np.float64)
    edge = np.float64(0.0031308)
    special = np.array([0.0, -0.0, 1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), edge, np.nextafter(edge, 0),
                        np.nextafter(edge, 1), 0.5, -1.0, 2.0, 1e-300, 5e-324, np.inf, -np.inf, np.nan])
    return np.concatenate([near, special])


@pytest.mark.parametrize("shape", F.CAP_SHAPES, ids=repr)
def test_srgb_encoder_at_the_cap(L, O, torch, srgb_edges, shape):
    """tray_linear_to_srgba_async against the oracle's ToSRGBA, with the edge values in the first
    pixels, in the last pixels below FIRST and from FIRST on (as many as the shape has there)."""
    n = shape.pixels
    rng = np.random.default_rng(n)
    vals = rng.random(3 * n)
    vals[n:2 * n] *= 0.004  # the linear segment and the knee
    vals[2 * n:2 * n + 3000] = rng.random(3000) * 3 - 1
    k = len(srgb_edges)
    vals[:k] = srgb_edges
    vals[3 * FIRST - k:3 * FIRST] = srgb_edges
    beyond = min(k, 3 * n - 3 * FIRST)
    if beyond:
        vals[3 * FIRST:3 * FIRST + beyond] = srgb_edges[k - beyond:]
        assert np.isnan(vals[3 * FIRST:]).any()
    assert beyond == min(k, 3 * F.srgb(n)["wrapped_threads"])
    want = O.linear_to_srgb_n(vals).reshape(n, 3)
    rgb = torch.from_numpy(vals).cuda()
    out = torch.full((4 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    for run in range(2):
        L.linear_to_srgba_async(rgb.data_ptr(), n, out.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[4 * n:] == 0xA5).all(), "the bytes after the output changed"
        got = got[:4 * n].reshape(n, 4)
        bad = np.flatnonzero((got[:, :3] != want).any(axis=1) | (got[:, 3] != 255))
        assert bad.size == 0, \
            f"{shape} run {run}: {bad.size} pixels differ, first {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"
    assert np.array_equal(bits(rgb.cpu().numpy()), bits(vals)), "the input changed"


# ------------------------------------------------------------ e. both filters --
FILTER_CASES = [(s, 5) for s in F.FILTER_SHAPES] + [(F.FILTER_SHAPES[0], 8)]  # 8: spacing 128, both ping-pong buffers
FILTER_IDS = [f"{s}-{it}" for s, it in FILTER_CASES]


@pytest.mark.parametrize("flags", [1, 0])
@pytest.mark.parametrize("shape,iterations", FILTER_CASES, ids=FILTER_IDS)
def test_denoise_at_the_filter_shapes(L, torch, shape, iterations, flags):
    colour, albedo, normal, depth = synthetic(shape.rows, shape.width)
    kw = dict(iterations=iterations, flags=flags, sigma_color=0.75, sigma_normal=0.5, sigma_depth=0.25)
    want = DR.denoise(colour, albedo, normal, depth, **kw)
    got = device_denoise(L, torch, colour, albedo, normal, depth, **kw)
    assert_same_bits(got, want, f"{shape} {iterations} iterations flags {flags}")
    assert np.array_equal(np.isnan(got), np.isnan(colour)) and np.isnan(colour).any()
    assert not np.array_equal(got[np.isfinite(colour)], colour[np.isfinite(colour)])


@pytest.mark.parametrize("flags", [1, 0])
@pytest.mark.parametrize("shape,iterations", FILTER_CASES, ids=FILTER_IDS)
def test_variance_filter_at_the_filter_shapes(L, torch, shape, iterations, flags):
    colour, albedo, normal, depth = synthetic(shape.rows, shape.width)
    variance = synthetic_variance(shape.rows, shape.width, colour)
    kw = dict(iterations=iterations, flags=flags, sigma_variance=3.0, sigma_normal=0.5, sigma_depth=0.25, epsilon=1e-9)
    want, want_v = R.denoise_variance(colour, variance, albedo, normal, depth, **kw)
    got, got_v = device_filter(L, torch, colour, variance, albedo, normal, depth, **kw)
    what = f"{shape} {iterations} iterations flags {flags}"
    assert_same_bits(got, want, what)
    assert_same_bits(got_v, want_v, what + ": variance_out")
    assert np.array_equal(np.isnan(got), np.isnan(colour)) and np.isnan(colour).any()
    assert not np.array_equal(got[np.isfinite(colour)], colour[np.isfinite(colour)])
    assert np.isnan(got_v).any() and np.isinf(got_v).any()
