"""Adaptive sampling (include/tray_adaptive.h) on the device: the renderer over a pixel list
against tray_render_async with the ordered sum, the fold with per-pixel counts and the
selection step against tests/adaptive_ref.py (written from the header), the invariant of
Tracer.RenderAdaptive's loop, and its conditions against the uniform RenderProgressive.

Every device-against-reference comparison is of bit patterns. Outputs are pre-filled with NaN
(or a marker) and the double outputs lie between guard words that must come back unchanged.
"""
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as A
import progressive_ref as R
from conftest import DEFAULT_BG, RICH_SETUP, ROOT
from test_gpu_denoise import assert_same_bits, book_frame, device_denoise
from test_gpu_parity import bg_struct, camera
from test_gpu_progressive import Fold, Guarded, _tracer, device_filter, device_passes
from test_gpu_query import bits, rich2, torch  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
W, H, DEPTH, SEED = 40, 24, 20, 2
MARK = 0x5A5A5A5A  # pre-fill of uint32 outputs
# The conditions test's margin on MSE(adaptive) / MSE(uniform): the worst ratio the CPU sweep
# (tools/adaptive_sweep.py on the oracle, profiles/adaptive_sweep.jsonl) measured for
# the default min_passes 8 and dilate 1, 1.6825 at 64x36, plus the spread of that ratio across its
# three sizes, 0.4558 (1.2267 at 32x18). Adaptive stops a pixel at the tolerance where the uniform
# run goes on refining it, so the ratio is above 1 by construction. Not tuned on the device result.
MSE_MARGIN = 1.6825 + 0.4558


@pytest.fixture(scope="module")
def dev_book(L, rich2, torch):
    dev = L.DeviceScene(rich2, bg_struct(L, DEFAULT_BG), 0)
    yield dev
    dev.release()


def i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()


def device_pixels(L, torch, dev, st, params, pixels, n_passes=1, plane=None, segments=True, stream=None):
    """tray_render_pixels_async -> ((n_passes, n, 3) float64, (n_passes, n) uint32 or None)."""
    n = len(pixels)
    out = Guarded(torch, max(n_passes * n * 3, 1))
    seg = torch.full((n_passes * n + 32,), MARK, dtype=torch.int32, device="cuda") if segments else None
    lst = i32(torch, pixels) if n else None
    pl = None if plane is None else torch.from_numpy(np.ascontiguousarray(plane, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    dev.render_pixels_async(st, params, lst.data_ptr() if n else None, n, out.ptr, n_passes,
                            pass_plane_ptr=None if pl is None else pl.data_ptr(),
                            segments_ptr=None if seg is None else seg.data_ptr() + 64,
                            stream=stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.get()[:n_passes * n * 3].reshape(n_passes, n, 3)
    if seg is None:
        return got, None
    s = seg.cpu().numpy().view(np.uint32)
    assert (s[:16] == MARK).all() and (s[16 + n_passes * n:] == MARK).all(), "segment guards changed"
    return got, s[16:16 + n_passes * n].reshape(n_passes, n)


def ordered_frames(L, torch, dev, st, passes, **pkw):
    """tray_render_async | TRAY_FLAG_ORDERED_SUM, one full render per pass: {pass: (frame, segments)}."""
    out = {}
    flags = pkw.pop("flags", 0) | L.FLAG_ORDERED_SUM
    for k in passes:
        p = L.make_params(flags=flags, pass_=k, **pkw)
        rows = L.params_rows(p)
        frame = torch.full((rows, p.width, 3), NAN, dtype=torch.float64, device="cuda")
        seg = torch.zeros((rows, p.width), dtype=torch.int32, device="cuda")
        dev.render_async(st, p, frame.data_ptr(), seg.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out[k] = (frame.cpu().numpy().reshape(-1, 3), seg.cpu().numpy().view(np.uint32).reshape(-1))
    return out


def check_list(got, seg, frames, pixels, passes_of, what):
    """got[k, i] must be frames[passes_of(k, pixel)][pixel]; an out-of-range entry holds zeros."""
    total = len(next(iter(frames.values()))[0])
    for k in range(got.shape[0]):
        for i, pix in enumerate(pixels):
            if pix >= total:
                assert (bits(got[k, i]) == 0).all() and (seg is None or seg[k, i] == 0), (what, k, i, "bad entry")
                continue
            frame, fseg = frames[passes_of(k, int(pix))]
            assert (bits(got[k, i]) == bits(frame[pix])).all(), \
                f"{what}: pass index {k}, entry {i} (pixel {pix}): {got[k, i]!r} for {frame[pix]!r}"
            assert seg is None or seg[k, i] == fseg[pix], (what, k, i, int(seg[k, i]), int(fseg[pix]))


# ------------------------------------------------ 1. the renderer over a pixel list --
@pytest.mark.parametrize("scan", ["bvh", "linear_scan"])
@pytest.mark.parametrize("r", [1, 3, 16])
def test_render_pixels_equals_the_ordered_render(L, torch, dev_book, r, scan):
    """40 x 24 book cover, depth 20: every list, pass count and pass plane gives, per (pixel, pass),
    the bits and the segment count of the full ordered-sum render of that pass."""
    flags = L.FLAG_LINEAR_SCAN if scan == "linear_scan" else 0
    st = camera(L, RICH_SETUP, W, H)
    kw = dict(width=W, height=H, max_depth=DEPTH, rays_per_pixel=r, ray_radius=0.5, seed=SEED, flags=flags)
    frames = ordered_frames(L, torch, dev_book, st, range(7), **kw)
    assert not np.array_equal(frames[0][0], frames[1][0])
    n = W * H
    lists = {"all": np.arange(n), "every_7th": np.arange(3, n, 7), "one": np.array([517]), "empty": np.arange(0),
             "bad_entry": np.array([5, n, 6, 2 ** 32 - 1, 900, n + 1, 7])}
    plane = (np.arange(n) % 4).astype(np.int32)
    for name, lst in lists.items():
        for n_passes in (1, 3):
            for pl, first in ((None, 0), (plane, 1)):
                # ordered sum accepted and changing nothing: set on every other call
                f = flags | (L.FLAG_ORDERED_SUM if n_passes == 3 else 0)
                p = L.make_params(W, H, DEPTH, r, 0.5, SEED, flags=f, pass_=first)
                got, seg = device_pixels(L, torch, dev_book, st, p, lst, n_passes, pl)
                assert got.shape == (n_passes, len(lst), 3)
                check_list(got, seg, frames, lst, lambda k, pix: first + (0 if pl is None else int(pl[pix])) + k,
                           f"r={r} {scan} {name} n_passes={n_passes} plane={pl is not None}")
    got, seg = device_pixels(L, torch, dev_book, st, L.make_params(W, H, DEPTH, r, 0.5, SEED, flags=flags),
                             lists["every_7th"], 2, segments=False)  # without segments
    check_list(got, None, frames, lists["every_7th"], lambda k, pix: k, "no segments")


def test_render_pixels_more_than_256_samples(L, torch, dev_book):
    """r = 300: a group is a whole workgroup and takes two rounds (256 + 44 samples)."""
    st = camera(L, RICH_SETUP, W, H)
    kw = dict(width=W, height=H, max_depth=8, rays_per_pixel=300, ray_radius=0.5, seed=SEED)
    frames = ordered_frames(L, torch, dev_book, st, (0, 1), **kw)
    lst = np.array([0, 39, 400, 401, 517, 700, 959, 5000])
    got, seg = device_pixels(L, torch, dev_book, st, L.make_params(W, H, 8, 300, 0.5, SEED), lst, 2)
    check_list(got, seg, frames, lst, lambda k, pix: k, "r=300")


def test_render_pixels_default_scene_without_bvh(L, O, torch):
    """The 5-sphere default scene has no BVH: the linear scan, with an open aperture."""
    setup = np.array([-2.0, 2, 1, 0, 0, -1, 0, 1, 0, 20.0, 1.0, 3.4641016151377544, 0.1])
    st = camera(L, setup, W, H)
    dev = L.DeviceScene(O.default_scene(), bg_struct(L, DEFAULT_BG), 0)
    try:
        assert dev.info().has_bvh == 0
        kw = dict(width=W, height=H, max_depth=DEPTH, rays_per_pixel=5, ray_radius=0.5, seed=7)
        frames = ordered_frames(L, torch, dev, st, (0, 1, 2), **kw)
        lst = np.arange(0, W * H, 3)
        got, seg = device_pixels(L, torch, dev, st, L.make_params(W, H, DEPTH, 5, 0.5, 7, pass_=1), lst, 2)
        check_list(got, seg, frames, lst, lambda k, pix: 1 + k, "default scene")
        assert len({int(s) for s in seg.reshape(-1)}) > 3  # paths of several lengths: the spheres are in view
    finally:
        dev.release()


@pytest.mark.parametrize("name,rowkw", [("y_start_5", dict(y_start=5, y_end=17)),
                                        ("tiles", dict(y_start=0, y_end=24, tile_rows=2, tile_count=3, tile_index=1))])
def test_render_pixels_row_sets(L, torch, dev_book, name, rowkw):
    """The list indexes the compact rows of the row set; the draws use the image's coordinates."""
    st = camera(L, RICH_SETUP, W, H)
    kw = dict(width=W, height=H, max_depth=DEPTH, rays_per_pixel=3, ray_radius=0.5, seed=SEED, **rowkw)
    frames = ordered_frames(L, torch, dev_book, st, (0, 1), **kw)
    p = L.make_params(W, H, DEPTH, 3, 0.5, SEED, **rowkw)
    rows = L.params_rows(p)
    assert rows == (12 if name == "y_start_5" else 8)
    lst = np.concatenate([np.arange(rows * W)[::-1], [rows * W]])  # descending, and the first index outside
    got, seg = device_pixels(L, torch, dev_book, st, p, lst, 2)
    check_list(got, seg, frames, lst, lambda k, pix: k, name)
    full = ordered_frames(L, torch, dev_book, st, (0,), width=W, height=H, max_depth=DEPTH, rays_per_pixel=3,
                          ray_radius=0.5, seed=SEED)[0][0]
    assert not np.array_equal(frames[0][0][:W], full[:W])  # the row set is not the image's first rows


# ------------------------------------------------------------- 2. the sparse fold --
class State:
    """A tray_adaptive_state on the device: mean and m2 between guard words, and the counts."""

    def __init__(self, L, torch, mean, m2, count):
        self.L, self.torch = L, torch
        self.rows, self.width = count.shape
        n = count.size * 3
        self.mean, self.m2 = Guarded(torch, n), Guarded(torch, n)
        self.mean.t[64:64 + n] = torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)).cuda()
        self.m2.t[64:64 + n] = torch.from_numpy(np.ascontiguousarray(m2, dtype=np.float64).reshape(-1)).cuda()
        self.count = torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).cuda()
        self.st = L.AdaptiveState(self.mean.ptr, self.m2.ptr, self.count.data_ptr(), self.width, self.rows)

    def fold(self, pixels, values, stream=None):
        lst, v = i32(self.torch, pixels), self.torch.from_numpy(np.ascontiguousarray(values)).cuda()
        self.torch.cuda.synchronize()
        self.L.adaptive_fold_async(self.st, lst.data_ptr(), len(pixels), v.data_ptr(), values.shape[0], 0,
                                   stream if stream is not None else self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        assert np.array_equal(bits(v.cpu().numpy()), bits(values)), "the values changed"

    def get(self):
        shape = (self.rows, self.width, 3)
        return self.mean.get()[:self.count.numel() * 3].reshape(shape), \
            self.m2.get()[:self.count.numel() * 3].reshape(shape), self.count.cpu().numpy()

    def select(self, variance=True, stream=None, **params):
        L, torch = self.L, self.torch
        n = self.rows * self.width
        ap = L.adaptive_params(**params)
        var = Guarded(torch, n * 3) if variance else None
        lst = torch.full((n + 32,), MARK, dtype=torch.int32, device="cuda")
        rec = Guarded(torch, 4, fill=-3.0)
        nbytes = L.adaptive_workspace_bytes(self.width, self.rows)
        assert nbytes % 8 == 0
        work = Guarded(torch, nbytes // 8)  # NaN bytes: the call owes the workspace no contents
        torch.cuda.synchronize()
        L.adaptive_select_async(self.st, ap, lst.data_ptr() + 64, rec.ptr, work.ptr, nbytes,
                                var.ptr if var else None, 0,
                                stream if stream is not None else torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        work.get()  # the guards around the workspace
        r = rec.get().view(L.ADAPTIVE_RECORD_DTYPE)[0]
        raw = lst.cpu().numpy().view(np.uint32)
        k = int(r["n_active"])
        assert (raw[:16] == MARK).all() and (raw[16 + k:] == MARK).all(), "the list wrote beyond n_active entries"
        return dict(variance=var.get()[:n * 3].reshape(self.rows, self.width, 3) if var else None,
                    pixels=raw[16:16 + k].copy(), n_active=k, unconverged=int(r["unconverged"]),
                    max_ratio=float(r["max_ratio"]), pixel_passes=int(r["pixel_passes"]), raw=rec.get().tobytes())


def random_state(rows, width, seed, max_count=9, special=True):
    """A state with mixed counts (0 and 1 included where there is room), converged and noisy pixels,
    stale NaN bytes under the count-0 pixels and the header's special values."""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, max_count + 1, (rows, width)).astype(np.int32)
    mean = rng.random((rows, width, 3))
    scale = np.where(rng.random((rows, width, 1)) < 0.5, 1e-6, 0.05)  # half the pixels converge easily
    m2 = scale * rng.random((rows, width, 3)) * (count * np.maximum(count - 1, 0))[..., None]
    mean[count == 0] = NAN
    m2[count == 0] = NAN
    if special and rows * width >= 40:
        fm, f2 = mean.reshape(-1, 3), m2.reshape(-1, 3)
        n = len(fm)
        f2[3 % n, 1], f2[11 % n, 0], f2[17 % n, 2], fm[23 % n, 0], fm[29 % n, 2] = NAN, INF, -1.0, NAN, INF
        fm[31 % n] = 0.0  # a black pixel: measured against the floor
    return mean, m2, count


def test_sparse_fold_full_list_equals_the_uniform_fold(L, torch):
    rows, width = 23, 37
    rng = np.random.default_rng(1)
    first, more = rng.random((3, rows, width, 3)), rng.random((4, rows, width, 3))
    more[1, 2, 3, 1], more[2, 5, 5, 0] = NAN, INF
    f = Fold(L, torch, rows, width, variance=False, metric=False)
    f.fold(first)
    mean, m2, n = f.state()
    s = State(L, torch, mean, m2, np.full((rows, width), n, np.int32))
    s.fold(np.arange(rows * width), more.reshape(4, -1, 3))
    f.fold(more)
    want = f.state()
    got = s.get()
    assert_same_bits(got[0], want[0], "full list: mean")
    assert_same_bits(got[1], want[1], "full list: m2")
    assert (got[2] == 7).all() and want[2] == 7


@pytest.mark.parametrize("rows,width,k", [(1, 1, 1), (17, 33, 1), (17, 33, 5), (65, 129, 3)])
def test_sparse_fold_scattered_list_and_mixed_counts(L, torch, rows, width, k):
    """The special values arrive as samples (a NaN and an infinity in `values`) and as the stale NaN
    bytes under the count-0 pixels. The states of the counted pixels are finite: `x - mean` with a
    NaN mean is a NaN whose sign no IEEE rule fixes (the device subtracts by adding the negated
    operand and returns it with its sign flipped, numpy on x86 returns it as it is), so that bit
    pattern is not the header's to promise."""
    mean, m2, count = random_state(rows, width, seed=rows + k, special=False)
    rng = np.random.default_rng(k)
    n = rows * width
    lst = rng.permutation(n)[: max(1, n // 3)]  # distinct, scattered, unordered
    assert n < 40 or ((count.reshape(-1)[lst] == 0).any() and (count.reshape(-1)[lst] > 1).any())
    lst = np.concatenate([lst, [n, 2 ** 32 - 1]]) if n > 1 else lst  # and two entries outside the image
    values = rng.random((k, len(lst), 3))
    if n >= 40:
        values[0, 1, 2], values[k - 1, 2, 0] = NAN, -INF
    s = State(L, torch, mean, m2, count)
    s.fold(lst, values)
    got, want = s.get(), A.fold_sparse(mean, m2, count, lst, values)
    assert_same_bits(got[0], want[0], "scattered list: mean")
    assert_same_bits(got[1], want[1], "scattered list: m2")
    assert np.array_equal(got[2], want[2])
    untouched = np.ones(n, dtype=bool)
    untouched[lst[lst < n]] = False
    assert np.array_equal(bits(got[0].reshape(-1, 3)[untouched]), bits(mean.reshape(-1, 3)[untouched]))
    assert np.array_equal(bits(got[1].reshape(-1, 3)[untouched]), bits(m2.reshape(-1, 3)[untouched]))
    assert np.array_equal(got[2].reshape(-1)[untouched], count.reshape(-1)[untouched])
    listed = lst[lst < n]
    assert np.isfinite(got[0].reshape(-1, 3)[listed[count.reshape(-1)[listed] == 0]]).any() or n < 40


# ---------------------------------------------------------------- 3. the selection --
# 1x1; 1x70 (a tail inside one wave's 128 pixels); 33x17 = 561 (a second workgroup of the metric
# pass, one block total); 129x65 = 8385 (17 metric workgroups, 9 block totals: the scan matters).
SELECT_SHAPES = [(1, 1), (1, 70), (17, 33), (65, 129)]


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("rows,width", SELECT_SHAPES)
def test_select_equals_the_restatement(L, torch, rows, width, dilate):
    mean, m2, count = random_state(rows, width, seed=7 * rows + width)
    s = State(L, torch, mean, m2, count)
    for kw in (dict(min_passes=3, max_passes=8), dict(min_passes=1, max_passes=64, tolerance=0.2),
               dict(min_passes=2, max_passes=2 ** 30, tolerance=0.0)):
        got = s.select(dilate=dilate, **kw)
        want = A.select(mean, m2, count, dilate=dilate, **kw)
        what = f"{width}x{rows} dilate {dilate} {kw}"
        assert_same_bits(got["variance"], want["variance"], what + ": variance")
        assert np.array_equal(got["pixels"], want["pixels"]), what
        assert (got["n_active"], got["unconverged"], got["pixel_passes"]) == \
            (want["n_active"], want["unconverged"], want["pixel_passes"]), what
        assert bits(np.float64(got["max_ratio"])) == bits(np.float64(want["max_ratio"])), what
        again = s.select(dilate=dilate, **kw)
        assert again["raw"] == got["raw"] and np.array_equal(again["pixels"], got["pixels"]), what + ": a second run"
        none = s.select(variance=False, dilate=dilate, **kw)  # without the variance plane: the same
        assert none["raw"] == got["raw"] and np.array_equal(none["pixels"], got["pixels"])
    after = s.get()
    assert np.array_equal(bits(after[0]), bits(mean)) and np.array_equal(bits(after[1]), bits(m2))
    assert np.array_equal(after[2], count)
    if rows * width >= 500:  # the case proves what it says
        w0 = A.select(mean, m2, count, dilate=0, min_passes=3, max_passes=8)
        w1 = A.select(mean, m2, count, dilate=1, min_passes=3, max_passes=8)
        assert 0 < w0["n_active"] < w1["n_active"] < rows * width and w0["unconverged"] > w0["n_active"]


@pytest.mark.parametrize("n", [1, 2, 5])
def test_select_record_with_uniform_counts_is_the_progressive_record(L, torch, n):
    rows, width = 23, 37
    rng = np.random.default_rng(n)
    frames = 0.5 + 0.05 * rng.normal(size=(n, rows, width, 3)) * rng.random((rows, width, 1))
    frames[0, 3, 3, 1] = NAN
    f = Fold(L, torch, rows, width)
    f.fold(frames)
    mean, m2, _ = f.state()
    s = State(L, torch, mean, m2, np.full((rows, width), n, np.int32))
    for min_passes in (1, 2):
        got = s.select(min_passes=min_passes, dilate=0)
        assert (got["unconverged"], bits(np.float64(got["max_ratio"]))) == \
            (f.metric()[0], bits(np.float64(f.metric()[1]))), (n, min_passes)
        assert_same_bits(got["variance"], f.variance.get((rows, width, 3)), "variance")
        assert got["pixel_passes"] == n * rows * width
    assert 0 < f.metric()[0] < rows * width or n == 1


# ------------------------------------------------ 4. the invariant of the whole loop --
def test_render_adaptive_pixels_hold_the_uniform_state_of_their_counts(L, torch, rich2, dev_book):
    """48 x 27, r = 4, max_passes 12: every pixel's mean and variance are those of the uniform
    ordered-sum passes 0 .. counts[p] - 1 (tray_render_passes_async frames, folded and gathered by
    count); with tolerance 0 every pixel runs to max_passes and `linear` is Accumulate's mean."""
    w, h, r, max_passes, batch, min_passes = 48, 27, 4, 12, 4, 3
    ray, t = _tracer(w, h, r)
    scene = ray.Scene.from_array(rich2)
    st = camera(L, RICH_SETUP, w, h)
    p = L.make_params(w, h, 50, r, 0.5, 2, flags=L.FLAG_ORDERED_SUM)
    top = max_passes + batch - 1
    frames = torch.full((top, h, w, 3), NAN, dtype=torch.float64, device="cuda")
    dev_book.render_passes_async(st, p, top, frames.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    frames = frames.cpu().numpy()
    states = {c: R.fold(None, frames[:c]) for c in range(1, top + 1)}
    img = t.RenderAdaptive(scene, max_passes, min_passes=min_passes, batch=batch, tolerance=0.3).copy()
    counts = t.counts
    assert counts.shape == (h, w) and counts.dtype == np.int32
    assert counts.min() >= min_passes and counts.max() <= max_passes + batch - 1
    assert len(np.unique(counts)) > 1 and t.passes == counts.max() and t.pixel_passes == int(counts.sum())
    assert t.pixel_passes < h * w * max_passes and t.seed == 2
    mean, var = np.empty((h, w, 3)), np.empty((h, w, 3))
    for c in np.unique(counts):
        mean[counts == c] = states[c][0][counts == c]
        var[counts == c] = R.variance_of_mean(states[c][1], c)[counts == c]
    assert_same_bits(t.linear, mean, "RenderAdaptive: the mean after counts[p] uniform passes")
    assert_same_bits(t.variance, var, "RenderAdaptive: the variance after counts[p] uniform passes")
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    L.check(L.lib().tray_to_srgba(np.ascontiguousarray(mean).ctypes.data, h * w, rgba.ctypes.data))
    assert np.array_equal(img, rgba)
    # tolerance 0: nothing with noise converges; every count reaches max_passes (12 = 3 + 4 + 4 + 1
    # does not divide: the last round overshoots, by less than a batch)
    t.RenderAdaptive(scene, max_passes, min_passes=4, batch=4, tolerance=0.0)
    noisy = (R.variance_of_mean(states[4][1], 4).sum(-1) > 0)
    assert (t.counts[noisy] == max_passes).all() and t.passes == max_passes
    acc_mean, _ = t.Accumulate(frames[:max_passes])
    assert_same_bits(t.linear[noisy], acc_mean[noisy], "tolerance 0: linear is Accumulate of the 12 frames")
    # denoise=True filters the same mean
    plain = t.linear.copy()
    t.RenderAdaptive(scene, max_passes, min_passes=4, batch=4, tolerance=0.0, denoise=True)
    assert np.isfinite(t.linear).all() and not np.array_equal(t.linear, plain)


# ------------------------------------- 4b. the filter and the guides behind the Tracer --
PINNED = dict(max_passes=8, min_passes=4, batch=4, tolerance=0.0)  # 48 x 27, r = 4, seed 2


def srgba(L, linear):
    linear = np.ascontiguousarray(linear)
    out = np.zeros(linear.shape[:2] + (4,), dtype=np.uint8)
    L.check(L.lib().tray_to_srgba(linear.ctypes.data, linear.shape[0] * linear.shape[1], out.ctypes.data))
    return out


@pytest.fixture(scope="module")
def unfiltered(L, torch, rich2):
    """RenderAdaptive and RenderProgressive without the filter, and RenderAOV's buffers: what the
    filtered calls below must be the composition of. Computed once and left unchanged."""
    ray, t = _tracer(48, 27, 4)
    scene = ray.Scene.from_array(rich2)
    t.RenderAdaptive(scene, **PINNED)
    adaptive = (t.linear.copy(), t.variance.copy())
    t.RenderProgressive(scene, 4, batch=4, tolerance=0.0)
    progressive = (t.linear.copy(), t.variance.copy())
    aov = t.RenderAOV(scene)
    assert np.isfinite(adaptive[1]).all() and np.isfinite(progressive[1]).all()
    return dict(scene=scene, adaptive=adaptive, progressive=progressive,
                guides={k: aov[k] for k in ("albedo", "normal", "depth")})


def test_render_adaptive_denoised_equals_the_composition(L, torch, unfiltered):
    """RenderAdaptive(denoise=True) is tray_denoise_variance_async over the `linear` and `variance` of
    the same call without the filter, guided by RenderAOV's buffers, then tray_to_srgba: bit for bit,
    with the tracer's own guides, with the caller's, and with an override."""
    mean, variance = unfiltered["adaptive"]
    g = unfiltered["guides"]
    want, _ = device_filter(L, torch, mean, variance, g["albedo"], g["normal"], g["depth"])
    assert not np.array_equal(want, mean)
    _, t = _tracer(48, 27, 4)
    got = t.RenderAdaptive(unfiltered["scene"], denoise=True, **PINNED).copy()
    assert_same_bits(t.linear, want, "RenderAdaptive(denoise=True): linear")
    assert_same_bits(t.variance, variance, "RenderAdaptive(denoise=True): variance")
    assert np.array_equal(got, srgba(L, want))
    again = t.RenderAdaptive(unfiltered["scene"], denoise=True, guides=g, **PINNED)
    assert np.array_equal(again, got)
    assert_same_bits(t.linear, want, "RenderAdaptive(guides=RenderAOV's): linear")
    half = L.denoise_variance_params(48, 27).sigma_variance / 2
    other, _ = device_filter(L, torch, mean, variance, g["albedo"], g["normal"], g["depth"], sigma_variance=half)
    t.RenderAdaptive(unfiltered["scene"], denoise=True, sigma_variance=half, **PINNED)
    assert_same_bits(t.linear, other, "RenderAdaptive(sigma_variance=half the default): linear")
    assert np.array_equal(t.imageData, srgba(L, other))
    assert not np.array_equal(bits(other), bits(want))


def test_guides_without_depth_give_the_c_call_with_a_null_depth(L, torch, unfiltered):
    g = {k: unfiltered["guides"][k] for k in ("albedo", "normal")}
    _, t = _tracer(48, 27, 4)
    mean, variance = unfiltered["adaptive"]
    assert_same_bits(t.Denoise(mean, g), device_denoise(L, torch, mean, g["albedo"], g["normal"], None),
                     "Denoise without depth")
    want, _ = device_filter(L, torch, mean, variance, g["albedo"], g["normal"], None)
    full, _ = device_filter(L, torch, mean, variance, **unfiltered["guides"])
    assert not np.array_equal(bits(want), bits(full))  # the depth term matters here
    t.RenderAdaptive(unfiltered["scene"], denoise=True, guides=g, **PINNED)
    assert_same_bits(t.linear, want, "RenderAdaptive without depth")
    assert np.array_equal(t.imageData, srgba(L, want))
    mean, variance = unfiltered["progressive"]
    want, _ = device_filter(L, torch, mean, variance, g["albedo"], g["normal"], None)
    t.RenderProgressive(unfiltered["scene"], 4, batch=4, tolerance=0.0, denoise=True, guides=g)
    assert_same_bits(t.linear, want, "RenderProgressive without depth")
    assert np.array_equal(t.imageData, srgba(L, want))


def test_a_guide_of_the_wrong_shape_is_refused(L, torch, unfiltered):
    g = dict(unfiltered["guides"], albedo=np.zeros((27, 48)))
    _, t = _tracer(48, 27, 4)
    with pytest.raises(ValueError):
        t.Denoise(unfiltered["adaptive"][0], g)
    with pytest.raises(ValueError):
        t.RenderProgressive(unfiltered["scene"], 4, batch=4, tolerance=0.0, denoise=True, guides=g)
    with pytest.raises(ValueError):
        t.RenderAdaptive(unfiltered["scene"], denoise=True, guides=g, **PINNED)


# ------------------------------------------------------------------ 5. conditions --
def test_conditions_against_the_uniform_progressive_run(L, torch, rich2, dev_book):
    """160 x 90, r = 16, max_passes 32, default tolerance, same seed, against RenderProgressive.
    (a) adaptive spends fewer pixel-passes (structural: the sky converges early); (b) every pixel the
    final select calls converged satisfies the formula, recomputed in numpy; (c) MSE against the
    independent r = 4096 pass-1 target <= MSE_MARGIN x the uniform run's. The ratios are printed."""
    w, h, r, max_passes = 160, 90, 16, 32
    target, _ = book_frame(L, torch, dev_book, w, h, 4096, pass_=1, aov=False)
    mse = lambda a: float(np.mean((a - target) ** 2))  # noqa: E731
    ray, t = _tracer(w, h, r)
    scene = ray.Scene.from_array(rich2)
    t.RenderProgressive(scene, max_passes)
    uniform, uniform_passes = t.linear.copy(), t.passes
    t.RenderAdaptive(scene, max_passes)
    ap = L.adaptive_params()
    counts, var, mean = t.counts, t.variance, t.linear
    print(f"adaptive {t.pixel_passes} pixel-passes against uniform {h * w * uniform_passes} "
          f"(ratio {t.pixel_passes / (h * w * uniform_passes):.4f}); counts {counts.min()}..{counts.max()}; "
          f"unconverged {t.unconverged}; MSE adaptive {mse(mean):.6e}, uniform {mse(uniform):.6e} "
          f"(ratio {mse(mean) / mse(uniform):.4f}, margin {MSE_MARGIN})")
    assert t.pixel_passes < h * w * uniform_passes
    with np.errstate(all="ignore"):
        v = (var[..., 0] + var[..., 1]) + var[..., 2]
        e = (mean[..., 0] * mean[..., 0] + mean[..., 1] * mean[..., 1]) + mean[..., 2] * mean[..., 2]
        m = np.where(e > ap.floor, e, ap.floor)
        converged = (counts >= 2) & (counts >= ap.min_passes) & (v <= (ap.tolerance * ap.tolerance) * m)
    assert int((~converged).sum()) == t.unconverged
    assert (counts[~converged] >= max_passes).all()  # what is left unconverged ran out of passes
    assert mse(mean) <= MSE_MARGIN * mse(uniform)


# --------------------------------------------------------- 6. concurrency and CLI --
def test_two_loops_in_flight_on_two_streams_give_the_solo_bits(L, torch, dev_book):
    """One round of the loop (select, render the list, fold, select) for two different states,
    solo and then both in flight on two streams without a host wait in between."""
    w, h, r = 48, 27, 4
    st = camera(L, RICH_SETUP, w, h)
    p = L.make_params(w, h, 50, r, 0.5, 2)
    n = w * h

    def setup(k):
        frames = device_passes(L, torch, dev_book, w, h, r, 2 + k, first=0).cpu().numpy()
        mean, m2, c = R.fold(None, frames)
        s = State(L, torch, mean, m2, np.full((h, w), c, np.int32))
        s.ap = L.adaptive_params(min_passes=2, max_passes=8, tolerance=0.1 + 0.1 * k)
        s.list = torch.full((n,), 0, dtype=torch.int32, device="cuda")
        s.rec = torch.zeros((4,), dtype=torch.float64, device="cuda")
        s.nbytes = L.adaptive_workspace_bytes(w, h)
        s.work = torch.empty((s.nbytes // 8,), dtype=torch.float64, device="cuda")
        s.values = torch.full((2, n, 3), NAN, dtype=torch.float64, device="cuda")
        return s

    def enqueue(s, stream, n_active):
        L.adaptive_select_async(s.st, s.ap, s.list.data_ptr(), s.rec.data_ptr(), s.work.data_ptr(), s.nbytes, None, 0,
                                stream)
        dev_book.render_pixels_async(st, p, s.list.data_ptr(), n_active, s.values.data_ptr(), 2,
                                     pass_plane_ptr=s.count.data_ptr(), stream=stream)
        L.adaptive_fold_async(s.st, s.list.data_ptr(), n_active, s.values.data_ptr(), 2, 0, stream)
        L.adaptive_select_async(s.st, s.ap, s.list.data_ptr(), s.rec.data_ptr(), s.work.data_ptr(), s.nbytes, None, 0,
                                stream)

    def result(s):
        return tuple(a.tobytes() for a in s.get()) + (s.rec.cpu().numpy().tobytes(), s.list.cpu().numpy().tobytes())

    solo, actives = [], []
    for k in (0, 1):
        s = setup(k)
        actives.append(A.select(*s.get(), tolerance=s.ap.tolerance, min_passes=2, max_passes=8)["n_active"])
        enqueue(s, torch.cuda.current_stream().cuda_stream, actives[k])
        torch.cuda.synchronize()
        solo.append(result(s))
    assert 0 < actives[0] and 0 < actives[1] and solo[0] != solo[1]
    pair = [setup(0), setup(1)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for k in (0, 1):
        enqueue(pair[k], streams[k].cuda_stream, actives[k])
    torch.cuda.synchronize()
    assert [result(s) for s in pair] == solo


def test_cli_renders_adaptively(L, rich2, tmp_path):
    from tray_amd import png

    save = str(tmp_path / "frame.png")
    r = subprocess.run([sys.executable, "-m", "tray_amd", "-width", "48", "-height", "27", "-r", "4", "-d", "50",
                        "-passes", "12", "-adaptive", "-save", save], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ray, t = _tracer(48, 27, 4)  # the CLI's defaults: seed 2 for the scene and the draws
    want = t.RenderAdaptive(ray.RichScene(2), 12)
    assert f"adaptive: {t.pixel_passes} pixel-passes of r=4 against {48 * 27 * 12}" in r.stdout, r.stdout
    img = png.decode_png(open(save, "rb").read())
    assert img.shape == (27, 48, 4) and np.array_equal(img, want)
