"""tests/adaptive_ref.py, the numpy restatement of include/tray_adaptive.h sections 3 and 4,
checked on the CPU: against progressive_ref on uniform counts, and on hand-made 5 x 4 states for
what the header adds (per-pixel counts, min and max passes, dilation, the list, the record)."""
import numpy as np
import pytest

import adaptive_ref as A
import progressive_ref as P

ROWS, W = 4, 5
INF, NAN = float("inf"), float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def quiet_state(n=4, rows=ROWS, width=W):
    """Every pixel converged at the default tolerance: mean 0.5, variance of the mean 1e-8."""
    mean = np.full((rows, width, 3), 0.5)
    m2 = np.full((rows, width, 3), 1e-8 * n * (n - 1))
    return mean, m2, np.full((rows, width), n, dtype=np.int32)


def noisy(m2, count, y, x):
    """Makes pixel (y, x) unconverged: a relative standard error of about 1."""
    n = int(count[y, x])
    m2[y, x] = 0.25 * n * (n - 1)


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_uniform_counts_are_progressive_ref(n):
    rng = np.random.default_rng(n)
    frames = rng.random((n, 6, 7, 3))
    mean, m2, cnt = P.fold(None, frames)
    s = A.select(mean, m2, np.full((6, 7), n, np.int32), min_passes=1, max_passes=64, dilate=0)
    unconverged, max_ratio, converged = P.metric(mean, m2, n)
    assert s["unconverged"] == unconverged and bits(s["max_ratio"]) == bits(max_ratio)
    assert np.array_equal(s["needs"], ~converged)
    assert np.array_equal(bits(s["variance"]), bits(P.variance_of_mean(m2, n)))
    assert s["pixel_passes"] == n * 42
    # min_passes 2 changes nothing (n >= 2 is in the metric already); the full list folds like P.fold
    assert A.select(mean, m2, np.full((6, 7), n, np.int32), min_passes=2, dilate=0)["unconverged"] == unconverged
    more = rng.random((3, 42, 3))
    fm, f2, fc = A.fold_sparse(mean, m2, np.full((6, 7), n, np.int32), np.arange(42), more)
    pm, p2, pc = P.fold((mean, m2, n), more.reshape(3, 6, 7, 3))
    assert np.array_equal(bits(fm), bits(pm)) and np.array_equal(bits(f2), bits(p2)) and (fc == pc).all()


@pytest.mark.parametrize("y,x,expect", [
    (0, 0, [(0, 0), (0, 1), (1, 0), (1, 1)]),                           # a corner: 4 pixels
    (3, 4, [(2, 3), (2, 4), (3, 3), (3, 4)]),
    (0, 2, [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)]),            # an edge: 6
    (2, 0, [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)]),
    (1, 4, [(0, 3), (0, 4), (1, 3), (1, 4), (2, 3), (2, 4)]),            # the right edge does not wrap to column 0
    (2, 2, [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3)]),
])
def test_dilation_at_corners_and_edges(y, x, expect):
    mean, m2, count = quiet_state()
    noisy(m2, count, y, x)
    s = A.select(mean, m2, count, min_passes=2, dilate=1)
    assert s["unconverged"] == 1 and s["needs"][y, x] and s["needs"].sum() == 1
    assert s["pixels"].tolist() == sorted(yy * W + xx for yy, xx in expect) and s["n_active"] == len(expect)
    assert s["pixels"].dtype == np.uint32
    s0 = A.select(mean, m2, count, min_passes=2, dilate=0)
    assert s0["pixels"].tolist() == [y * W + x] and s0["unconverged"] == 1


def test_min_and_max_passes():
    mean, m2, count = quiet_state(4)
    assert A.select(mean, m2, count, min_passes=4)["n_active"] == 0
    s = A.select(mean, m2, count, min_passes=5)  # converged by the metric, but below min_passes
    assert s["unconverged"] == s["n_active"] == ROWS * W
    count[1, 1] = 5
    m2[1, 1] = 1e-8 * 20
    s = A.select(mean, m2, count, min_passes=5, dilate=0)
    assert s["n_active"] == ROWS * W - 1 and 1 * W + 1 not in s["pixels"].tolist()
    # max_passes: a pixel that needs more but has its passes is counted unconverged and not listed;
    mean, m2, count = quiet_state(4)
    noisy(m2, count, 2, 2)
    s = A.select(mean, m2, count, min_passes=2, max_passes=4, dilate=1)
    assert s["unconverged"] == 1 and s["n_active"] == 0 and s["wanted"].sum() == 9
    # its dilated neighbours with fewer passes still are
    count[2, 3] = 3
    m2[2, 3] = 1e-8 * 6
    s = A.select(mean, m2, count, min_passes=2, max_passes=4, dilate=1)
    assert s["pixels"].tolist() == [2 * W + 3] and s["unconverged"] == 1


def test_count_0_and_1_and_pixel_passes():
    mean, m2, count = quiet_state(4)
    count[0, 0], count[3, 4] = 0, 1
    mean[0, 0] = m2[0, 0] = NAN  # never folded: stale bytes
    s = A.select(mean, m2, count, min_passes=1, dilate=0)
    assert np.isposinf(s["variance"][0, 0]).all() and np.isposinf(s["variance"][3, 4]).all()
    assert s["pixels"].tolist() == [0, ROWS * W - 1] and s["unconverged"] == 2
    assert s["pixel_passes"] == 4 * (ROWS * W - 2) + 1
    # max_ratio: +inf counts (q >= 0); the NaN pixel's q is left out
    assert s["max_ratio"] == INF
    fm, f2, fc = A.fold_sparse(mean, m2, count, [0, 19, 7, 999], np.ones((2, 4, 3)))
    assert fc[0, 0] == 2 and fc[3, 4] == 3 and fc[1, 2] == 6 and fc.sum() == count.sum() + 6
    assert (fm[0, 0] == 1.0).all() and (f2[0, 0] == 0.0).all()  # started from zero, not from the NaN
    assert np.array_equal(bits(fm[2]), bits(mean[2])) and np.array_equal(bits(f2[2]), bits(m2[2]))  # untouched


@pytest.mark.parametrize("where,value,unconverged", [
    ("m2", NAN, 1),     # a NaN variance makes v <= T * m false
    ("m2", INF, 1),
    ("mean", NAN, 0),   # a NaN e is measured against the floor (tray_progressive.h): 3e-8 <= T * 2^-10
    ("mean", INF, 0),   # v <= T * inf
    ("m2", -1.0, 0),    # a negative variance compares as converged, as in tray_progressive.h
])
def test_nan_and_inf_follow_the_formula(where, value, unconverged):
    mean, m2, count = quiet_state(4)
    (m2 if where == "m2" else mean)[1, 2, 1] = value
    s = A.select(mean, m2, count, min_passes=2, dilate=0)
    assert s["unconverged"] == s["n_active"] == unconverged
    assert s["pixels"].tolist() == ([1 * W + 2] if unconverged else [])
    # a NaN or negative q is left out of the maximum; the NaN mean's q is measured against the floor
    expect = {("m2", INF): INF, ("mean", NAN): 3e-8 * 2 ** 10}.get((where, value), 3e-8 / 0.75)
    assert s["max_ratio"] == pytest.approx(expect, rel=1e-12)
    # a NaN state of a noisy pixel stays unconverged
    noisy(m2, count, 3, 3)
    mean[3, 3, 0] = NAN
    assert A.select(mean, m2, count, min_passes=2, dilate=0)["needs"][3, 3]


def test_list_is_ascending_and_distinct():
    rng = np.random.default_rng(5)
    mean = rng.random((9, 11, 3))
    m2 = rng.random((9, 11, 3)) * 0.05
    count = rng.integers(0, 9, (9, 11)).astype(np.int32)
    for dilate in (0, 1):
        s = A.select(mean, m2, count, min_passes=3, max_passes=7, dilate=dilate)
        p = s["pixels"].astype(np.int64)
        assert (np.diff(p) > 0).all() and s["n_active"] == p.size
        assert np.array_equal(p, np.flatnonzero(s["active"]))
        assert (count.reshape(-1)[p] < 7).all()
        assert s["pixel_passes"] == int(count.sum())
    assert set(A.select(mean, m2, count, 0.05, A.FLOOR, 3, 7, 0)["pixels"]) <= set(s["pixels"])
