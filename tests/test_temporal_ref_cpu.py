"""tests/temporal_ref.py, the numpy restatement of include/tray_temporal.h, on the oracle's
centre-ray hits: the properties the header states, on the default scene and a small book cover at
33 x 17. The GPU tests compare the device with this restatement bit for bit."""
import numpy as np
import pytest

import progressive_ref as P
import temporal_ref as R
from conftest import RICH_SETUP

W, H = 33, 17
DEFAULT_SETUP = np.array([-2.0, 2.0, 1.0, 0, 0, -1.0, 0, 1, 0, 20.0, 1.0, 12.0 ** 0.5, 0.1])  # tracer.go:52-58
NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module", params=["default", "book"])
def world(request, O):
    """(spheres, setup, camera, hits of the camera's centre rays): computed once per scene."""
    spheres, setup = (O.default_scene(), DEFAULT_SETUP) if request.param == "default" else \
        (O.rich_scene(2, 3), RICH_SETUP)
    cam = O.camera_initialize(setup, W, H)[1]
    return spheres, setup, cam, R.oracle_hits(O, spheres, cam, W, H)


def frames_of(k, seed=1):
    return np.random.default_rng(seed).random((k, H, W, 3))


def test_a_static_camera_snaps_every_pixel(world):
    _, _, cam, hits = world
    z, u, v, ok = R.project(cam, cam, W, H, *hits)
    assert (hits[0] >= 0).any() and (len(world[0]) == 5 or (hits[0] < 0).any())  # spheres, and sky on the book cover
    assert ok.all() and R.snapped_mask(u, v).all()
    err = max(np.abs(u - np.arange(W)[None, :]).max(), np.abs(v - np.arange(H)[:, None]).max())
    assert err < R.SNAP * 2.0 ** -10, err  # far below snap
    assert np.array_equal(np.floor(u + 0.5), np.broadcast_to(np.arange(W, dtype=float)[None, :], (H, W)))
    assert np.array_equal(np.floor(v + 0.5), np.broadcast_to(np.arange(H, dtype=float)[:, None], (H, W)))
    hit = hits[0] >= 0  # z is the root the previous centre ray would have had: the depth test passes
    assert (np.abs(hits[1][hit] - z[hit]) <= 1e-9 * z[hit]).all()


def test_static_steps_are_the_accumulators_fold_bit_for_bit(world):
    _, _, cam, hits = world
    frames = frames_of(5)
    state = None
    for k in range(5):
        state, (fresh, age_sum) = R.step(cam, cam, frames[k], hits, state)
        assert (fresh, age_sum) == ((W * H, W * H) if k == 0 else (0, (k + 1) * W * H))
        assert np.array_equal(bits(state["colour"]), bits(P.fold(None, frames[:k + 1])[0])), k
    assert (state["age"] == 5).all()
    assert np.array_equal(state["index"], hits[0])
    assert np.array_equal(bits(state["depth"]), bits(np.where(hits[0] >= 0, hits[1], np.inf)))


@pytest.mark.parametrize("cause", ["behind", "aside"])
def test_a_camera_turned_away_gives_all_fresh_pixels(world, O, cause):
    """Two causes: the old camera looked the other way (z <= 0), or aside by more than the field
    of view (z > 0, u or v out of range)."""
    spheres, setup, cam, hits = world
    prev_setup = np.array(setup, dtype=np.float64)
    to = prev_setup[3:6] - prev_setup[0:3]
    if cause == "behind":
        prev_setup[3:6] = prev_setup[0:3] - to
    else:  # turn the view direction by 80 degrees about +y
        c, s = np.cos(np.radians(80.0)), np.sin(np.radians(80.0))
        prev_setup[3:6] = prev_setup[0:3] + np.array([c * to[0] + s * to[2], to[1], -s * to[0] + c * to[2]])
    prev = O.camera_initialize(prev_setup, W, H)[1]
    z, u, v, ok = R.project(cam, prev, W, H, *hits)
    assert not ok.any()
    if cause == "behind":
        assert (z <= 0).all()
    else:
        assert (z > 0).any() and not ((u > -1) & (u < W) & (v > -1) & (v < H) & (z > 0)).any()
    frame = frames_of(1)[0]
    history, _ = R.step(prev, None, frames_of(1, 2)[0], R.oracle_hits(O, spheres, prev, W, H))
    state, rec = R.step(cam, prev, frame, hits, history)
    assert np.array_equal(bits(state["colour"]), bits(frame)) and (state["age"] == 1).all()
    assert rec == (W * H, W * H)


def orbit_pair(world, O, degrees=1.0):
    spheres, setup, cam, hits = world
    prev = O.camera_initialize(R.orbit_setup(setup, -degrees), W, H)[1]
    return prev, R.oracle_hits(O, spheres, prev, W, H)


def test_max_history_1_returns_the_frame(world, O):
    _, _, cam, hits = world
    prev, prev_hits = orbit_pair(world, O)
    history, _ = R.step(prev, None, frames_of(1, 2)[0], prev_hits)
    frame = frames_of(1)[0]
    state, rec = R.step(cam, prev, frame, hits, history, max_history=1)
    assert np.array_equal(bits(state["colour"]), bits(frame)) and (state["age"] == 1).all() and rec == (W * H, W * H)
    moved, rec = R.step(cam, prev, frame, hits, history)  # the same pair does fold with room for history
    assert 0 <= rec[0] < W * H and (moved["age"] == 2).any()


def test_nan_history_is_never_taken_and_a_nan_frame_pixel_stays_alone(world, O):
    _, _, cam, hits = world
    history, _ = R.step(cam, None, frames_of(1, 2)[0], hits)
    history["colour"][3, 4, 1] = NAN
    history["colour"][H - 1, W - 1] = NAN
    frame = frames_of(1)[0]
    frame[5, 6, 2] = NAN
    state, rec = R.step(cam, cam, frame, hits, history)
    nan = np.isnan(state["colour"])
    assert nan.sum() == 1 and nan[5, 6, 2]  # the frame's own NaN, alone
    for y, x in ((3, 4), (H - 1, W - 1)):  # the NaN history was refused: the pixel is fresh
        assert state["age"][y, x] == 1 and np.array_equal(bits(state["colour"][y, x]), bits(frame[y, x]))
    assert rec[0] == 2
    after, rec = R.step(cam, cam, frames_of(1, 3)[0], hits, state)  # the NaN lives for one frame
    assert not np.isnan(after["colour"]).any() and after["age"][5, 6] == 1 and rec[0] == 1
    # under a moving camera a NaN history pixel drops out of its neighbours' bilinear taps too
    prev, prev_hits = orbit_pair(world, O)
    history, _ = R.step(prev, None, frames_of(1, 2)[0], prev_hits)
    history["colour"][H // 2, :, 0] = NAN
    state, _ = R.step(cam, prev, frames_of(1)[0], hits, history)
    assert not np.isnan(state["colour"]).any()


def test_ages_never_exceed_max_history_and_the_record_counts_the_planes(world, O):
    _, _, cam, hits = world
    prev, prev_hits = orbit_pair(world, O)
    rng = np.random.default_rng(4)
    history, _ = R.step(prev, None, frames_of(1, 2)[0], prev_hits)
    history["age"] = rng.integers(0, 40, size=(H, W)).astype(np.int32)
    for cap in (2, 7, 32):
        state, (fresh, age_sum) = R.step(cam, prev, frames_of(1)[0], hits, history, max_history=cap)
        assert state["age"].min() >= 1 and state["age"].max() <= cap
        assert fresh == int((state["age"] == 1).sum()) and age_sum == int(state["age"].sum())
        assert fresh < W * H  # history survives
