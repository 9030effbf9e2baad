"""tests/temporal_variance_ref.py, the numpy restatement of include/tray_temporal_variance.h, on the
oracle's centre-ray hits: the properties the header states, on the default scene and a small book
cover at 33 x 17. The GPU tests compare the device with this restatement bit for bit."""
import numpy as np
import pytest

import adaptive_ref as A
import progressive_ref as P
import temporal_ref as R
import temporal_variance_ref as V
from conftest import RICH_SETUP

W, H = 33, 17
DEFAULT_SETUP = np.array([-2.0, 2.0, 1.0, 0, 0, -1.0, 0, 1, 0, 20.0, 1.0, 12.0 ** 0.5, 0.1])  # tracer.go:52-58
NAN, INF = float("nan"), float("inf")
f8 = np.float64


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


def moved_setup(setup, which, k=1):
    s = np.array(setup, dtype=f8)
    if which == "orbit":
        return R.orbit_setup(setup, 1.0 * k)
    s[0:3] = s[0:3] + 0.1 * k * (s[3:6] - s[0:3])  # a dolly towards look_at
    return s


def plain(state):
    return {n: state[n] for n in ("colour", "age", "index", "depth")}


@pytest.mark.parametrize("which", ["orbit", "dolly"])
def test_colour_age_index_depth_are_the_plain_steps_bits(world, O, which):
    """Three chained steps: everything tray_temporal.h defines is untouched by the M2 that rides along,
    whatever that M2 holds (random, infinite and NaN values are mixed into the first history)."""
    spheres, setup, _, _ = world
    cams = [O.camera_initialize(moved_setup(setup, which, k), W, H)[1] for k in range(4)]
    hits = [R.oracle_hits(O, spheres, c, W, H) for c in cams]
    frames = frames_of(4)
    want, _ = R.step(cams[0], None, frames[0], hits[0])
    got, var, _ = V.step(cams[0], None, frames[0], hits[0])
    assert (got["m2"] == 0).all() and not np.signbit(got["m2"]).any() and np.isinf(var).all()
    rng = np.random.default_rng(3)
    got["m2"] = rng.random((H, W, 3))
    got["m2"][1, 2] = (INF, NAN, -INF)
    want["age"] = got["age"] = rng.integers(0, 9, size=(H, W)).astype(np.int32)
    bilinear, fresh = 0, []
    for k in range(1, 4):
        want, want_rec = R.step(cams[k], cams[k - 1], frames[k], hits[k], want, max_history=6)
        got, var, rec = V.step(cams[k], cams[k - 1], frames[k], hits[k], got, max_history=6)
        assert rec == want_rec
        for name in ("age", "index"):
            assert np.array_equal(got[name], want[name]), (k, name)
        for name in ("colour", "depth"):
            assert np.array_equal(bits(got[name]), bits(want[name])), (k, name)
        assert np.array_equal(bits(var), bits(A.variance(got["m2"], got["age"]))), k
        z, u, v, ok = R.project(cams[k], cams[k - 1], W, H, *hits[k])
        bilinear += int((ok & ~R.snapped_mask(u, v)).sum())
        fresh.append(rec[0])
    assert bilinear > 0 and 0 < fresh[0] < W * H and max(fresh) < W * H, fresh  # both paths of the fold


def test_static_steps_are_the_accumulators_m2_and_variance_bit_for_bit(world):
    _, _, cam, hits = world
    frames = frames_of(5)
    state = None
    for k in range(5):
        state, var, rec = V.step(cam, cam, frames[k], hits, state)
        mean, m2, n = P.fold(None, frames[:k + 1])
        assert rec == ((W * H, W * H) if k == 0 else (0, (k + 1) * W * H))
        assert np.array_equal(bits(state["colour"]), bits(mean)), k
        assert np.array_equal(bits(state["m2"]), bits(m2)), k
        assert np.array_equal(bits(var), bits(P.variance_of_mean(m2, n))), k
    assert (state["age"] == 5).all() and (state["m2"] > 0).all()


def scalar_cap_chain(xs, max_history):
    """One channel of one pixel under a static camera, straight from the header's sections 2a-2c:
    (colour, m2, age) after folding xs in order."""
    c, m2, age = f8(xs[0]), f8(0.0), 1
    for x in xs[1:]:
        x = f8(x)
        Wt = f8(0.0) + f8(1.0)
        h = (f8(0.0) + f8(1.0) * c) / Wt
        m = (f8(0.0) + f8(1.0) * m2) / Wt
        k = min(age, max_history - 1) + 1
        n0 = k - 1
        if age > n0:
            m = m * (f8(n0 - 1) / f8(age - 1))
        t = x - h
        c = h + t / f8(k)
        m2 = m + t * (x - c)
        age = k
    return c, m2, age


def test_the_cap_scales_m2_by_the_sample_variance_rule(world):
    """max_history = 4 over 8 static frames: the age stops at 4 and from then on the history's m2 is
    scaled by (n0 - 1) / (A - 1) = 2 / 3 before the fold, which keeps m2 / (n - 1): a direct scalar
    re-computation of one pixel agrees bit for bit, and the scaling is really taken."""
    _, _, cam, hits = world
    frames = frames_of(8)
    state = None
    for k in range(8):
        state, var, _ = V.step(cam, cam, frames[k], hits, state, max_history=4)
        assert (state["age"] == min(k + 1, 4)).all()
    for y, x, ch in ((0, 0, 0), (H // 2, W // 2, 1), (H - 1, W - 1, 2)):
        c, m2, age = scalar_cap_chain(frames[:, y, x, ch], 4)
        assert age == 4
        assert bits(state["colour"][y, x, ch]) == bits(c) and bits(state["m2"][y, x, ch]) == bits(m2)
        assert bits(var[y, x, ch]) == bits(m2 / (f8(4) * f8(3)))
    uncapped = None
    for k in range(8):
        uncapped, _, _ = V.step(cam, cam, frames[k], hits, uncapped, max_history=32)
    assert (state["m2"] < uncapped["m2"]).all()


def test_max_history_2_builds_m2_from_a_zeroed_history(world):
    """n0 = 1: the history counts as one sample, whose m2 is 0 whatever it held (A > 1), or is kept
    (A = 1, where it is 0 already): out.m2 = 0 * m + t * (X - out.colour)."""
    _, _, cam, hits = world
    frames = frames_of(4)
    state = None
    for k in range(4):
        prev = state
        state, var, _ = V.step(cam, cam, frames[k], hits, state, max_history=2)
        if prev is not None:
            t = frames[k] - prev["colour"]
            want = t * (frames[k] - state["colour"])
            if k >= 2:
                want = prev["m2"] * f8(0.0) + want
            else:
                want = prev["m2"] + want
            assert np.array_equal(bits(state["m2"]), bits(want)), k
            assert (state["age"] == 2).all() and np.array_equal(bits(var), bits(state["m2"] / (f8(2) * f8(1))))
    c, m2, age = scalar_cap_chain(frames[:, 2, 3, 1], 2)
    assert age == 2 and bits(state["m2"][2, 3, 1]) == bits(m2)


def test_an_age_past_max_history_after_a_refill_is_scaled_too(world):
    """A refill folds passes into the state from outside the step, so A may exceed max_history: with
    max_history = 4 and A = 7 the step folds at k = 4 and scales m by (3 - 1) / (7 - 1)."""
    _, _, cam, hits = world
    frames = frames_of(3)
    state, _, _ = V.step(cam, None, frames[0], hits)
    state, _, _ = V.step(cam, cam, frames[1], hits, state)
    state["age"][:] = 7  # as after a refill of 5 passes
    state["m2"] = np.random.default_rng(8).random((H, W, 3))
    out, var, rec = V.step(cam, cam, frames[2], hits, state, max_history=4)
    assert (out["age"] == 4).all() and rec == (0, 4 * W * H)
    m = (0.0 + 1.0 * state["m2"]) / (0.0 + 1.0) * (f8(2) / f8(6))
    t = frames[2] - state["colour"]
    colour = state["colour"] + t / f8(4)
    assert np.array_equal(bits(out["colour"]), bits(colour))
    assert np.array_equal(bits(out["m2"]), bits(m + t * (frames[2] - colour)))
    assert np.array_equal(bits(var), bits(out["m2"] / (f8(4) * f8(3))))


def test_fresh_pixels_have_m2_zero_and_infinite_variance(world, O):
    spheres, setup, cam, hits = world
    prev = O.camera_initialize(R.orbit_setup(setup, -1.0), W, H)[1]
    history, _, _ = V.step(prev, None, frames_of(1, 2)[0], R.oracle_hits(O, spheres, prev, W, H))
    history["m2"] = np.random.default_rng(6).random((H, W, 3))
    history["age"][:, ::3] = 0  # pixels without history: their neighbours lose taps, some pixels every tap
    for kw in (dict(), dict(max_history=1)):
        state, var, rec = V.step(cam, prev, frames_of(1)[0], hits, history, **kw)
        fresh = state["age"] == 1
        assert rec[0] == int(fresh.sum()) > 0
        assert (state["m2"][fresh] == 0).all() and not np.signbit(state["m2"][fresh]).any()
        assert np.isposinf(var[fresh]).all() and np.isfinite(var[~fresh]).all()
        assert fresh.all() == bool(kw)
    first, var, rec = V.step(cam, None, frames_of(1)[0], hits)
    assert rec == (W * H, W * H) and (first["m2"] == 0).all() and np.isposinf(var).all()


def test_nan_and_infinite_values_stay_in_their_own_pixel(world):
    """A NaN or infinite frame value reaches its own colour and m2 only; an infinite or NaN m2 in the
    history travels with its colour into the pixels that take it and decides nothing."""
    _, _, cam, hits = world
    history, _, _ = V.step(cam, None, frames_of(1, 2)[0], hits)
    history, _, _ = V.step(cam, cam, frames_of(1, 3)[0], hits, history)
    history["m2"][3, 4] = (INF, NAN, 0.5)
    frame = frames_of(1)[0]
    frame[5, 6, 2] = NAN
    frame[7, 8, 0] = INF
    state, var, rec = V.step(cam, cam, frame, hits, history)
    clean, clean_var, clean_rec = V.step(cam, cam, frames_of(1)[0], hits, dict(history, m2=np.zeros((H, W, 3))))
    assert rec == clean_rec == (0, 3 * W * H)  # M2 decides nothing: no pixel is fresh
    odd = ~np.isfinite(state["m2"])
    want = np.zeros((H, W, 3), dtype=bool)
    want[3, 4, 0] = want[3, 4, 1] = want[5, 6, 2] = want[7, 8, 0] = True
    assert np.array_equal(odd, want)
    assert np.isposinf(state["m2"][3, 4, 0]) and np.isnan(state["m2"][3, 4, 1]) and np.isnan(state["m2"][5, 6, 2])
    assert np.array_equal(~np.isfinite(var), want)
    assert np.array_equal(np.isnan(state["colour"]), np.isnan(frame))
    # the next step refuses the NaN colour (that pixel is fresh, m2 0.0) and carries the infinite m2 on
    after, _, rec = V.step(cam, cam, frames_of(1, 4)[0], hits, state)
    assert rec[0] == 1 and after["age"][5, 6] == 1 and (after["m2"][5, 6] == 0).all()
    assert np.isposinf(after["m2"][3, 4, 0]) and np.isnan(after["m2"][3, 4, 1])


def test_list_variance_and_the_refill_chain(world, O):
    """Sections 3 and 4 on the restatements: after one orbit step the selection with min_passes 1 + R
    lists the pixels younger than 1 + R and their neighbours and nothing else; the fold moves exactly
    those; the list's variance refresh equals a whole-frame recomputation."""
    spheres, setup, cam, hits = world
    Rf = 3
    prev = O.camera_initialize(R.orbit_setup(setup, -1.0), W, H)[1]
    state = None
    for k in range(5):
        state, _, _ = V.step(prev, prev, frames_of(1, 10 + k)[0], R.oracle_hits(O, spheres, prev, W, H) if k == 0
                             else prev_hits, state)
        prev_hits = (state["index"], state["depth"])
    state["age"][4:7, 5:9] = 2  # a patch that was fresh two frames ago,
    state["age"][10:14, 18:22] = 0  # and a block without history: its inner pixels are fresh in the next step
    state, var, rec = V.step(cam, prev, frames_of(1)[0], hits, state)
    sel = V.refill_list(state, Rf, V.MAX_HISTORY)
    young = state["age"] < 1 + Rf
    assert 0 < rec[0] < young.sum() < W * H and (state["age"][young] > 1).any()
    assert np.array_equal(sel["needs"], young)  # the tolerance is out of the way: only the count decides
    grown = np.zeros((H + 2, W + 2), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            grown[dy:dy + H, dx:dx + W] |= young
    assert np.array_equal(sel["active"], grown[1:-1, 1:-1]) and sel["n_active"] == len(sel["pixels"])
    values = np.random.default_rng(12).random((Rf, sel["n_active"], 3))
    pixels = np.concatenate([sel["pixels"], [W * H, 2 ** 32 - 1]])  # bad entries are skipped
    filled = V.refill_fold(state, pixels, np.concatenate([values, np.zeros((Rf, 2, 3))], axis=1))
    listed = sel["active"]
    assert np.array_equal(filled["age"], state["age"] + Rf * listed)
    for name in ("colour", "m2"):
        assert np.array_equal(bits(filled[name])[~listed], bits(state[name])[~listed])
        assert (bits(filled[name])[listed] != bits(state[name])[listed]).any()
    stale = var.copy()
    fresh_var = V.list_variance(filled, pixels, stale)
    assert np.array_equal(bits(fresh_var), bits(V.list_variance(filled, None, None)))
    assert np.array_equal(bits(fresh_var), bits(A.variance(filled["m2"], filled["age"])))
    assert np.array_equal(bits(stale), bits(var)) and np.isfinite(fresh_var[listed]).all()
