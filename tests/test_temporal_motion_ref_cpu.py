"""tests/temporal_motion_ref.py, the numpy restatement of include/tray_temporal_motion.h, on the
oracle's centre-ray hits at 16 x 9: the two reductions to the static steps as bit patterns, what the
new target means (the previous camera's ray through (u, v) meets the previous sphere at Q'), that a
moved sphere leaves no ghost, and that a degenerate previous sphere makes its pixels fresh. The GPU
tests compare the device with this restatement bit for bit."""
import numpy as np
import pytest

import scene_update_cases as C
import temporal_motion_ref as M
import temporal_ref as R
import temporal_variance_ref as V
from conftest import RICH_SETUP

W, H = 16, 9
DEFAULT_SETUP = np.array([-2.0, 2.0, 1.0, 0, 0, -1.0, 0, 1, 0, 20.0, 1.0, 12.0 ** 0.5, 0.1])  # tracer.go:52-58
NAN, INF = float("nan"), float("inf")
f8 = np.float64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want, what):
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.dtype.kind == "f":
            assert ((bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))).all(), (what, name)
        else:
            assert np.array_equal(g, w), (what, name)


@pytest.fixture(scope="module", params=["default", "book"])
def world(request, O):
    spheres, setup = (O.default_scene(), DEFAULT_SETUP) if request.param == "default" else \
        (O.rich_scene(2, 3), RICH_SETUP)
    return request.param, spheres, setup


def history_of(rng, hits, m2):
    """A history over the given hits: random colours and ages, some pixels without history."""
    age = rng.integers(0, 9, size=(H, W)).astype(np.int32)
    state = dict(colour=rng.random((H, W, 3)), age=age, index=hits[0].copy(),
                 depth=np.where(hits[0] >= 0, hits[1], INF))
    if m2:
        state["m2"] = rng.random((H, W, 3))
    return state


@pytest.mark.parametrize("which", ["static", "orbit"])
def test_equal_geometries_reproduce_the_static_steps_bit_for_bit(world, O, which):
    """Section 3, the first reduction: prev_geometry equal to the scene's gives temporal_ref.step and
    temporal_variance_ref.step, every plane and the record."""
    _, spheres, setup = world
    prev = O.camera_initialize(setup, W, H)[1]
    cam = O.camera_initialize(R.orbit_setup(setup, 1.0) if which == "orbit" else setup, W, H)[1]
    hits, prev_hits = R.oracle_hits(O, spheres, cam, W, H), R.oracle_hits(O, spheres, prev, W, H)
    geo = C.geometry(spheres)
    frame = np.random.default_rng(1).random((H, W, 3))
    for m2 in (False, True):
        history = history_of(np.random.default_rng(2), prev_hits, m2)
        got, var, rec, motion = M.step(cam, prev, frame, hits, history, geo, geo.copy(), m2, max_history=6)
        if m2:
            want, want_var, want_rec = V.step(cam, prev, frame, hits, history, max_history=6)
            assert np.array_equal(bits(var), bits(want_var))
        else:
            want, want_rec = R.step(cam, prev, frame, hits, history, max_history=6)
            assert var is None
        same(got, want, (which, m2))
        assert set(got) == set(want) and rec == want_rec and 0 < rec[0] < W * H
        z, u, v, ok = R.project(cam, prev, W, H, *hits)
        assert np.array_equal(np.isnan(motion[..., 0]), ~ok) and np.array_equal(np.isnan(motion[..., 1]), ~ok)
        x, y = np.meshgrid(np.arange(W, dtype=f8), np.arange(H, dtype=f8))
        assert np.array_equal(bits(motion[ok]), bits(np.stack([u - x, v - y], axis=-1)[ok]))
        if which == "static":
            assert np.abs(motion[ok]).max() < R.SNAP
        first, _, first_rec, none = M.step(cam, None, frame, hits, None, geo, geo, m2)
        assert none is None and first_rec == (W * H, W * H)  # a null history writes no motion plane
        assert M.step(cam, prev, frame, hits, history, geo, geo, m2, max_history=1)[3] is None


def test_the_target_is_the_same_surface_point_of_the_previous_sphere(O):
    """Semantics, static camera, one sphere translated by (0.15, 0.05, -0.1) and rescaled by 1.25: for
    every pixel that hits it and projects in range, the previous camera's ray through the non-integer
    (u, v), traced by the oracle against the previous geometry, where it hits the same sphere at a
    depth within 1e-9 relative of z, hits it at Q' within 1e-9 |Q'|."""
    prev_spheres = O.rich_scene(2, 3)
    cam = O.camera_initialize(RICH_SETUP, W, H)[1]
    index0, _ = R.oracle_hits(O, prev_spheres, cam, W, H)
    seen = [i for i in range(1, len(prev_spheres)) if (index0 == i).sum() >= 2]  # the three large spheres
    assert seen
    checked = 0
    for i in seen:
        spheres = prev_spheres.copy()
        spheres["center"][i] += (0.15, 0.05, -0.1)
        spheres["radius"][i] *= 1.25
        geo, prev_geo = C.geometry(spheres), C.geometry(prev_spheres)
        index, t = R.oracle_hits(O, spheres, cam, W, H)
        Qp, moved = M.target(cam, W, H, index, t, geo, prev_geo)
        assert np.array_equal(moved, index == i)
        z, u, v, ok = M.project(cam, cam, W, H, index, t, geo, prev_geo)
        P, p00, pxv, pyv = R._cam(cam)
        for y, x in np.argwhere(moved & ok):
            d = (p00 + pxv * u[y, x] + pyv * v[y, x]) - P
            j, rec = O.scene_hit(prev_spheres, P, d, 1e-6, np.inf)
            if j != i or abs(rec[6] - z[y, x]) > 1e-9 * z[y, x]:
                continue  # the back of the previous sphere, or another sphere in front of it
            point = P + d * rec[6]
            assert np.abs(point - Qp[y, x]).max() <= 1e-9 * np.linalg.norm(Qp[y, x]), (i, y, x)
            checked += 1
    assert checked > 0


def constants(n):
    """A colour per list index, the last row for a miss (index -1)."""
    return np.random.default_rng(11).random((n + 1, 3))


def test_a_moved_sphere_leaves_no_ghost(O):
    """At 32 x 18, where the small spheres cover a few pixels each. History colour = a constant per
    sphere index, the frame = the same constants for the current hits, geometry = jitter of the small
    book cover: whatever is folded, every output channel stays within 1e-12 of its own index's
    constant, also where a moved sphere was seen before and something else is seen now."""
    prev_spheres = O.rich_scene(2, 3)
    spheres = C.jitter(prev_spheres)
    W, H = 32, 18
    cam = O.camera_initialize(RICH_SETUP, W, H)[1]
    prev_hits, hits = R.oracle_hits(O, prev_spheres, cam, W, H), R.oracle_hits(O, spheres, cam, W, H)
    table = constants(len(spheres))
    moved_index = np.zeros(len(spheres) + 1, dtype=bool)
    moved_index[C.small_of(prev_spheres)] = True
    uncovered = moved_index[prev_hits[0]] & (hits[0] != prev_hits[0])
    assert uncovered.sum() > 0
    frame = table[hits[0]]
    for m2 in (False, True):
        history = dict(colour=table[prev_hits[0]], age=np.full((H, W), 5, dtype=np.int32), index=prev_hits[0].copy(),
                       depth=np.where(prev_hits[0] >= 0, prev_hits[1], INF))
        if m2:
            history["m2"] = np.zeros((H, W, 3))
        got, _, rec, _ = M.step(cam, cam, frame, hits, history, C.geometry(spheres), C.geometry(prev_spheres), m2)
        assert np.abs(got["colour"] - table[hits[0]]).max() <= 1e-12
        assert 0 < rec[0] < W * H and (got["age"][moved_index[hits[0]]] > 1).any()  # moved spheres do fold


@pytest.mark.parametrize("what", ["zero_radius", "nan_radius", "inf_radius", "nan_centre", "inf_centre"])
def test_a_degenerate_previous_sphere_makes_exactly_its_pixels_fresh(O, what):
    """The previous geometry holds a zero, NaN or infinite radius or centre for one sphere, and the
    history is what the oracle sees of that geometry (no ray hits such a sphere). A NaN or an infinity
    gives a non-finite projection, a zero radius a history without that index: either way every pixel
    of that sphere is fresh, and under a static camera no other pixel is."""
    spheres = O.rich_scene(2, 3)
    cam = O.camera_initialize(RICH_SETUP, W, H)[1]
    hits = R.oracle_hits(O, spheres, cam, W, H)
    i = int(next(i for i in range(1, len(spheres)) if (hits[0] == i).sum() >= 2))  # a large sphere
    prev_spheres = spheres.copy()
    if what.endswith("radius"):
        prev_spheres["radius"][i] = dict(zero=0.0, nan=NAN, inf=INF)[what.split("_")[0]]
    else:
        prev_spheres["center"][i, 1] = dict(nan=NAN, inf=-INF)[what.split("_")[0]]
    prev_hits = R.oracle_hits(O, prev_spheres, cam, W, H)
    assert not (prev_hits[0] == i).any()
    rng = np.random.default_rng(4)
    for m2 in (False, True):
        history = history_of(rng, prev_hits, m2)
        history["age"] = np.maximum(history["age"], 1)
        got, _, rec, motion = M.step(cam, cam, rng.random((H, W, 3)), hits, history, C.geometry(spheres),
                                     C.geometry(prev_spheres), m2)
        assert np.array_equal(got["age"] == 1, hits[0] == i) and rec[0] == int((hits[0] == i).sum())
        if what != "zero_radius":
            assert np.isnan(motion[hits[0] == i]).all() and not np.isnan(motion[hits[0] != i]).any()
