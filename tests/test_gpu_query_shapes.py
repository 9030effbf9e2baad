"""Every kernel that finds its hits outside the megakernel (tray_scene_hit_async,
tray_scene_occluded_async, tray_ray_color_async, tray_render_aov_async, tray_render_pixels_async and
both instances of the temporal step: all through query_hit / query_occluded of
tray_query_device.hpp) on every shape of tests/query_shapes.py: leaves of 1, 2 and 4 spheres, 0, 1 and
2 out-of-tree spheres, the smallest tree and none, and traversal stacks on both sides of each
threshold at which a launch gives up the tree for the linear scan, the launch with exactly 64 KiB of
dynamic LDS included. The helpers and the tolerances are those of the files that test the same calls
on the book cover; the references are the oracle, the composition of the public queries, and the
megakernel, which reaches the same scenes through its own traversal and stack overflow area.

Then the lane-to-group shapes of the pixel-list renderer (render_pixels_kernel): a group that fills a
wave, leaves lanes of it idle, is the first to span the workgroup, shares it, fills it, and takes a
second round.

Every case first asserts, from the oracle's side, that its rays do exercise the traversal
(query_shapes.assert_live), and for the temporal cases that some but not all pixels are fresh.
"""
import numpy as np
import pytest

import query_shapes as Q
import temporal_ref as R
import temporal_variance_ref as V
from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_adaptive import check_list, dev_book, device_pixels, ordered_frames  # noqa: F401 (fixtures)
from test_gpu_aov import assert_aov_equal, composed, device_aov
from test_gpu_parity import bg_struct, camera
from test_gpu_query import (INF, TOL, assert_hits_equal, bits, device_colors, device_hits, oracle_camera_rays,
                            oracle_hits, rich2, torch)  # noqa: F401 (fixtures)
from test_gpu_shade import device_occluded
from test_gpu_temporal import CAP, assert_state, device_step, pair_of, random_history
from test_gpu_temporal import device_hits as centre_hits
from test_gpu_temporal_variance import random_m2, same_bits_or_nan, var_step

pytestmark = pytest.mark.gpu

W, H = Q.W, Q.H
SEED, DEPTH = 9, 12
FLAGS = [("tree", 0), ("scan", 1)]  # TRAY_FLAG_LINEAR_SCAN; "tree" is the library's own choice (it may scan)


class Case:
    pass


@pytest.fixture(scope="module", params=Q.SHAPES, ids=repr)
def case(request, L, O, torch):
    """One upload per shape, with its facts asserted; the rays of the hit, occlusion and colour
    checks (the 40 x 24 camera rays at r = 1 and as many secondary rays leaving their hit points in
    random directions) and the r = 3 camera rays of the frame checks, with the oracle's hits."""
    c = Case()
    c.shape = request.param
    c.spheres = c.shape.build(O)
    c.n = len(c.spheres)
    c.bg = bg_struct(L, DEFAULT_BG)
    c.dev = Q.upload(L, c.shape, c.spheres, c.bg)
    try:
        c.info = c.dev.info()
        print(f"{c.shape.name}: {Q.facts(c.info)} traversal {Q.traversal(L, c.info) if c.info.has_bvh else None}")
        c.st = camera(L, c.shape.setup, W, H)
        c.prim, c.ids = oracle_camera_rays(O, c.st.as_array(), W, range(H), 1, 0, 0.5, SEED)
        first = oracle_hits(O, L, c.spheres, c.prim)
        pts = first["point"][first["index"] >= 0]
        d = np.random.default_rng(2).normal(size=(len(pts), 3))
        c.rays = np.concatenate([c.prim, np.concatenate([pts, d], axis=1)])
        if c.shape.originals:  # and three rays from the camera at each duplicated sphere: equal roots
            twice = c.spheres[c.shape.originals:]
            eye = np.asarray(c.shape.setup[:3], dtype=np.float64)
            at = np.repeat(twice["center"], 3, axis=0) + 0.4 * np.repeat(twice["radius"], 3)[:, None] * \
                np.random.default_rng(3).normal(size=(3 * len(twice), 3))
            c.rays = np.concatenate([c.rays, np.concatenate([np.broadcast_to(eye, at.shape), at - eye], axis=1)])
        c.want = np.concatenate([first, oracle_hits(O, L, c.spheres, c.rays[len(c.prim):])])
        Q.assert_live(c.shape, c.n, c.info.bound, c.rays[:, :3], c.want["index"], "camera and secondary rays")
        Q.assert_live(c.shape, c.n, c.info.bound, c.prim[:, :3], first["index"], "camera rays")
        assert (c.want["front_face"][c.want["index"] >= 0] == 0).any()  # some hits from inside
        c.rays3, _ = oracle_camera_rays(O, c.st.as_array(), W, range(H), 3, 0, 0.5, SEED)
        c.want3 = oracle_hits(O, L, c.spheres, c.rays3)
        Q.assert_live(c.shape, c.n, c.info.bound, c.rays3[:, :3], c.want3["index"], "r = 3 camera rays")
        yield c
    finally:
        c.dev.release()


# -------------------------------------------------------------------- hit --
def test_hit(L, torch, case):
    c = case
    for name, flags in FLAGS:
        got = device_hits(L, torch, c.dev, c.rays, flags=flags)
        assert (got["index"] < c.n).all() and (got["index"] >= -1).all(), f"{c.shape} {name}: an index outside the list"
        if c.shape.originals:  # equal roots: the sphere listed first wins, never its appended copy
            assert (got["index"] < c.shape.originals).all(), f"{c.shape} {name}: an appended sphere won a tie"
        assert_hits_equal(got, c.want, f"{c.shape} {name}")
    if c.shape.originals:
        small = np.nonzero(c.spheres["radius"][:c.shape.originals] < 0.5)[0][:40]
        assert np.isin(c.want["index"], small).sum() >= 20  # the duplicated spheres are hit


# --------------------------------------------------------------- occluded --
def test_occluded(L, O, torch, case):
    """The same rays at t_end = +inf, at each ray's own closest root (strict: that root no longer
    counts, and no other lies below it) and one ulp above it (it is back), and at one root for all
    rays; the answer is the hit query's index >= 0 at that end."""
    c = case
    hit = c.want["index"] >= 0
    root = np.where(hit, c.want["t"], 1.0)
    above = np.nextafter(root, INF)
    middle = float(np.sort(c.want["t"][hit])[hit.sum() // 2])
    # the oracle agrees with the rule used for the per-ray ends
    for i in np.nonzero(hit)[0][::17]:
        r = c.rays[i]
        assert O.scene_hit(c.spheres, r[:3], r[3:], 1e-6, float(root[i]))[0] < 0
        assert O.scene_hit(c.spheres, r[:3], r[3:], 1e-6, float(above[i]))[0] == c.want["index"][i]
    for name, flags in FLAGS:
        what = f"{c.shape} {name}"
        closest = device_hits(L, torch, c.dev, c.rays, flags=flags)["index"] >= 0
        assert np.array_equal(closest, hit), what
        for label, kw, ref in (("+inf", dict(t_end=INF), closest),
                               ("own root", dict(ends=root), np.zeros(len(hit), dtype=bool)),
                               ("one ulp above", dict(ends=above), closest),
                               ("one root", dict(t_end=middle),
                                device_hits(L, torch, c.dev, c.rays, t_end=middle, flags=flags)["index"] >= 0)):
            got = device_occluded(torch, c.dev, c.rays, flags=flags, **kw)
            assert set(np.unique(got)) <= {0, 1}, f"{what} {label}: a byte was not written"
            bad = np.nonzero(got.astype(bool) != ref)[0]
            assert bad.size == 0, f"{what} {label}: {bad.size} rays differ, first {bad[:3]}"
            if label == "one root":
                assert ref.any() and not ref[hit].all()


# ------------------------------------------------------------- ray colour --
def test_ray_color(L, O, torch, case):
    c = case
    want = [O.ray_color(c.spheres, DEFAULT_BG, r[:3], r[3:], DEPTH, SEED, int(i[0]), int(i[1]))
            for r, i in zip(c.prim, c.ids)]
    ref = np.array([w[0] for w in want])
    rseg = np.array([w[1] for w in want], dtype=np.uint32)
    assert (rseg > 1).any()  # paths that go on after their first hit (under the dome every path runs to the depth)
    frames = []
    for name, flags in FLAGS:
        rgb, seg = device_colors(L, torch, c.dev, c.prim, DEPTH, SEED, c.ids, flags)
        assert np.array_equal(seg, rseg), f"{c.shape} {name}: {int((seg != rseg).sum())} paths took different decisions"
        err = float(np.abs(rgb - ref).max())
        print(f"{c.shape} ray colour {name}: L-inf {err:.3e}")
        assert err <= TOL, f"{c.shape} {name}: L-inf {err}"
        frames.append(rgb)
    assert np.array_equal(bits(frames[0]), bits(frames[1])), f"{c.shape}: the tree and the scan differ"


# -------------------------------------------------------- feature buffers --
def test_feature_buffers(L, torch, case):
    """r = 3 against CameraRays -> Scene.Hit reduced in sample order (test_aov_equals_composed_queries);
    the index plane holds list indices: the oracle's first-sample hits."""
    c = case
    first = np.ascontiguousarray(c.want3["index"].reshape(H, W, 3)[:, :, 0]).astype(np.int32)
    for name, flags in FLAGS:
        p = L.make_params(W, H, 10, 3, 0.5, SEED, flags=flags)
        got = device_aov(L, torch, c.dev, c.st, p)
        want = composed(L, torch, c.dev, c.bg, c.spheres, c.st, p, flags)
        assert (want["index"] >= 0).any() and (want["coverage"] > 0).any()
        assert_aov_equal(got, want, f"{c.shape} {name}")
        assert np.array_equal(got["index"], first), f"{c.shape} {name}: the index plane is not the oracle's"


# ------------------------------------------------------------- pixel list --
def test_pixel_list(L, torch, case):
    """r = 3, depth 12, 2 passes of every 7th pixel and a bad entry against the megakernel's
    ordered-sum render of the same passes: bits and segment counts."""
    c = case
    n = W * H
    lst = np.concatenate([np.arange(3, n, 7), [n + 5]])
    listed = lst[lst < n]
    Q.assert_live(c.shape, c.n, c.info.bound, c.rays3.reshape(n, 3, 6)[listed][..., :3],
                  c.want3["index"].reshape(n, 3)[listed], "listed pixels")
    kw = dict(width=W, height=H, max_depth=DEPTH, rays_per_pixel=3, ray_radius=0.5, seed=SEED)
    frames = ordered_frames(L, torch, c.dev, c.st, (0, 1), **kw)
    lit = bool(frames[0][0].any())  # under the dome no path reaches the sky: every pixel is black, in every pass
    assert lit == (c.shape.name != "dome")
    assert not lit or not np.array_equal(frames[0][0], frames[1][0])
    for name, flags in FLAGS:
        got, seg = device_pixels(L, torch, c.dev, c.st, L.make_params(W, H, DEPTH, 3, 0.5, SEED, flags=flags), lst, 2)
        check_list(got, seg, frames, lst, lambda k, pix: k, f"{c.shape} {name}")


# ---------------------------------------------------------- temporal step --
def _temporal_inputs(L, O, torch, c, which):
    s_prev, s_cur = pair_of(c.shape.setup, which)
    prev, cam = camera(L, s_prev, W, H), camera(L, s_cur, W, H)
    seen = R.oracle_hits(O, c.spheres, cam.as_array(), W, H)
    o, _ = R.centre_rays(cam.as_array(), W, H)
    Q.assert_live(c.shape, c.n, c.info.bound, np.broadcast_to(o, (W * H, 3)), seen[0], f"{which} centre rays")
    hits = centre_hits(L, torch, c.dev, cam, W, H)
    assert np.array_equal(hits[0], seen[0]), f"{c.shape} {which}: the centre rays' hits are not the oracle's"
    assert np.array_equal(bits(hits[1][seen[0] >= 0]), bits(seen[1][seen[0] >= 0]))
    tp = L.temporal_params(max_history=CAP)
    history = random_history(np.random.default_rng(5), centre_hits(L, torch, c.dev, prev, W, H), W, H,
                             tp.depth_tolerance)
    frame = np.random.default_rng(W * 1000 + H + len(which)).random((H, W, 3))
    frame[H // 2, W // 2, 1] = float("nan")
    return prev, cam, seen, hits, tp, history, frame


def _fresh_some(c, which, rec, got):
    assert rec == (int((got["age"] == 1).sum()), int(got["age"].astype(np.int64).sum()))
    print(f"{c.shape} {which}: fresh {rec[0]} of {W * H}")
    assert 0 < rec[0] < W * H, "the case exercises neither the fold nor the fresh path"


@pytest.mark.parametrize("which", ["orbit", "dolly"])
def test_temporal_step(L, O, torch, case, which):
    c = case
    prev, cam, seen, hits, tp, history, frame = _temporal_inputs(L, O, torch, c, which)
    want, want_rec = R.step(cam.as_array(), prev.as_array(), frame, hits, history, CAP, tp.depth_tolerance, tp.snap)
    got, rec = device_step(L, torch, c.dev, cam, prev, tp, frame, history, W, H)
    assert_state(got, want, f"{c.shape} {which}")
    assert rec == want_rec
    assert np.array_equal(got["index"], seen[0]), f"{c.shape} {which}: the index plane is not the oracle's"
    _fresh_some(c, which, rec, got)
    scan, scan_rec = device_step(L, torch, c.dev, cam, prev,
                                 L.temporal_params(max_history=CAP, flags=L.FLAG_LINEAR_SCAN), frame, history, W, H)
    assert_state(scan, got, f"{c.shape} {which} TRAY_FLAG_LINEAR_SCAN")
    assert scan_rec == rec


@pytest.mark.parametrize("which", ["orbit", "dolly"])
def test_temporal_var_step(L, O, torch, case, which):
    c = case
    prev, cam, seen, hits, tp, history, frame = _temporal_inputs(L, O, torch, c, which)
    history["m2"] = random_m2(np.random.default_rng(6), W, H)
    want, want_var, want_rec = V.step(cam.as_array(), prev.as_array(), frame, hits, history, CAP, tp.depth_tolerance,
                                      tp.snap)
    got, var, rec = var_step(L, torch, c.dev, cam, prev, tp, frame, history, W, H)
    what = f"{c.shape} {which} m2"
    assert_state(got, want, what)
    assert rec == want_rec
    same_bits_or_nan(got["m2"], want["m2"], what)
    same_bits_or_nan(var, want_var, what + " variance")
    assert np.array_equal(got["index"], seen[0]), f"{what}: the index plane is not the oracle's"
    _fresh_some(c, which, rec, got)
    scan, scan_var, scan_rec = var_step(L, torch, c.dev, cam, prev,
                                        L.temporal_params(max_history=CAP, flags=L.FLAG_LINEAR_SCAN), frame, history,
                                        W, H)
    assert_state(scan, got, what + " TRAY_FLAG_LINEAR_SCAN")
    same_bits_or_nan(scan["m2"], got["m2"], what + " TRAY_FLAG_LINEAR_SCAN")
    same_bits_or_nan(scan_var, var, what + " TRAY_FLAG_LINEAR_SCAN variance")
    assert scan_rec == rec


# ------------------------------------- group shapes of the pixel-list renderer --
# g = min(r, 256) lanes serve one (pixel, pass) group; a group of at most 64 lanes lies within a
# wave, a larger one within the workgroup; r > 256 takes ceil(r / 256) rounds through the running sum.
GROUP_LIST = np.array([0, 39, 400, 401, 517, 700, 959, 5000])  # 5000: a bad entry (960 pixels)
GROUP_DEPTH, GROUP_SEED = 8, 2


def _group_frames(L, torch, dev, st, r, flags):
    kw = dict(width=W, height=H, max_depth=GROUP_DEPTH, rays_per_pixel=r, ray_radius=0.5, seed=GROUP_SEED, flags=flags)
    return ordered_frames(L, torch, dev, st, (0, 1, 2), **kw)


@pytest.mark.parametrize("r", [33, 48,  # idle lanes in the group's wave
                               64,      # a wave exactly
                               65,      # the first workgroup-wide group
                               100,     # two groups per workgroup, 56 idle lanes
                               128, 255,
                               256,     # one full round
                               257,     # a second round of one sample
                               512])    # two full rounds
def test_render_pixels_group_shapes(L, torch, dev_book, r):
    st = camera(L, RICH_SETUP, W, H)
    plane = (np.arange(W * H) % 2).astype(np.int32)
    assert len(set(plane[GROUP_LIST[:-1]].tolist())) == 2
    frames = _group_frames(L, torch, dev_book, st, r, 0)
    for name, flags in FLAGS:
        p = L.make_params(W, H, GROUP_DEPTH, r, 0.5, GROUP_SEED, flags=flags)
        got, seg = device_pixels(L, torch, dev_book, st, p, GROUP_LIST, 2, plane)
        check_list(got, seg, frames, GROUP_LIST, lambda k, pix: int(plane[pix]) + k, f"r={r} {name}")


@pytest.mark.parametrize("lst", [[517], [0, 39, 400, 401, 517, 700, 959, 5000, 123]], ids=["one", "nine"])
def test_render_pixels_group_counts(L, torch, dev_book, lst):
    """r = 100: two groups per workgroup. One pass of the 1-entry or the 9-entry list is an odd number
    of groups: the last workgroup holds one group and one empty slot. Two passes fill it."""
    r, lst = 100, np.array(lst)
    st = camera(L, RICH_SETUP, W, H)
    plane = (np.arange(W * H) % 2).astype(np.int32)
    frames = _group_frames(L, torch, dev_book, st, r, 0)
    for name, flags in FLAGS:
        p = L.make_params(W, H, GROUP_DEPTH, r, 0.5, GROUP_SEED, flags=flags)
        for n_passes in (1, 2):
            got, seg = device_pixels(L, torch, dev_book, st, p, lst, n_passes, plane)
            check_list(got, seg, frames, lst, lambda k, pix: int(plane[pix]) + k,
                       f"{len(lst)} entries {name} n_passes={n_passes}")
