"""Camera extremes on a scene that stays put, on the device against the oracle
(cases: tests/camera_extremes.py; that the oracle is a sound reference for them, that
every case is live, and the two device shortcuts restated on the CPU:
tests/test_camera_extremes_cpu.py).

Go sets the length of a camera ray's direction freely: a pinhole's is proportional to
FocalLength, a lens camera's is about FocusDistance. Sphere.Hit is scale-free in FP64,
the FP32 slab cull (trav_begin32) and the candidate bound (pixel_beam) are not. Every
case renders four ways (default, linear scan, no candidate lists, and lists that all
overflow so that every camera ray takes the traversal's place), and its camera rays
go through the ray queries; everything must match the oracle under
extremes.assert_frames_match, and the default frame must be the linear scan's bit for bit.
"""
import numpy as np
import pytest

import camera_extremes as C
import extremes as X
from test_gpu_aov import assert_aov_equal, composed, device_aov
from test_gpu_parity import bg_struct
from test_gpu_query import assert_hits_equal, device_camera_rays, device_colors, device_hits, oracle_hits

pytestmark = pytest.mark.gpu

FLAGS = [("bvh", 0), ("linear", 1)]
case_param = pytest.mark.parametrize("case", C.CASES, ids=C.IDS)


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()
    return torch


def device_frame(L, case, r, radius=X.RAY_RADIUS, flags=0):
    p = L.make_params(X.W, X.H, X.DEPTH, r, radius, C.SEED, flags=flags)
    return L.render(C.scene(case.scene), bg_struct(L, X.DEFAULT_BG), C.camera_of(L, case), p, 0, segments=True)


def in_slab_range(rays):
    d = rays[:, 3:]
    with np.errstate(all="ignore"):
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return (a >= 1e-30) & (a <= 1e30)


def same_bits_or_nan(got, want):
    """Bit-equal, a NaN standing for any NaN: its sign and payload are nobody's contract
    (Go's own 0 / 0 differs between amd64 and arm64), and a zero direction (the
    cancel-focal=2^-60 case: Unit divides 0 by 0) makes every pixel one."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return g.shape == w.shape and bool(np.all((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))))


# ------------------------------------------------------- 1. frames, four ways ----
@case_param
def test_frames_four_ways(L, O, torch, knobs, case):
    ref = C.oracle_frame(O, L, case)
    default = device_frame(L, case, case.r)
    linear = device_frame(L, case, case.r, flags=L.FLAG_LINEAR_SCAN)
    knobs(primary_candidates=0)
    nocand = device_frame(L, case, case.r)
    knobs(primary_candidates=None)
    X.assert_frames_match(linear, ref, case.id + ", linear scan")
    X.assert_frames_match(default, ref, case.id + ", default")
    X.assert_frames_match(nocand, ref, case.id + ", no candidate lists")
    assert same_bits_or_nan(default[0], linear[0]) and X.bit_identical(default[1], linear[1]), case.id
    # r = 4 under an anti-aliasing disc of 30 pixels, which covers the frame: the lists overflow
    for radius in C.overflow_radii(case):
        wide = device_frame(L, case, 4, radius)
        X.assert_frames_match(wide, C.oracle_frame(O, L, case, 4, radius), f"{case.id}, ray radius {radius}")
    n_seg, n_sph, n_box = depth1_stats(L, torch, case, 4, radius)
    ok = in_slab_range(C.frame_rays(O, L, case, 4, radius)[0])
    assert n_seg == X.W * X.H * 4
    # Nothing but an overflowed list makes a depth-1 render test a box; a camera ray outside
    # slab_dir_ok's range tests every sphere (1 out of the tree, 23 in it) instead.
    assert n_box > 0 or not ok.any(), (case.id, n_box)
    if not ok.any():
        assert n_sph == n_seg * 24, (case.id, n_sph)


def depth1_stats(L, torch, case, r, radius):
    """(Scene.Hit calls, sphere tests, box tests) of a depth-1 render: camera rays only."""
    spheres, st = C.scene(case.scene), C.camera_of(L, case)
    dev = L.DeviceScene(spheres, bg_struct(L, X.DEFAULT_BG), 0)
    try:
        assert dev.info().has_bvh == 1 and dev.info().n_global == 1
        p1 = L.make_params(X.W, X.H, 1, r, radius, C.SEED)
        assert dev.plan(st, p1).bvh == 1
        out = torch.empty((X.H, X.W, 3), dtype=torch.float64, device="cuda")
        stats = torch.zeros(3, dtype=torch.int64, device="cuda")
        dev.render_stats_async(st, p1, out.data_ptr(), stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return stats.tolist()
    finally:
        dev.release()


# ------------------------------------------------------- 2. fixed-point path ----
@pytest.mark.parametrize("k", [-110, -530])
def test_r64_fixed_point_sums(L, O, knobs, k):
    case = C.BY_ID[f"focal=2^{k}"]
    ref = C.oracle_frame(O, L, case, 64)
    dev = L.DeviceScene(C.scene(case.scene), bg_struct(L, X.DEFAULT_BG), 0)
    try:
        plan = dev.plan(C.camera_of(L, case), L.make_params(X.W, X.H, X.DEPTH, 64, X.RAY_RADIUS, C.SEED)).as_dict()
    finally:
        dev.release()
    assert plan["bvh"] == 1 and plan["fixed_point_shift"] > 0 and plan["acc_slots"] > 0, plan
    default = device_frame(L, case, 64)
    linear = device_frame(L, case, 64, flags=L.FLAG_LINEAR_SCAN)
    knobs(primary_candidates=0)
    nocand = device_frame(L, case, 64)
    knobs(primary_candidates=None)
    for frame, how in ((default, "default"), (linear, "linear scan"), (nocand, "no candidate lists")):
        X.assert_frames_match(frame, ref, f"{case.id}, r = 64, {how}")
    assert same_bits_or_nan(default[0], linear[0]) and X.bit_identical(default[1], linear[1]), case.id


# ------------------------------------------------------------ 3. CameraRays ----
@case_param
def test_camera_rays_bit_for_bit(L, O, torch, case):
    p = L.make_params(X.W, X.H, X.DEPTH, case.r, X.RAY_RADIUS, C.SEED)
    rays, ids = device_camera_rays(L, torch, C.camera_of(L, case), p)
    want, want_ids = C.frame_rays(O, L, case)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), want_ids)
    assert same_bits_or_nan(rays.cpu().numpy(), want), case.id


# ------------------------------------------- 4. Scene.Hit and Scene.RayColor ----
def query_reference(O, L, case):
    key = ("query-ref", case.id)
    if key not in C._cache:
        spheres = C.scene(case.scene)
        rays, ids = C.frame_rays(O, L, case)
        col = [O.ray_color(spheres, X.DEFAULT_BG, r[:3], r[3:], X.DEPTH, C.SEED, int(i[0]), int(i[1]))
               for r, i in zip(rays, ids)]
        C._cache[key] = (oracle_hits(O, L, spheres, rays), np.array([c[0] for c in col]),
                         np.array([c[1] for c in col], dtype=np.uint32))
    return C._cache[key]


@case_param
@pytest.mark.parametrize("name,flags", FLAGS)
def test_hit_and_ray_color_of_the_camera_rays(L, O, torch, case, name, flags):
    rays, ids = C.frame_rays(O, L, case)
    want, rgb, seg = query_reference(O, L, case)
    if case.live:
        assert (want["index"] > 0).sum() >= 100  # index 0 is the ground
    dev = L.DeviceScene(C.scene(case.scene), bg_struct(L, X.DEFAULT_BG), 0)
    try:
        got = device_hits(L, torch, dev, rays, flags=flags)
        col = device_colors(L, torch, dev, rays, X.DEPTH, C.SEED, ids, flags=flags)
    finally:
        dev.release()
    assert_hits_equal(got, want, f"{case.id}, {name}")
    X.assert_frames_match(col, (rgb, seg), f"{case.id}, {name}, RayColor")


# --------------------------------------------------- 5. the guard's boundary ----
def steps(v, n):
    """v and its n neighbours on either side."""
    out = [float(v)]
    for _ in range(n):
        out = [float(np.nextafter(out[0], 0.0))] + out + [float(np.nextafter(out[-1], np.inf))]
    return out


def boundary_lengths(target):
    """Component pairs (x, y) with x * x + y * y at `target`'s boundary: y = 0 and x within
    3 ulp of sqrt(target) (x * x then lands within a few ulp of target, on both sides and on
    it), and a 4 : 3 pair for each of the three doubles pred(target), target, succ(target)."""
    r = float(np.sqrt(target))
    want = {float(np.nextafter(target, 0.0)), float(target), float(np.nextafter(target, np.inf))}
    pairs = {}
    for y in steps(0.6 * r, 40):
        for x in steps(0.8 * r, 3):
            if x * x + y * y in want:
                pairs.setdefault(x * x + y * y, (x, y))
    assert set(pairs) == want
    return [(x, 0.0) for x in steps(r, 3)] + list(pairs.values())


def boundary_rays(O, L, M):
    """Rays whose |d|^2 is 1e-30 or 1e30, the double on either side of it, or a few ulp
    further: one or two components carry the length, the others are zero or below the
    clamp's 1e-30, of either sign. Origins: hit points of the focal-length-1 frame (on
    sphere surfaces), a point 3 before the centre of a unit sphere, and a point on the
    bound (one coordinate nextafter(M, 0)) looking back at that sphere."""
    case = C.BY_ID["focal=2^0"]
    spheres = C.scene(case.scene)
    hit = oracle_hits(O, L, spheres, C.centre_rays(O, L, case))
    points = hit["point"][hit["index"] > 0][::17][:6]
    centre = np.array(spheres[X.VICTIM]["center"])
    edge = float(np.nextafter(M, 0.0))
    tiny2 = [(0.0, 0.0), (5e-31, 0.0), (-5e-31, 0.0), (3e-31, -7e-31), (-2e-33, 4e-31), (5e-324, -5e-324)]
    tiny1 = [0.0, 5e-31, -5e-31, -2e-33, 5e-324]
    out = []
    for target in (1e-30, 1e30):
        for x, y in boundary_lengths(target):
            for axis in range(3):
                second, third = (axis + 1) % 3, (axis + 2) % 3
                for sign in (1.0, -1.0):
                    dirs = []
                    for t in (tiny2 if y == 0.0 else tiny1):
                        d = np.zeros(3)
                        d[axis] = sign * x
                        d[second], d[third] = (t[0], t[1]) if y == 0.0 else (y, t)
                        dirs.append(d)
                    u = dirs[0] / x  # scaled first: the squares of a 1e-15 vector would lose bits
                    u /= np.linalg.norm(u)
                    on_bound = centre - u * ((centre[axis] + sign * edge) / u[axis])
                    on_bound[axis] = -sign * edge
                    for o in (*points, centre - 3.0 * u, on_bound):
                        out += [np.r_[o, d] for d in dirs]
    return np.array(out)


_boundary = {}


def boundary_reference(O, L, M):
    if not _boundary:
        spheres = C.scene("moved")
        rays = boundary_rays(O, L, M)
        col = [O.ray_color(spheres, X.DEFAULT_BG, r[:3], r[3:], X.DEPTH, C.SEED, 0, 0) for r in rays]
        _boundary["ref"] = (rays, oracle_hits(O, L, spheres, rays), np.array([c[0] for c in col]),
                            np.array([c[1] for c in col], dtype=np.uint32))
    return _boundary["ref"]


@pytest.mark.parametrize("name,flags", FLAGS)
def test_rays_on_the_query_guards_boundary(L, O, torch, name, flags):
    dev = L.DeviceScene(C.scene("moved"), bg_struct(L, X.DEFAULT_BG), 0)
    try:
        M = dev.info().bound
        rays, want, rgb, seg = boundary_reference(O, L, M)
        d = rays[:, 3:]
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        for target in (1e-30, 1e30):
            near = np.abs(a / target - 1.0) < 1e-12
            for v in (np.nextafter(target, 0.0), target, np.nextafter(target, np.inf)):
                assert (a == v).sum() >= 100, (target, v)
            below, above = near & (a < target), near & (a >= target)
            if target < 1:  # both sides of the small boundary hit tree spheres
                assert (want["index"][below] > 0).sum() >= 100 and (want["index"][above] > 0).sum() >= 100
            else:           # a direction longer than 1e15 puts every root below Interval.Start
                assert (want["index"][near] < 0).all()
        assert (np.abs(rays[:, :3]).max(1) == np.nextafter(M, 0.0)).sum() >= 100
        got = device_hits(L, torch, dev, rays, flags=flags)
        ids = np.zeros((len(rays), 2), dtype=np.uint32)  # the reference's draws: pixel 0, sample 0
        col = device_colors(L, torch, dev, rays, X.DEPTH, C.SEED, ids, flags=flags)
    finally:
        dev.release()
    assert_hits_equal(got, want, name)
    X.assert_frames_match(col, (rgb, seg), name + ", RayColor")


# ------------------------------------------------------------- 6. RenderAOV ----
FOCAL = [c for c in C.CASES if c.id.startswith("focal=2^")]


@pytest.mark.parametrize("case", FOCAL, ids=[c.id for c in FOCAL])
@pytest.mark.parametrize("name,flags", FLAGS)
def test_aov_equals_composed_queries(L, O, torch, case, name, flags):
    spheres, st = C.scene(case.scene), C.camera_of(L, case)
    p = L.make_params(X.W, X.H, X.DEPTH, case.r, X.RAY_RADIUS, C.SEED, flags=flags)
    bg = bg_struct(L, X.DEFAULT_BG)
    dev = L.DeviceScene(spheres, bg, 0)
    try:
        got = device_aov(L, torch, dev, st, p)
        want = composed(L, torch, dev, bg, spheres, st, p, flags)
    finally:
        dev.release()
    if case.live:  # what the composition holds comes from queries the tests above pin to the oracle
        hits = query_reference(O, L, case)[0]["index"].reshape(X.H, X.W, case.r)[:, :, 0]
        assert np.array_equal(want["index"], hits.astype(np.int32)) and (want["index"] > 0).sum() >= 100
    assert_aov_equal(got, want, f"{case.id} {name}")
