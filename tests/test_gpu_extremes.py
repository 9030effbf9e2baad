"""FP64-range extremes and degenerate scene data on the device against the oracle
(scenes, cases and the comparison rule: tests/extremes.py; that the oracle is a
sound reference for them and that every case is live: tests/test_extremes_cpu.py).

The megakernel's FP64 shortcuts (sqrt_cr, rcp_cr, sdiv_rcp, div_root, disc's
wa == 0 case) each have a branch for operands outside a comfortable range, and
the BVH culls in FP32 with margins scaled by the scene bound. Here whole scenes
are scaled by 2^k from 2^-530 to 2^511, one scene mixes magnitudes (a cluster
inside a mirror 2^7 times its size) and one sphere of a scene takes zero,
subnormal, huge, infinite and NaN fields in turn.

Rule (extremes.assert_frames_match): per-pixel Scene.Hit counts equal,
non-finite colour entries of the same class and sign, finite ones within
1e-12 max(1, |ref|): the attenuation product order is the only difference.

Each test also asserts which path ran: tray_scene_get_info().has_bvh and
tray_render_plan_get().bvh. A scene has a tree iff all of it is finite and
within +-2^28 (tray_bvh.cpp); otherwise it takes the linear scan.
"""
import numpy as np
import pytest

import extremes as X
from test_gpu_parity import bg_struct
from test_gpu_query import assert_hits_equal, device_colors, device_hits, oracle_camera_rays, oracle_hits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()
    return torch


def device_frame(L, spheres, st, spp, seed, flags=0, depth=X.DEPTH):
    p = L.make_params(X.W, X.H, depth, spp, X.RAY_RADIUS, seed, flags=flags)
    return L.render(spheres, bg_struct(L, X.DEFAULT_BG), st, p, 0, segments=True)


def paths_reported(L, spheres, st, spp, seed):
    """(has_bvh, plan of a default render, plan of a linear-scan render)."""
    dev = L.DeviceScene(spheres, bg_struct(L, X.DEFAULT_BG), 0)
    try:
        info = dev.info()
        plan = dev.plan(st, L.make_params(X.W, X.H, X.DEPTH, spp, X.RAY_RADIUS, seed)).as_dict()
        lin = dev.plan(st, L.make_params(X.W, X.H, X.DEPTH, spp, X.RAY_RADIUS, seed,
                                         flags=L.FLAG_LINEAR_SCAN)).as_dict()
        return int(info.has_bvh), plan, lin
    finally:
        dev.release()


def three_ways(L, knobs, spheres, st, spp, seed):
    """Default (BVH and candidate lists where the scene has a tree), linear scan, no candidate lists."""
    default = device_frame(L, spheres, st, spp, seed)
    linear = device_frame(L, spheres, st, spp, seed, flags=L.FLAG_LINEAR_SCAN)
    knobs(primary_candidates=0)
    nocand = device_frame(L, spheres, st, spp, seed)
    knobs(primary_candidates=None)
    return default, linear, nocand


# ------------------------------------------------------------ A. scale sweep ----
SWEEP = [(name, k) for name in X.SCENES for k in X.scales_of(name)]


@pytest.mark.parametrize("name,k", SWEEP, ids=[f"{n}-2^{k}" for n, k in SWEEP])
def test_scale_sweep(L, O, knobs, name, k):
    spheres, st = X.scene_at(L, name, k)
    spp, seed = X.RENDER[name]
    ref = X.oracle_frame(O, L, name, k)
    default, linear, nocand = three_ways(L, knobs, spheres, st, spp, seed)
    what = f"{name} at 2^{k}"
    X.assert_frames_match(linear, ref, what + ", linear scan")
    X.assert_frames_match(default, ref, what + ", default")
    X.assert_frames_match(nocand, ref, what + ", no candidate lists")
    if name == "MIRRORS24":
        for frame, how in ((default, "default"), (linear, "linear scan"), (nocand, "no candidate lists")):
            X.assert_frames_match(frame, X.numpy_frame(L, k), f"{what}, {how}, against the numpy restatement")
    assert X.bit_identical(default[0], linear[0]) and X.bit_identical(default[1], linear[1]), what
    # which path this scale ran
    has_bvh, plan, lin = paths_reported(L, spheres, st, spp, seed)
    tree = int(k <= X.LAST_BVH_SCALE[name])
    assert tree == X.expect_has_bvh(spheres)
    assert (has_bvh, plan["bvh"], lin["bvh"]) == (tree, tree, 0), what
    assert plan["fixed_point_shift"] == 0 and plan["acc_slots"] == 0  # r < 64: FP64 sums in sample order


@pytest.mark.parametrize("name", list(X.SCENES))
@pytest.mark.parametrize("k", [0, 100])
def test_scale_through_fixed_point_sums(L, O, knobs, name, k):
    """r = 64: the on-chip fixed-point pixel sums, through the tree (2^0) and the linear scan (2^100)."""
    spheres, st = X.scene_at(L, name, k)
    _, seed = X.RENDER[name]
    ref = X.oracle_frame(O, L, name, k, spp=64)
    default, linear, nocand = three_ways(L, knobs, spheres, st, 64, seed)
    what = f"{name} at 2^{k}, r = 64"
    X.assert_frames_match(linear, ref, what + ", linear scan")
    X.assert_frames_match(default, ref, what + ", default")
    X.assert_frames_match(nocand, ref, what + ", no candidate lists")
    assert X.bit_identical(default[0], linear[0]) and X.bit_identical(default[1], linear[1]), what
    has_bvh, plan, lin = paths_reported(L, spheres, st, 64, seed)
    tree = int(k <= X.LAST_BVH_SCALE[name])
    assert (has_bvh, plan["bvh"], lin["bvh"]) == (tree, tree, 0), what
    # fixed-point sums either way; kept on chip by the BVH kernel, through the sample buffer by the linear scan
    assert plan["fixed_point_shift"] > 0 and (plan["acc_slots"] > 0) == bool(tree), plan


# -------------------------------------------------------- B. mixed magnitude ----
@pytest.fixture(scope="module", params=[X.LAST_BVH_SCALE["ENCLOSED24"], X.ENCLOSED_SUSPECT],
                ids=lambda k: f"2^{k}")
def returning_rays(request, O, L):
    """A few hundred rays from the oracle's hit points on the enclosure that hit a
    cluster sphere next (the CPU trace of every sample of the frame), with the
    oracle's hit records. 2^123: the origins are beyond FLT_MAX; 2^22: the largest
    scale with a tree."""
    k = request.param
    spheres, st = X.scene_at(L, "ENCLOSED24", k)
    spp, seed = X.RENDER["ENCLOSED24"]
    rays = []
    for sample in range(spp):
        rays += X.enclosure_returns(X.trace_sample(O, spheres, st.as_array(), spp, seed, sample))
    rays = np.array(rays)
    want = oracle_hits(O, L, spheres, rays)
    assert len(rays) >= 200 and (want["index"] > 0).all() and len(set(want["index"].tolist())) >= 8
    return k, spheres, rays, want


@pytest.mark.parametrize("how,flags", [("default", 0), ("linear", 1)])
def test_rays_from_the_enclosure_into_the_cluster(L, torch, returning_rays, how, flags):
    k, spheres, rays, want = returning_rays
    dev = L.DeviceScene(spheres, bg_struct(L, X.DEFAULT_BG), 0)
    try:
        assert dev.info().has_bvh == int(k <= X.LAST_BVH_SCALE["ENCLOSED24"])
        got = device_hits(L, torch, dev, rays, flags=flags)
    finally:
        dev.release()
    assert_hits_equal(got, want, f"ENCLOSED24 at 2^{k}, {how}")


# ------------------------------------------------------ C. degenerate fields ----
DEGENERATE = X.degenerate_cases()


@pytest.mark.parametrize("case", DEGENERATE, ids=[c[0] for c in DEGENERATE])
def test_degenerate_field(L, O, case):
    spheres = X.apply_case(case)
    st = X.camera_state(L, X.MIXED_SETUP)
    spp, seed = X.RENDER["MIXED24"]
    ref = X.degenerate_frame(O, L, case)
    linear = device_frame(L, spheres, st, spp, seed, flags=L.FLAG_LINEAR_SCAN)
    default = device_frame(L, spheres, st, spp, seed)
    X.assert_frames_match(linear, ref, case[0] + ", linear scan")
    X.assert_frames_match(default, ref, case[0] + ", default")
    has_bvh, plan, lin = paths_reported(L, spheres, st, spp, seed)
    # Non-finite geometry: the documented fallback. 1e200 is finite but beyond
    # the bound: the same. Zero, subnormal and tiny radii and every material
    # field keep the tree.
    tree = 0 if X.nonfinite_geometry(case) else int(not (X.is_geometry(case) and case[4] == 1e200))
    assert tree == X.expect_has_bvh(spheres)
    # An infinite or NaN albedo keeps the tree (Scene.Hit queries use it) but renders through
    # the linear scan, whose instance multiplies an ended path's black by its attenuations.
    wild = case[2] == "albedo" and not np.isfinite(case[4])
    assert (has_bvh, plan["bvh"], lin["bvh"]) == (tree, int(tree and not wild), 0), case[0]


@pytest.mark.parametrize("material", [X.LAMBERTIAN, X.METAL])
def test_nan_albedo_leaves_the_fixed_point_sums(L, O, material):
    """r = 64 with a NaN albedo: no colour bound, so the plan reports the FP64 sums
    (fixed_point_shift == 0), and the frame still matches, NaN for NaN."""
    case = next(c for c in DEGENERATE if c[1] == material and c[2] == "albedo" and c[4] != c[4])
    spheres = X.apply_case(case)
    st = X.camera_state(L, X.MIXED_SETUP)
    _, seed = X.RENDER["MIXED24"]
    ref = O.render(spheres, X.DEFAULT_BG, st.as_array(), X.W, X.H, 64, X.DEPTH, X.RAY_RADIUS, seed, workers=4)
    assert np.isnan(ref[0]).any(axis=2).sum() >= 30
    has_bvh, plan, _ = paths_reported(L, spheres, st, 64, seed)
    assert has_bvh == 1 and plan["bvh"] == 0  # the linear scan's instance for such albedos
    assert plan["fixed_point_shift"] == 0 and plan["acc_slots"] == 0, plan
    X.assert_frames_match(device_frame(L, spheres, st, 64, seed), ref, case[0] + ", r = 64")
    X.assert_frames_match(device_frame(L, spheres, st, 64, seed, flags=L.FLAG_LINEAR_SCAN), ref,
                          case[0] + ", r = 64, linear scan")


WILD = [c for c in DEGENERATE if c[2] == "albedo" and not np.isfinite(c[4])]


@pytest.mark.parametrize("case", WILD, ids=[c[0] for c in WILD])
def test_infinite_or_nan_albedo_at_the_last_level(L, O, case):
    """Depth 2: most paths end black at the last level, many of them on the victim.
    Go scatters there too and multiplies the black by the albedo (NaN), unless the
    metal absorbs (0); r = 4 and r = 64 (no fixed-point sums without a colour bound)."""
    spheres = X.apply_case(case)
    st = X.camera_state(L, X.MIXED_SETUP)
    _, seed = X.RENDER["MIXED24"]
    for spp in (4, 64):
        ref = O.render(spheres, X.DEFAULT_BG, st.as_array(), X.W, X.H, spp, 2, X.RAY_RADIUS, seed, workers=4)
        assert np.isnan(ref[0]).any(axis=2).sum() >= 30
        X.assert_frames_match(device_frame(L, spheres, st, spp, seed, depth=2), ref, f"{case[0]}, r = {spp}")
        X.assert_frames_match(device_frame(L, spheres, st, spp, seed, flags=L.FLAG_LINEAR_SCAN, depth=2), ref,
                              f"{case[0]}, r = {spp}, linear scan")


@pytest.mark.parametrize("case", WILD, ids=[c[0] for c in WILD])
@pytest.mark.parametrize("how,flags", [("default", 0), ("linear", 1)])
def test_ray_color_with_an_infinite_or_nan_albedo(L, O, torch, case, how, flags):
    """Scene.RayColor for the frame's camera rays: an ended path's black is
    multiplied by the attenuations above it (inf * 0 = NaN * 0 = NaN, also at
    the last level when its material scatters), ray by ray as the oracle."""
    spheres = X.apply_case(case)
    st = X.camera_state(L, X.MIXED_SETUP)
    spp, seed = X.RENDER["MIXED24"]
    rays, ids = oracle_camera_rays(O, st.as_array(), X.W, range(X.H), spp, 0, X.RAY_RADIUS, seed)
    for depth in (X.DEPTH, 2):  # 2: most paths end at the last level, many of them on the victim
        want = [O.ray_color(spheres, X.DEFAULT_BG, r[:3], r[3:], depth, seed, int(i[0]), int(i[1]))
                for r, i in zip(rays, ids)]
        rgb = np.array([w[0] for w in want])
        seg = np.array([w[1] for w in want], dtype=np.uint32)
        black_nan = np.isnan(rgb).any(axis=1) & (seg == depth)
        assert black_nan.sum() >= (30 if depth == 2 else 1), (depth, int(black_nan.sum()))
        dev = L.DeviceScene(spheres, bg_struct(L, X.DEFAULT_BG), 0)
        try:
            got = device_colors(L, torch, dev, rays, depth, seed, ids, flags=flags)
        finally:
            dev.release()
        X.assert_frames_match(got, (rgb, seg), f"{case[0]}, {how}, depth {depth}")


# a zero-size box in the tree; finite but beyond the bound; NaN (both: no tree)
HIT_CASES = [c for c in DEGENERATE if c[0] in ("m2-radius=0", "m2-center1=1e200", "m2-center2=nan")]
assert len(HIT_CASES) == 3


@pytest.mark.parametrize("case", HIT_CASES, ids=[c[0] for c in HIT_CASES])
@pytest.mark.parametrize("how,flags", [("default", 0), ("linear", 1)])
def test_scene_hit_on_degenerate_geometry(L, O, torch, case, how, flags):
    """Scene.Hit for the frame's camera rays (sample 0) and for the rays that leave
    their hit points: records bit-equal to the oracle's."""
    spheres = X.apply_case(case)
    st = X.camera_state(L, X.MIXED_SETUP)
    spp, seed = X.RENDER["MIXED24"]
    rays = np.array([np.r_[o, d] for path in X.trace_sample(O, spheres, st.as_array(), spp, seed, 0)
                     for o, d, _ in path])
    want = oracle_hits(O, L, spheres, rays)
    assert len(rays) >= 2 * X.W * X.H and (want["index"] >= 0).sum() >= X.W * X.H
    dev = L.DeviceScene(spheres, bg_struct(L, X.DEFAULT_BG), 0)
    try:
        assert dev.info().has_bvh == X.expect_has_bvh(spheres)
        got = device_hits(L, torch, dev, rays, flags=flags)
    finally:
        dev.release()
    assert_hits_equal(got, want, f"{case[0]}, {how}")
