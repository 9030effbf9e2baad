"""FP64-range extremes and degenerate scene data, the part that needs no device
(tests/extremes.py builds the scenes; tests/test_gpu_extremes.py runs them on
the device).

1. The oracle is a sound reference at every scale: on the RNG-free MIRRORS24 it
   equals the independent numpy restatement (tests/golden/make_golden.py) bit
   for bit from 2^-530 to 2^511.
2. Liveness: the scenes do what the GPU tests rely on. ENCLOSED24 at 2^123 sends
   rays from beyond FLT_MAX into a cluster within float range; every degenerate
   field changes the frame.
3. The host decisions (tree or linear scan) the GPU tests assert, checked here
   against the documented rule. tray_scene_upload itself needs a device.
"""
import numpy as np
import pytest

import extremes as X

FLT_MAX = float(np.finfo(np.float32).max)


# ----------------------------------------------- 1. oracle == numpy restatement --
@pytest.mark.parametrize("k", X.SCALES)
def test_oracle_equals_numpy_restatement_at_scale(O, L, k):
    rgb, seg = X.oracle_frame(O, L, "MIRRORS24", k)
    img, nseg = X.numpy_frame(L, k)
    assert np.array_equal(seg, nseg), f"2^{k}: {int((seg != nseg).sum())} pixels took different paths"
    nan = np.isnan(rgb)
    assert np.array_equal(nan, np.isnan(img)), f"2^{k}: NaN in different places"
    assert np.array_equal(rgb[~nan].view(np.uint64), img[~nan].view(np.uint64)), \
        f"2^{k}: max difference {np.nanmax(np.abs(rgb - img))}"
    # what the scale does to the frame (so that each k is known to test something)
    print(f"2^{k}: segments {int(seg.min())}..{int(seg.max())}, {len(np.unique(seg))} distinct, "
          f"{int(np.isfinite(rgb).all(axis=2).sum())} of {seg.size} pixels finite")
    if 20 <= k <= 200:  # ordinary paths, up to the depth cap
        assert seg.max() == X.DEPTH and len(np.unique(seg)) >= 10
    if k >= 400:  # |direction|^2 overflows: nothing is hit, every path is its camera ray
        assert seg.max() == 1
    if k <= -100:  # t * direction underflows against the hit epsilon 1e-6: at most one reflection
        assert seg.max() <= 2
    if k >= 511:
        assert not np.isfinite(rgb).any()
    else:
        assert np.isfinite(rgb).all()


def test_camera_state_is_the_oracles_at_every_scale(O, L):
    """tray_camera_initialize and the oracle's Camera.Initialize give the same 21
    doubles for every scene and scale of the sweep (the GPU tests hand the
    library's to both sides)."""
    for name, (_, setup) in X.SCENES.items():
        for k in X.scales_of(name):
            _, t = X.scaled(np.zeros(0, dtype=X.SPHERE_DTYPE), setup, k)
            got = X.camera_state(L, t).as_array()
            _, want = O.camera_initialize(t, X.W, X.H)
            assert got.tobytes() == want.tobytes(), (name, k)


# ------------------------------------------------------------- 2. liveness ------
@pytest.fixture(scope="module")
def enclosed_trace(O, L):
    spp, seed = X.RENDER["ENCLOSED24"]
    s, st = X.scene_at(L, "ENCLOSED24", X.ENCLOSED_SUSPECT)
    return [X.trace_sample(O, s, st.as_array(), spp, seed, sample) for sample in range(spp)]


def test_trace_counts_the_oracles_segments(O, L, enclosed_trace):
    """The segment-by-segment trace (GetRay, Scene.Hit, Scatter) walks the paths
    of the oracle's own frame: same Scene.Hit count in every pixel."""
    _, seg = X.oracle_frame(O, L, "ENCLOSED24", X.ENCLOSED_SUSPECT)
    mine = np.sum([[len(p) for p in paths] for paths in enclosed_trace], axis=0).reshape(X.H, X.W)
    assert np.array_equal(mine, seg)


def test_enclosed24_sends_rays_from_beyond_float_into_the_cluster(O, L, enclosed_trace):
    k = X.ENCLOSED_SUSPECT
    s, _ = X.scene_at(L, "ENCLOSED24", k)
    assert s["radius"][0] == 2.0 ** 129 > FLT_MAX
    assert float((np.abs(s["center"][1:]) + s["radius"][1:, None]).max()) < 2.0 ** 126 < FLT_MAX
    returns = X.enclosure_returns(enclosed_trace[0])
    _, seg = X.oracle_frame(O, L, "ENCLOSED24", k)
    distinct = len(np.unique(seg))
    print(f"ENCLOSED24 at 2^{k}: {len(returns)} segments of sample 0 leave the enclosure and hit a cluster sphere; "
          f"{distinct} distinct per-pixel Scene.Hit counts")
    assert len(returns) >= 50
    assert distinct >= 20
    # each of them starts where FP32 has no finite value
    assert all(np.abs(r[:3]).max() > FLT_MAX for r in returns)
    # and the same paths exist at 2^22, the largest scale the tree is built for
    s22, st22 = X.scene_at(L, "ENCLOSED24", X.LAST_BVH_SCALE["ENCLOSED24"])
    spp, seed = X.RENDER["ENCLOSED24"]
    r22 = X.enclosure_returns(X.trace_sample(O, s22, st22.as_array(), spp, seed, 0))
    print(f"ENCLOSED24 at 2^{X.LAST_BVH_SCALE['ENCLOSED24']}: {len(r22)} such segments")
    assert len(r22) >= 50


DEGENERATE = X.degenerate_cases()


@pytest.mark.parametrize("case", DEGENERATE, ids=[c[0] for c in DEGENERATE])
def test_degenerate_case_changes_the_frame(O, L, case):
    rgb, _ = X.degenerate_frame(O, L, case)
    base, _ = X.degenerate_frame(O, L, case[1])
    same = (rgb == base) | (np.isnan(rgb) & np.isnan(base))
    changed = int((~same).any(axis=2).sum())
    print(f"{case[0]}: {changed} of {X.W * X.H} pixels differ from the unmodified scene")
    assert changed >= 30


def test_degenerate_cases_cover_the_listed_values():
    assert len(DEGENERATE) == 3 * (len(X.RADII) + len(X.CENTERS)) + 2 * len(X.PARAMS) + 2 * len(X.ALBEDOS)
    assert len({c[0] for c in DEGENERATE}) == len(DEGENERATE)
    v = X.mixed24()[X.VICTIM]
    assert tuple(v["center"]) == (4.0, 1.0, 0.0) and v["radius"] == 1.0


# ------------------------------------------------------- 3. host decisions ------
def test_which_scales_have_a_tree(L):
    """LAST_BVH_SCALE (what the GPU tests assert of tray_scene_get_info and
    tray_render_plan_get) is the documented rule applied to the scaled scenes:
    every sphere box within +-2^28."""
    for name in X.SCENES:
        has = {k: X.expect_has_bvh(X.scene_at(L, name, k)[0]) for k in X.scales_of(name)}
        assert has == {k: int(k <= X.LAST_BVH_SCALE[name]) for k in X.scales_of(name)}, name
    # the scenes the project is measured on keep theirs
    from oracle import oracle

    assert X.expect_has_bvh(oracle.rich_scene(2)) == 1


def test_which_degenerate_cases_have_a_tree():
    """Non-finite geometry and finite geometry beyond the bound: linear scan.
    Zero, subnormal and tiny radii, and every material field: the tree."""
    for case in DEGENERATE:
        v = case[4]
        beyond = X.is_geometry(case) and not (abs(v) <= X.BVH_MAX_BOUND)
        assert X.expect_has_bvh(X.apply_case(case)) == int(not beyond), case[0]
        if X.nonfinite_geometry(case):
            assert beyond
