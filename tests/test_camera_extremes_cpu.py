"""Camera extremes on a scene that stays put (tests/camera_extremes.py), on the CPU:

1. the oracle's GetRay is a sound reference for every case (bit-equal to the numpy
   restatement of camera.go written from the Go source, tests/golden/make_golden.py);
2. every case is live or dead as camera_extremes says, so none silently stops hitting;
3. the primary-ray candidate bound (pixel_beam / beam_reaches, restated in
   tests/test_candidate_bound_cpu.py) holds every tree sphere the oracle's rays hit, or
   reports the beam unusable;
4. the FP32 slab cull (trav_begin32 and one box test of trav_node, restated here in
   numpy float32) never culls the box of a sphere the oracle's ray hits, nor the
   union box of the tree: the range argument at the top of tray_bvh.cpp, checked
   without a GPU.

3 and 4 carry a control each: the rule before the guards existed (any dn2 > 0
makes a list; every direction goes through the clamp) does drop hits on these cameras.
"""
import numpy as np
import pytest

import camera_extremes as C
import extremes as X
from test_candidate_bound_cpu import beam, beam_ok, camera_rays, hits, reaches

make_golden = X.make_golden


def case_param():
    return pytest.mark.parametrize("case", C.CASES, ids=C.IDS)


def tree_hits(O, L, case):
    """(ray index, sphere index) of the pixel-centre rays that hit a tree sphere."""
    h = C.centre_hits(O, L, case)
    tm = C.tree_mask(C.scene(case.scene))
    i = np.flatnonzero((h >= 0) & tm[np.maximum(h, 0)])
    return i, h[i]


# ------------------------------------------------------- 1. oracle soundness ----
@case_param()
def test_oracle_get_ray_is_the_numpy_restatement(O, L, case):
    s = case.setup
    with np.errstate(all="ignore"):
        cam = make_golden.camera_initialize(s[0:3], s[3:6], s[6:9], s[9], s[10], X.W, X.H, focus=s[11],
                                            aperture=s[12])
    st = C.camera_of(L, case).as_array()
    st_bits, cam_bits = np.asarray(st).view(np.uint64), cam.view(np.uint64)
    # a pinhole's lens vectors are SMul(u, 0): zeros of either sign, which nothing reads
    assert np.all((cam_bits == st_bits) | ((cam == 0) & (np.asarray(st) == 0))), "Camera.Initialize differs"
    rays, ids = C.frame_rays(O, L, case)
    got = np.empty_like(rays)
    with np.errstate(all="ignore"):
        for n, (pixel, sample) in enumerate(ids):
            off = O.in_disc(C.SEED, int(pixel), int(sample), 0, X.RAY_RADIUS) if case.r > 1 else (0.0, 0.0)
            lens = O.in_disc(C.SEED, int(pixel), int(sample), 1, 1.0) if s[12] > 0 else (0.0, 0.0)
            o, d = make_golden.get_ray(cam, float(pixel % X.W), float(pixel // X.W), off[0], off[1], lens)
            got[n] = (*o, *d)
    assert np.array_equal(got.view(np.uint64), rays.view(np.uint64)), \
        f"{int((got.view(np.uint64) != rays.view(np.uint64)).any(1).sum())} rays differ"
    # the pixel-centre rays of the liveness and soundness tests are sample 0's with no offset
    centre = C.centre_rays(O, L, case)
    if case.r == 1:
        assert np.array_equal(centre.view(np.uint64), rays.view(np.uint64))


# -------------------------------------------------------------- 2. liveness ----
@case_param()
def test_case_is_live_or_dead_as_stated(O, L, case):
    spheres = C.scene(case.scene)
    assert X.expect_has_bvh(spheres) == 1 and int(C.tree_mask(spheres).sum()) == 23
    n = len(tree_hits(O, L, case)[0])
    if case.live is True:
        assert n >= 100, f"{case.id}: only {n} pixel-centre rays hit a tree sphere"
    elif case.live is None:
        assert n >= 20, f"{case.id}: only {n} pixel-centre rays hit a tree sphere"
    else:
        assert n == 0, f"{case.id}: {n} hits although {case.why}"


def test_focal_length_one_hits_102(O, L):
    """The figure the liveness bound comes from; with a subnormal |d|^2 the reference hits more."""
    assert len(tree_hits(O, L, C.BY_ID["focal=2^0"])[0]) == 102
    assert len(tree_hits(O, L, C.BY_ID["focal=2^-537"])[0]) == X.W * X.H


# ---------------------------------------------- 3. candidate-bound soundness ----
def bound_misses(O, L, case, ok_rule):
    """[(pixel, sphere)] the oracle hits but the pixel's candidate set leaves out, over the
    pixels whose beam `ok_rule` accepts; and how many hits were checked against a set."""
    spheres = C.scene(case.scene)
    tm = C.tree_mask(spheres)
    tree_index = np.flatnonzero(tm)
    centers, radii = spheres["center"][tm], np.abs(spheres["radius"][tm])
    cam = C.camera_of(L, case)
    rays_i, sph = tree_hits(O, L, case)
    hit_of = dict(zip(rays_i.tolist(), sph.tolist()))
    rng = np.random.default_rng(11)
    missing, checked = [], 0
    with np.errstate(all="ignore"):
        for pixel in range(X.W * X.H):
            x, y = pixel % X.W, pixel // X.W
            if not ok_rule(cam, case.r, X.RAY_RADIUS, x, x, y, y):
                continue  # no list: the pixel's rays traverse
            cand = reaches(*beam(cam, case.r, X.RAY_RADIUS, x, x, y, y), centers, radii)
            want = np.zeros(len(centers), dtype=bool)
            if pixel in hit_of:
                want[np.searchsorted(tree_index, hit_of[pixel])] = True
            if case.r > 1:  # every ray the pixel can trace, sampled in both discs and on their rims
                org, dirs = camera_rays(cam, case.r, X.RAY_RADIUS, float(x), float(y), rng, 400)
                want |= hits(org, dirs, centers, radii).any(0)
            checked += int(want.sum())
            missing += [(pixel, int(tree_index[k])) for k in np.flatnonzero(want & ~cand)]
            # a tile's list must hold its pixels' lists
            xa, ya = x - x % 8, y - y % 8
            xb, yb = min(xa + 7, X.W - 1), min(ya + 7, X.H - 1)
            if ok_rule(cam, case.r, X.RAY_RADIUS, xa, xb, ya, yb):
                tile = reaches(*beam(cam, case.r, X.RAY_RADIUS, xa, xb, ya, yb), centers, radii)
                missing += [(pixel, int(tree_index[k])) for k in np.flatnonzero(want & ~tile)]
    return missing, checked


# cases whose beams are in range: the bound itself is what the test checks there
LISTS_BUILT = ("focal=2^-300", "focal=2^-100", "focal=2^0", "focal=2^20", "focal=2^-110-r4", "focal=2^0-r4",
               "lens-focal=2^-300", "lens-focal=2^100", "lens-focus=2^0", "lens-focus=2^20", "vfov=1.0", "vfov=340.0",
               "focal=-1", "focal=-2^-100", "cancel-focal=2^-40")


@case_param()
def test_every_hit_sphere_is_a_candidate_or_the_beam_is_refused(O, L, case):
    missing, checked = bound_misses(O, L, case, beam_ok)
    assert not missing, f"{case.id}: {len(missing)} (pixel, sphere) hits outside the candidate set, first {missing[0]}"
    if case.id in LISTS_BUILT:
        assert checked >= 100, (case.id, checked)  # lists were built and checked, not refused


def old_ok(cam, spp, ray_radius, xa, xb, ya, yb):
    """pixel_beam's rule before the range test: any axis with dn2 > 0 longer than twice the radii."""
    _, D, ra, rb = beam(cam, spp, ray_radius, xa, xb, ya, yb)
    dn2 = D @ D
    return bool(np.sqrt(dn2) > 2.0 * (ra + rb) and dn2 > 0)


@pytest.mark.parametrize("k", [-530, -532, -535, -537])
def test_control_the_bound_without_the_range_test_drops_hits(O, L, k):
    """Why beam_ok tests dn2: with a subnormal |D|^2 the same bound leaves hit spheres out."""
    missing, _ = bound_misses(O, L, C.BY_ID[f"focal=2^{k}"], old_ok)
    assert missing, k


# ---------------------------------------------------- 4. the FP32 slab cull ----
F = np.float32


def f32_down(v):
    f = np.asarray(v, dtype=np.float64).astype(F)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, F(-np.inf)), f)


def f32_up(v):
    f = np.asarray(v, dtype=np.float64).astype(F)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, F(np.inf)), f)


def padded_boxes(spheres):
    """tray_bvh.cpp: every tree sphere's box padded by 4e-6 M and rounded outward to float
    (M: the scene bound, at least 1, out-of-tree spheres included), and their union."""
    r = np.abs(spheres["radius"])[:, None]
    lo, hi = spheres["center"] - r, spheres["center"] + r
    m = max(1.0, float(np.abs(lo).max()), float(np.abs(hi).max()))
    pad = 4e-6 * m
    tm = C.tree_mask(spheres)
    blo, bhi = f32_down(lo - pad), f32_up(hi + pad)
    blo[~tm], bhi[~tm] = np.inf, -np.inf
    return blo, bhi, f32_down(lo[tm].min(0) - pad), f32_up(hi[tm].max(0) + pad)


def fma32(a, b, c):
    """fmaf for float32 operands: the product of two floats is exact in binary64 and the
    sum's binary64 rounding sits 29 bits below a float's, so the one place this can differ
    from the fused operation is a tie that the padding's 60 ulp do not care about."""
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def slab_dir_ok(dirs):
    """tray_device.hpp slab_dir_ok: 1e-30 <= |dir|^2 <= 1e30, with Sphere.Hit's own |dir|^2."""
    with np.errstate(all="ignore"):
        a = (dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2]
        return (a >= 1e-30) & (a <= 1e30)


def slab_setup(org, dirs):
    """trav_begin32: (inv, org * inv) per axis."""
    with np.errstate(all="ignore"):
        d = dirs.astype(F)
        d = np.where(np.abs(d) < F(1e-30), F(1e-30), d)
        inv = F(1.0) / d  # the device's reciprocal is within 1 ulp of this
        return inv, org.astype(F) * inv


def slab_enters(lo, hi, inv, oi, tlim):
    """trav_node's test of one box (lo, hi: (n, 3) float32) for n rays: not culled?"""
    near = np.where(inv < 0, hi, lo)
    far = np.where(inv < 0, lo, hi)
    tn3, tf3 = fma32(near, inv, -oi), fma32(far, inv, -oi)
    tn = np.fmax(np.fmax(np.fmax(tn3[:, 0], tn3[:, 1]), tn3[:, 2]), F(0.0))  # fmaxf / fminf drop a NaN
    tf = np.fmin(np.fmin(np.fmin(tf3[:, 0], tf3[:, 1]), tf3[:, 2]), tlim)
    return tn <= tf


def culled_hits(O, L, case, guard):
    """How many of the oracle's tree hits (pixel centres, plus every sample at r > 1) the
    restated slab test would cull: (from the sphere's own box, from the union box, hits,
    hits that reach the slab test). guard: a ray outside slab_dir_ok never reaches the
    slab test (the device tests every tree sphere in FP64 for it: the megakernel's refill,
    query_hit's linear scan); without it (the rule before) every ray does."""
    spheres = C.scene(case.scene)
    tm = C.tree_mask(spheres)
    blo, bhi, ulo, uhi = padded_boxes(spheres)
    rays = C.centre_rays(O, L, case)
    if case.r > 1:
        rays = np.concatenate([rays, C.frame_rays(O, L, case)[0]])
    recs = [O.scene_hit(spheres, r[:3], r[3:], 1e-6, np.inf) for r in rays]
    keep = np.array([i for i, (idx, _) in enumerate(recs) if idx >= 0 and tm[idx]], dtype=int)
    n_hits = len(keep)
    if guard and n_hits:
        keep = keep[slab_dir_ok(rays[keep, 3:])]
    if keep.size == 0:
        return 0, 0, n_hits, 0
    idx = np.array([recs[i][0] for i in keep])
    t = np.array([recs[i][1][6] for i in keep])
    inv, oi = slab_setup(rays[keep, :3], rays[keep, 3:])
    with np.errstate(all="ignore"):
        tlim = f32_up(t)  # the tightest culling distance the traversal can hold: the hit's own root
    own = int((~slab_enters(blo[idx], bhi[idx], inv, oi, tlim)).sum())
    union = int((~slab_enters(np.broadcast_to(ulo, inv.shape), np.broadcast_to(uhi, inv.shape), inv, oi, tlim)).sum())
    return own, union, n_hits, len(keep)


# live cases whose directions are inside slab_dir_ok: the slab test itself is what is checked there
SLAB_TESTED = ("focal=2^-40", "focal=2^0", "focal=2^20", "focal=2^0-r4", "lens-focal=2^-300", "lens-focal=2^100",
               "lens-focus=2^0", "lens-focus=2^20", "vfov=1e-300", "vfov=340.0", "focal=-1", "cancel-focal=2^-40")


@case_param()
def test_slab_cull_keeps_every_hit_box(O, L, case):
    own, union, n, tested = culled_hits(O, L, case, guard=True)
    assert (own, union) == (0, 0), f"{case.id}: of {tested} hits the slab test culls {own} from the sphere's own " \
                                   f"box, {union} from the union box"
    if case.live:
        assert n >= 100
    if case.id in SLAB_TESTED:
        assert tested == n >= 100, (case.id, tested, n)
    if case.id in ("focal=2^-84", "focal=2^-530", "lens-both=2^-110"):
        assert tested == 0 and n >= 20, (case.id, tested, n)  # every hit ray is outside the range


@pytest.mark.parametrize("k", [-100, -110, -120, -300])
def test_control_the_clamp_alone_culls_the_whole_tree(O, L, k):
    """Without slab_dir_ok the clamp turns every component into +1e-30: the sign is lost and
    the union box of the tree is rejected for every hit ray. At 2^-90 the clamp is not reached."""
    own, union, n, tested = culled_hits(O, L, C.BY_ID[f"focal=2^{k}"], guard=False)
    assert n == tested == 102 and union == 102 and own == 102
    assert culled_hits(O, L, C.BY_ID["focal=2^-90"], guard=False)[:2] == (0, 0)
