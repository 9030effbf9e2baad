"""Case builders for the camera-extreme tests (tests/test_camera_extremes_cpu.py,
tests/test_gpu_camera_extremes.py). No tests here.

tests/extremes.py scales the camera together with its scene, so a camera ray's
direction there keeps a length of order one relative to the scene. Here the
scene stays put and the camera alone goes to extremes: Go sets the length of a
camera ray freely (pinhole: rayDirection = pixelSample - Position, proportional
to FocalLength; lens: about FocusDistance), Sphere.Hit does not care, and the
device's FP32 slab cull (trav_begin32) and its candidate bound (pixel_beam) must
not care either.

Scene: extremes.mixed24() moved by -(13, 2, 3), so that the book-cover camera
sits at the origin (a camera away from the origin rounds pixel00 onto its
position long before the focal length gets interesting; that is the
"cancel" family below, on the unmoved scene). 24 spheres, the ground out of
the tree. Frame: extremes.W x extremes.H, depth extremes.DEPTH.

A case is live when the oracle's pixel-centre rays hit tree spheres (at least
100 of them: 102 at focal length 1) and dead when they hit none; the CPU tests
assert which, so a case cannot silently stop testing anything.
"""
from collections import namedtuple

import numpy as np

import extremes as X

SHIFT = np.array([13.0, 2.0, 3.0])
SEED = 7
OVERFLOW_RADIUS = 30.0  # with r = 4: every pixel's disc covers the frame, so every candidate list overflows

# setup layout: pos3, look_at3, up3, vfov, focal, focus, aperture
BASE = np.array([0, 0, 0, -13, -2, -3, 0, 1, 0, 20.0, 1.0, 0.0, 0.0])

# id, scene ("moved" / "unmoved"), setup, rays per pixel, live, why a dead case hits nothing
Case = namedtuple("Case", "id scene setup r live why")

FOCAL_K = (-1000, -540, -537, -535, -532, -530, -525, -512, -300, -120, -110, -100, -90, -84, -80, -40, 0, 10, 20,
           25, 60, 126, 127, 128, 130, 511, 600)
FOCAL_R4_K = (-535, -530, -110, -84, 0)
LENS_FOCAL_K = (-300, -100, -40, 0, 40, 100)
FOCUS_K = (-300, -100, -10, 0, 4, 10, 20, 40, 100)
VFOV = (1e-300, 1e-9, 1.0, 179.0, 179.9999999, 180.0, 181.0, 340.0, -20.0)
VFOV_LIVE = (1e-300, 1e-9, 1.0, 340.0, -20.0)
CANCEL_K = (-60, -40, 0)

UNDERFLOW = "|d|^2 underflows to 0: every root is infinite or NaN"
TOO_LONG = "every root t is below Interval.Start = 1e-6"
AWAY = "the rays point away from the scene"


def _setup(**kw):
    s = BASE.copy()
    for k, v in kw.items():
        i = {"pos": slice(0, 3), "look": slice(3, 6), "vfov": 9, "focal": 10, "focus": 11, "aperture": 12}[k]
        s[i] = v
    return s


def _p2(k):
    return float(np.ldexp(1.0, k))


def cases():
    out = []
    for k in FOCAL_K:
        live = -537 <= k <= 20
        out.append(Case(f"focal=2^{k}", "moved", _setup(focal=_p2(k)), 1, live,
                        None if live else UNDERFLOW if k < 0 else TOO_LONG))
    for k in FOCAL_R4_K:
        out.append(Case(f"focal=2^{k}-r4", "moved", _setup(focal=_p2(k)), 4, True, None))
    for k in LENS_FOCAL_K:  # the direction's length stays about the focus distance; focus time 10 * 2^-k
        out.append(Case(f"lens-focal=2^{k}", "moved", _setup(focal=_p2(k), focus=10.0, aperture=0.1), 4, True, None))
    for k in FOCUS_K:
        live = 0 <= k <= 20
        out.append(Case(f"lens-focus=2^{k}", "moved", _setup(focus=_p2(k), aperture=0.1), 4, live,
                        None if live else "the lens offset outweighs the focus point: the rays leave sideways"
                        if k < 0 else TOO_LONG))
    # A lens camera whose directions are below the FP32 clamp. The lens radius is half the focus
    # distance, so the rays fan out by up to 27 degrees and only some reach the scene: live = None
    # (the centre rays hit 26 tree spheres; at least 20 are asked for).
    out.append(Case("lens-both=2^-110", "moved", _setup(focus=_p2(-110), aperture=_p2(-110)), 4, None, None))
    for v in VFOV:
        live = v in VFOV_LIVE
        out.append(Case(f"vfov={v!r}", "moved", _setup(vfov=v), 1, live,
                        None if live else "no pixel centre lies within the scene's few degrees"))
    # Go accepts negative lengths: a negative focal length puts the viewport behind the camera
    out.append(Case("focal=-1", "moved", _setup(look=SHIFT, focal=-1.0), 1, True, None))
    out.append(Case("focal=-2^-100", "moved", _setup(look=SHIFT, focal=-_p2(-100)), 1, True, None))
    out.append(Case("lens-focus=-10", "moved", _setup(focus=-10.0, aperture=0.1), 4, False, AWAY))
    for k in CANCEL_K:  # the unmoved scene: pixel00 = position - w * focal + ... rounds at ulp(13) = 2^-49
        s = np.array([*X.MIXED_SETUP[:3], 0, 0, 0, 0, 1, 0, 20.0, _p2(k), 0.0, 0.0])
        out.append(Case(f"cancel-focal=2^{k}", "unmoved", s, 1, k >= -40,
                        "pixel00 rounds onto the position: every direction is the zero vector" if k < -40 else None))
    return out


CASES = cases()
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}

_cache = {}


def overflow_radii(case):
    """The anti-aliasing radii of a case's render with overflowing lists; the overflow is
    asserted at the last. 30 pixels cover the 24 x 14 frame, and at 20 degrees the frame
    shows more spheres than a list holds. A view of 1 or 1e-9 degrees shows one or two
    spheres however many of its own pixels the disc covers, so nothing overflows there: those
    two cases also render with a disc of the same angle as 30 pixels at 20 degrees."""
    if case.id in ("vfov=1e-09", "vfov=1.0"):
        return (OVERFLOW_RADIUS, OVERFLOW_RADIUS * 20.0 / case.setup[9])
    return (OVERFLOW_RADIUS,)


def scene(which):
    """The 24 spheres of a case; computed once, not to be written to."""
    if which not in _cache:
        s = X.mixed24()
        if which == "moved":
            s["center"] -= SHIFT
        _cache[which] = s
    return _cache[which]


def tree_mask(spheres):
    """The spheres in the tree: all but the ground (kBvhGlobals, tray_bvh.cpp)."""
    return np.abs(spheres["radius"]) < 100.0


def camera_of(L, case):
    key = ("cam", case.id)
    if key not in _cache:
        _cache[key] = X.camera_state(L, case.setup)
    return _cache[key]


def centre_rays(O, L, case):
    """The oracle's rays through the pixel centres (sample word 0; a lens camera's
    lens point is that word's draw): (W * H, 6), rows first."""
    key = ("centre", case.id)
    if key not in _cache:
        cam = camera_of(L, case).as_array()
        rays = []
        for y in range(X.H):
            for x in range(X.W):
                o, d = O.get_ray(cam, float(x), float(y), 0.0, 0.0, SEED, y * X.W + x, 0)
                rays.append(np.r_[o, d])
        _cache[key] = np.array(rays)
    return _cache[key]


def frame_rays(O, L, case, r=None, radius=X.RAY_RADIUS):
    """What RenderLines traces for the case's frame: (rays (n, 6), ids (n, 2)), pass 0."""
    r = case.r if r is None else r
    key = ("rays", case.id, r, radius)
    if key not in _cache:
        cam = camera_of(L, case).as_array()
        rays, ids = [], []
        for pixel in range(X.W * X.H):
            for s in range(r):
                off = O.in_disc(SEED, pixel, s, 0, radius) if r > 1 else (0.0, 0.0)
                o, d = O.get_ray(cam, float(pixel % X.W), float(pixel // X.W), off[0], off[1], SEED, pixel, s)
                rays.append(np.r_[o, d])
                ids.append((pixel, s))
        _cache[key] = (np.array(rays), np.array(ids, dtype=np.uint32))
    return _cache[key]


def hit_indices(O, spheres, rays):
    """Scene.Hit's sphere index per ray (-1: a miss), from the oracle."""
    return np.array([O.scene_hit(spheres, r[:3], r[3:], 1e-6, np.inf)[0] for r in rays])


def centre_hits(O, L, case):
    key = ("centre-hits", case.id)
    if key not in _cache:
        _cache[key] = hit_indices(O, scene(case.scene), centre_rays(O, L, case))
    return _cache[key]


def oracle_frame(O, L, case, r=None, radius=X.RAY_RADIUS):
    """The oracle's (rgb, segments) of the case's frame; computed once and shared."""
    r = case.r if r is None else r
    key = ("frame", case.id, r, radius)
    if key not in _cache:
        _cache[key] = O.render(scene(case.scene), X.DEFAULT_BG, camera_of(L, case).as_array(), X.W, X.H, r, X.DEPTH,
                               radius, SEED, workers=4)
    return _cache[key]
