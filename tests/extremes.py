"""Scene and case builders for the FP64-range and degenerate-field tests
(tests/test_extremes_cpu.py, tests/test_gpu_extremes.py). No tests here.

Three 24-sphere scenes (24 >= kBvhMinSpheres, so the tree is built where the
upload accepts the scene), all rendered at 24 x 14:

MIRRORS24   make_golden.mirror_scene() plus 17 small mirrors: RNG-free (r = 1,
            pinhole, Metal{Fuzz: 0}), so make_golden.render_rngfree restates it.
ENCLOSED24  a cluster of metal spheres inside one concave mirror of radius 64.
            Rays that leave the cluster come back from a hit point on the
            enclosure: at 2^123 that point is beyond FLT_MAX while every
            cluster box is a finite float.
MIXED24     ground, the three large spheres of the book cover and 20 small ones
            around them: Lambertian, fuzzy metal and glass.

scaled() multiplies every length of a scene and its camera by 2^k, which is
exact in binary64 until a value leaves the normal range.
"""
import sys

import numpy as np

from conftest import GOLDEN, RICH_SETUP
from oracle.oracle import SPHERE_DTYPE

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_golden  # noqa: E402  (tests/golden/make_golden.py: the numpy restatement)

W, H, DEPTH = 24, 14, 12
RAY_RADIUS = 0.5
LAMBERTIAN, METAL, DIELECTRIC = 1, 2, 3

# 2^k for the sweep. 2^-530 squares to a subnormal, 2^511 squares to 2^1022 and
# 2^512 would overflow R*R; 127 / 128 / 130 straddle FLT_MAX = 2^128 (1 - 2^-24).
SCALES = (-530, -300, -100, -30, -20, -10, 0, 20, 64, 100, 127, 128, 130, 200, 400, 510, 511)
# ENCLOSED24 only. 122 / 123 / 124: the enclosure's radius 64 * 2^k crosses FLT_MAX.
# 22 / 23: it crosses 2^28, the largest scene bound the upload builds a tree for
# (BVH_MAX_BOUND below), so 22 is the largest mixed-magnitude scene the BVH traverses.
ENCLOSED_EXTRA_SCALES = (22, 23, 122, 123, 124)
ENCLOSED_SUSPECT = 123

MIRRORS_SETUP = np.array([0.3, 1.1, 3.2, 0.0, 0.5, 0.0, 0, 1, 0, 40.0, 1.0, 1.0, 0.0])
ENCLOSED_SETUP = np.array([0.3, 1.1, 6.0, 0.0, 0.8, 0.0, 0, 1, 0, 40.0, 1.0, 6.0, 0.05])
MIXED_SETUP = np.array(RICH_SETUP, dtype=np.float64)

# name -> (rays per pixel, seed)
RENDER = {"MIRRORS24": (1, 1), "ENCLOSED24": (4, 5), "MIXED24": (4, 7)}


def mirrors24():
    base = make_golden.mirror_scene()
    rng = np.random.default_rng(3)
    s = np.zeros(24, dtype=SPHERE_DTYPE)
    s[:7] = base
    n = 17
    x = rng.uniform(-2.5, 2.5, n)
    z = rng.uniform(-2.5, 2.5, n)
    s["center"][7:] = np.stack([x, np.full(n, 0.15), z], axis=1)
    s["radius"][7:] = 0.15
    s["albedo"][7:] = rng.uniform(0.3, 0.95, (n, 3))
    s["material"] = METAL
    return s


def enclosed24():
    rng = np.random.default_rng(3)
    s = np.zeros(24, dtype=SPHERE_DTYPE)
    s["material"] = METAL
    s[0]["center"], s[0]["radius"], s[0]["albedo"] = (0.0, 0.0, 0.0), 64.0, (0.9, 0.9, 0.9)
    n = 23
    x = rng.uniform(-2.5, 2.5, n)
    y = rng.uniform(0.1, 2.0, n)
    z = rng.uniform(-2.5, 2.5, n)
    s["center"][1:] = np.stack([x, y, z], axis=1)
    s["radius"][1:] = rng.uniform(0.2, 0.6, n)
    s["param"][1:] = rng.choice([0.0, 1.0, 1.5], n)
    s["albedo"][1:] = rng.uniform(0.3, 0.95, (n, 3))
    return s


VICTIM = 3  # MIXED24's front large sphere at (4, 1, 0)


def mixed24():
    rng = np.random.default_rng(24)
    s = np.zeros(24, dtype=SPHERE_DTYPE)
    s[0] = ((0.0, -1000.0, 0.0), 1000.0, (0.5, 0.5, 0.5), 0.0, LAMBERTIAN, 0)
    s[1] = ((0.0, 1.0, 0.0), 1.0, (0.0, 0.0, 0.0), 1.5, DIELECTRIC, 0)
    s[2] = ((-4.0, 1.0, 0.0), 1.0, (0.4, 0.2, 0.1), 0.0, LAMBERTIAN, 0)
    s[VICTIM] = ((4.0, 1.0, 0.0), 1.0, (0.7, 0.6, 0.5), 0.0, METAL, 0)
    n = 20
    # the stretch of ground the book-cover camera sees in front of and beside the large spheres
    s["center"][4:] = np.stack([rng.uniform(-3.0, 8.0, n), np.full(n, 0.2), rng.uniform(-2.5, 3.5, n)], axis=1)
    s["radius"][4:] = 0.2
    s["albedo"][4:] = rng.uniform(0.1, 0.95, (n, 3))
    kinds = np.arange(n) % 3
    s["material"][4:] = np.choose(kinds, [LAMBERTIAN, METAL, DIELECTRIC])
    s["param"][4:] = np.choose(kinds, [0.0, 0.3, 1.5])
    return s


SCENES = {"MIRRORS24": (mirrors24, MIRRORS_SETUP), "ENCLOSED24": (enclosed24, ENCLOSED_SETUP),
          "MIXED24": (mixed24, MIXED_SETUP)}


def scales_of(name):
    return tuple(sorted(SCALES + (ENCLOSED_EXTRA_SCALES if name == "ENCLOSED24" else ())))


def scaled(scene, setup, k):
    """Centres, radii, camera position and look-at, focal length, focus distance
    and aperture times 2^k. Up, the field of view and the materials stay."""
    f = np.ldexp(1.0, k)
    s = scene.copy()
    s["center"] *= f
    s["radius"] *= f
    t = np.array(setup, dtype=np.float64)
    t[0:6] *= f
    t[10:13] *= f
    return s, t


# --------------------------------------------------------- degenerate fields --
# The victim's fields before a case changes one, per material: values every case
# below differs from, so that each case can be seen in the frame.
VICTIM_BASE = {
    LAMBERTIAN: dict(albedo=(0.7, 0.6, 0.5), param=0.0),
    METAL: dict(albedo=(0.7, 0.6, 0.5), param=0.5),
    DIELECTRIC: dict(albedo=(0.7, 0.6, 0.5), param=1.5),
}

DENORM_MIN = 5e-324
RADII = (0.0, -0.0, DENORM_MIN, 1e-200, 1e200, np.inf, -np.inf, np.nan)
CENTERS = ((0, np.inf), (1, -np.inf), (2, np.nan), (1, 1e200))  # (component, value)
PARAMS = (0.0, -1.0, np.inf, np.nan, DENORM_MIN)
ALBEDOS = ((0, 0.0), (1, -0.5), (2, np.inf), (0, np.nan))       # (component, value)


def _tag(v):
    if v != v:
        return "nan"
    if v == 0:
        return "-0" if np.signbit(v) else "0"
    return repr(float(v)).replace("+", "")


def victim_scene(material):
    s = mixed24()
    s[VICTIM]["material"] = material
    s[VICTIM]["albedo"] = VICTIM_BASE[material]["albedo"]
    s[VICTIM]["param"] = VICTIM_BASE[material]["param"]
    return s


def degenerate_cases():
    """[(id, material, field, component-or-None, value)]. Geometry cases run for
    every material. A field that the material never reads cannot show in a frame
    (Lambertian reads no param, Dielectric no albedo), so those pairs are left out."""
    out = []
    for m in (LAMBERTIAN, METAL, DIELECTRIC):
        for v in RADII:
            out.append((f"m{m}-radius={_tag(v)}", m, "radius", None, v))
        for c, v in CENTERS:
            out.append((f"m{m}-center{c}={_tag(v)}", m, "center", c, v))
        if m != LAMBERTIAN:
            for v in PARAMS:
                out.append((f"m{m}-param={_tag(v)}", m, "param", None, v))
        if m != DIELECTRIC:
            for c, v in ALBEDOS:
                out.append((f"m{m}-albedo{c}={_tag(v)}", m, "albedo", c, v))
    return out


def apply_case(case):
    """The MIXED24 scene of a degenerate case."""
    _, m, field, comp, v = case
    s = victim_scene(m)
    if comp is None:
        s[VICTIM][field] = v
    else:
        s[field][VICTIM, comp] = v
    return s


def is_geometry(case):
    return case[2] in ("radius", "center")


def nonfinite_geometry(case):
    return is_geometry(case) and not np.isfinite(case[4])


# ------------------------------------------------------------ comparison rule --
def value_class(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def assert_frames_match(got, ref, what, tol=1e-12):
    """The comparison rule: per-pixel Scene.Hit counts equal; non-finite colour
    entries equal in class and sign; finite ones within tol * max(1, |ref|)
    (the attenuation product order is the one permitted difference)."""
    (rgb, seg), (rrgb, rseg) = got, ref
    assert rgb.shape == rrgb.shape and seg.shape == rseg.shape, what
    bad = seg != rseg
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels took different paths, first {np.argwhere(bad)[0]}: " \
                          f"{seg[bad][0]} for {rseg[bad][0]}"
    cls, rcls = value_class(rgb), value_class(rrgb)
    assert np.array_equal(cls, rcls), f"{what}: {int((cls != rcls).sum())} entries differ in finite/inf/NaN class"
    fin = rcls == 0
    if fin.any():
        err = np.abs(rgb[fin] - rrgb[fin]) / np.maximum(1.0, np.abs(rrgb[fin]))
        assert float(err.max()) <= tol, f"{what}: colour error {float(err.max()):.3e}"


def bit_identical(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------- oracle tracing --
def trace_sample(O, spheres, cam, spp, seed, sample=0, depth=DEPTH, width=W, height=H):
    """One sample of every pixel, segment by segment, through the oracle's
    GetRay / Scene.Hit / Scatter. Returns one list per pixel of
    (origin, direction, hit index) with index -1 for a miss."""
    paths = []
    for y in range(height):
        for x in range(width):
            pixel = y * width + x
            off = O.in_disc(seed, pixel, sample, 0, RAY_RADIUS) if spp > 1 else (0.0, 0.0)
            o, d = O.get_ray(cam, float(x), float(y), off[0], off[1], seed, pixel, sample)
            path = []
            for bounce in range(depth):
                idx, rec = O.scene_hit(spheres, o, d, 1e-6, np.inf)
                path.append((o, d, idx))
                if idx < 0:
                    break
                ok, _, o2, d2 = O.scatter(spheres[idx:idx + 1], o, d, rec[0:3], rec[3:6], rec[7], seed, pixel,
                                          sample, bounce)
                if not ok:
                    break
                o, d = o2, d2
            paths.append(path)
    return paths


def enclosure_returns(paths, enclosure=0):
    """The segments that start at a hit point on the enclosure and hit a cluster
    sphere next: [(origin, direction)]."""
    out = []
    for path in paths:
        for a, b in zip(path, path[1:]):
            if a[2] == enclosure and b[2] > enclosure:
                out.append(np.r_[b[0], b[1]])
    return out


# ------------------------------------------------- shared cases and references --
DEFAULT_BG = np.array([1.0, 1.0, 1.0, 0.4, 0.65, 1.0])
_cache = {}


def camera_state(L, setup, width=W, height=H):
    """tray_camera_initialize (host only): the camera both the device and the references get."""
    import ctypes

    d3 = ctypes.c_double * 3
    cs = L.CameraSetup(d3(*setup[0:3]), d3(*setup[3:6]), d3(*setup[6:9]), *[float(v) for v in setup[9:13]])
    st = L.CameraState()
    L.check(L.lib().tray_camera_initialize(ctypes.byref(cs), width, height, ctypes.byref(st)))
    return st


def scene_at(L, name, k):
    """(spheres, camera state) of a named scene at 2^k; computed once, not to be written to."""
    key = ("scene", name, k)
    if key not in _cache:
        make, setup = SCENES[name]
        s, t = scaled(make(), setup, k)
        _cache[key] = (s, camera_state(L, t))
    return _cache[key]


def oracle_frame(O, L, name, k, spp=None):
    """The oracle's (rgb, segments) of a named scene at 2^k; computed once and shared."""
    rays, seed = RENDER[name]
    spp = rays if spp is None else spp
    key = ("oracle", name, k, spp)
    if key not in _cache:
        s, st = scene_at(L, name, k)
        _cache[key] = O.render(s, DEFAULT_BG, st.as_array(), W, H, spp, DEPTH, RAY_RADIUS, seed, workers=4)
    return _cache[key]


def numpy_frame(L, k):
    """MIRRORS24 at 2^k through make_golden.render_rngfree, with the camera state
    of tray_camera_initialize (make_golden.camera_initialize lacks Go's
    NearZero(viewDirection) default, camera.go:67, which fires at small scales)."""
    key = ("numpy", k)
    if key not in _cache:
        s, st = scene_at(L, "MIRRORS24", k)
        with np.errstate(all="ignore"):
            _cache[key] = make_golden.render_rngfree(s, st.as_array(), W, H, DEPTH, DEFAULT_BG)
    return _cache[key]


def degenerate_frame(O, L, case_or_material):
    """The oracle's frame of a degenerate case, or of the unmodified victim scene of a material."""
    key = ("degenerate", case_or_material if isinstance(case_or_material, int) else case_or_material[0])
    if key not in _cache:
        s = victim_scene(case_or_material) if isinstance(case_or_material, int) else apply_case(case_or_material)
        spp, seed = RENDER["MIXED24"]
        st = camera_state(L, MIXED_SETUP)
        _cache[key] = O.render(s, DEFAULT_BG, st.as_array(), W, H, spp, DEPTH, RAY_RADIUS, seed, workers=4)
    return _cache[key]


# ----------------------------------------------------------- host decisions --
# tray_scene_upload builds the tree iff every coordinate and radius is finite and
# every sphere box lies within +-2^28 (kBvhMaxBound, tray_amd/csrc/bvh.hpp; the
# derivation is at the top of tray_bvh.cpp); anything else takes the linear scan,
# and without a tree a render has no candidate lists either. A scene with an
# infinite or NaN albedo keeps its tree for Scene.Hit queries but renders through
# the linear scan (tray_render_plan_get().bvh == 0).
BVH_MAX_BOUND = 2.0 ** 28


def expect_has_bvh(spheres):
    r = np.abs(spheres["radius"])[:, None]
    with np.errstate(invalid="ignore"):
        reach = np.maximum(np.abs(spheres["center"] - r), np.abs(spheres["center"] + r))
    return int(len(spheres) >= 16 and bool(np.all(reach <= BVH_MAX_BOUND)))  # NaN compares false


# The largest k of each scene's sweep that still has a tree, written out so a
# reader sees which path each scale ran (2000 * 2^17 < 2^28 < 2000 * 2^18 for the
# ground spheres of radius 1000 centred 1000 below; 64 * 2^22 = 2^28 for the
# enclosure): k at or below it renders through the BVH and the candidate lists,
# k above it through the linear scan.
LAST_BVH_SCALE = {"MIRRORS24": 0, "ENCLOSED24": 22, "MIXED24": 0}
