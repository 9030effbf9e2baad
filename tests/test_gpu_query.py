"""Batched ray queries (include/tray_query.h) on the device against the oracle's
restatement of Camera.GetRay, Scene.Hit and Scene.RayColor, and against the
unchanged megakernel.

Contract: camera rays and hit records are the reference's bits (tray.h's
arithmetic contract); path decisions (Scene.Hit counts) are exact; colours
differ from the oracle by the attenuation product order only (outer-first on the
device, inner-first in Go's recursion), and from the megakernel not at all.
"""
import ctypes

import numpy as np
import pytest

from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_parity import bg_struct, camera

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the project's parity gate (BASELINE.json)
INF = float("inf")
PINHOLE_SETUP = np.r_[RICH_SETUP[:12], 0.0]

# test 1's row set: rows 2..15 in 2-row tiles, every third tile from the second -> rows 4, 5, 10, 11
W1, H1, SEED1, PASS1, RADIUS1 = 33, 17, 21, 2, 0.5
TILES1 = dict(y_start=2, y_end=15, tile_rows=2, tile_count=3, tile_index=1)
ROWS1 = [4, 5, 10, 11]


# ------------------------------------------------------------------ helpers --
def oracle_camera_rays(O, cam, w, rows, r, pass_, radius, seed):
    """What RenderLines traces: (n, 6) rays and (n, 2) ids in (row, column, sample) order."""
    rays, ids = [], []
    for y in rows:
        for x in range(w):
            for s in range(r):
                pixel, word = y * w + x, pass_ * r + s
                off = O.in_disc(seed, pixel, word, 0, radius) if r > 1 else (0.0, 0.0)
                o, d = O.get_ray(cam, float(x), float(y), off[0], off[1], seed, pixel, word)
                rays.append(np.r_[o, d])
                ids.append((pixel, word))
    return np.array(rays), np.array(ids, dtype=np.uint32)


def device_camera_rays(L, torch, st, params):
    n = L.camera_rays_count(params)
    rays = torch.full((n, 6), float("nan"), dtype=torch.float64, device="cuda")
    ids = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    L.camera_rays_async(st, params, rays.data_ptr(), ids.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    return rays, ids


def device_hits(L, torch, dev, rays, t_end=INF, flags=0, stream=None):
    r = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)).cuda()
    h = torch.full((len(r), 8), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.current_stream().synchronize()
    dev.hit_async(r.data_ptr(), len(r), h.data_ptr(), t_end, flags,
                  (stream or torch.cuda.current_stream()).cuda_stream)
    torch.cuda.synchronize()
    return h.cpu().numpy().reshape(-1).view(L.HIT_DTYPE)


def device_colors(L, torch, dev, rays, depth, seed, ids=None, flags=0):
    r = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)).cuda()
    i = None if ids is None else torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).view(np.int32)).cuda()
    rgb = torch.full((len(r), 3), float("nan"), dtype=torch.float64, device="cuda")
    seg = torch.zeros(len(r), dtype=torch.int32, device="cuda")
    dev.ray_color_async(r.data_ptr(), len(r), depth, seed, rgb.data_ptr(), None if i is None else i.data_ptr(),
                        seg.data_ptr(), flags, torch.cuda.current_stream().cuda_stream)
    return rgb.cpu().numpy(), seg.cpu().numpy().view(np.uint32)


def oracle_hits(O, L, spheres, rays, t_end=INF):
    out = np.zeros(len(rays), dtype=L.HIT_DTYPE)
    out["index"] = -1
    for i, r in enumerate(np.asarray(rays, dtype=np.float64).reshape(-1, 6)):
        idx, rec = O.scene_hit(spheres, r[:3], r[3:], 1e-6, t_end)
        if idx >= 0:
            out[i] = (rec[0:3], rec[3:6], rec[6], idx, int(rec[7]))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_hits_equal(got, want, what):
    bad = np.nonzero(got["index"] != want["index"])[0]
    assert bad.size == 0, f"{what}: {bad.size} rays hit another sphere, first ray {bad[:1]}: " \
                          f"{got['index'][bad[:1]]} for {want['index'][bad[:1]]}"
    assert np.array_equal(got["front_face"], want["front_face"]), what
    for f in ("t", "point", "normal"):
        g, w = got[f], want[f]
        assert np.array_equal(bits(g), bits(w)), f"{what}: {f} differs, max {np.nanmax(np.abs(g - w))}"
    # a miss is all zeros
    miss = got["index"] < 0
    assert not got["t"][miss].any() and not got["point"][miss].any() and not got["normal"][miss].any(), what


# ----------------------------------------------------------------- fixtures --
@pytest.fixture(scope="module")
def torch():
    import torch

    torch.cuda.init()
    return torch


@pytest.fixture(scope="module")
def rich2(O):
    return O.rich_scene(2)


@pytest.fixture(scope="module")
def dev2(L, rich2, torch):
    dev = L.DeviceScene(rich2, bg_struct(L, DEFAULT_BG), 0)
    assert dev.info().has_bvh == 1 and dev.info().n_spheres == 486
    yield dev
    dev.release()


@pytest.fixture(scope="module")
def rays_a(L, O):
    """Set (a): the camera rays of test 1's first case, from the oracle."""
    st = camera(L, RICH_SETUP, W1, H1)
    return oracle_camera_rays(O, st.as_array(), W1, ROWS1, 3, PASS1, RADIUS1, SEED1)


@pytest.fixture(scope="module")
def hits_a(L, O, rich2, rays_a):
    return oracle_hits(O, L, rich2, rays_a[0])


def adversarial_scene(n=1200):
    """The random-radius scene of test_gpu_parity.test_bvh_adversarial_spheres, n spheres:
    overlapping, nested, duplicated, tiny and huge."""
    from oracle.oracle import SPHERE_DTYPE

    rng = np.random.default_rng(11)
    s = np.zeros(n, dtype=SPHERE_DTYPE)
    s["center"] = rng.uniform(-3, 3, (n, 3))
    s["radius"] = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), n))
    s["material"] = rng.integers(1, 4, n)
    s["albedo"] = rng.uniform(0.2, 0.95, (n, 3))
    s["param"] = np.where(s["material"] == 3, 1.5, rng.uniform(0, 0.6, n))
    s[50:60] = s[40:50]                     # exact duplicates: tie -> lowest index
    s[60:70] = s[40:50]
    s["radius"][60:70] *= 0.5               # nested
    s[0]["center"], s[0]["radius"] = (0, -5000, 0), 4990.0  # huge ground
    return s


# ------------------------------------------------------- 1. camera rays ------
@pytest.mark.parametrize("case,setup,r", [("dof_r3", RICH_SETUP, 3), ("dof_r1", RICH_SETUP, 1),
                                          ("pinhole_r3", PINHOLE_SETUP, 3)])
def test_camera_rays_bit_for_bit(L, O, torch, case, setup, r):
    st = camera(L, setup, W1, H1)
    p = L.make_params(W1, H1, 10, r, RADIUS1, SEED1, pass_=PASS1, **TILES1)
    assert L.params_rows(p) == len(ROWS1)
    rays, ids = device_camera_rays(L, torch, st, p)
    want_rays, want_ids = oracle_camera_rays(O, st.as_array(), W1, ROWS1, r, PASS1, RADIUS1, SEED1)
    got = rays.cpu().numpy()
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), want_ids)
    assert got.shape == want_rays.shape == (len(ROWS1) * W1 * r, 6)
    assert np.array_equal(got, want_rays), f"{case}: max difference {np.abs(got - want_rays).max()}"
    if setup[12] == 0.0:  # pinhole: every ray leaves the camera position
        assert np.array_equal(got[:, :3], np.tile(setup[:3], (len(got), 1)))


def test_camera_rays_without_ids(L, torch):
    st = camera(L, RICH_SETUP, W1, H1)
    p = L.make_params(W1, H1, 10, 2, RADIUS1, SEED1)
    with_ids, _ = device_camera_rays(L, torch, st, p)
    n = L.camera_rays_count(p)
    rays = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    L.camera_rays_async(st, p, rays.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(rays, with_ids)


# ------------------------------------------------------- 2. closest hit ------
FLAGS = [("bvh", 0), ("linear", 1)]


@pytest.mark.parametrize("name,flags", FLAGS)
def test_hit_camera_rays(L, torch, dev2, rays_a, hits_a, name, flags):
    """(a) test 1's rays."""
    assert (hits_a["index"] >= 0).sum() >= 200 and len(set(hits_a["index"].tolist())) > 10
    assert_hits_equal(device_hits(L, torch, dev2, rays_a[0], flags=flags), hits_a, name)


@pytest.fixture(scope="module")
def secondary(L, O, rich2, hits_a):
    """(b) ~2,000 rays leaving the hit points of (a) in random directions: they start on
    surfaces (self-intersection at t ~ 0) and, through glass, inside spheres."""
    pts = hits_a["point"][hits_a["index"] >= 0]
    reps = -(-2000 // len(pts))
    org = np.repeat(pts, reps, axis=0)[:2000]
    d = np.random.default_rng(1).normal(size=(len(org), 3))
    rays = np.concatenate([org, d], axis=1)
    return rays, oracle_hits(O, L, rich2, rays)


@pytest.mark.parametrize("name,flags", FLAGS)
def test_hit_secondary_rays(L, torch, dev2, secondary, name, flags):
    rays, want = secondary
    assert (want["front_face"][want["index"] >= 0] == 0).any()  # some hits from inside
    assert_hits_equal(device_hits(L, torch, dev2, rays, flags=flags), want, name)


@pytest.fixture(scope="module")
def special(L, O, rich2, dev2):
    """(c) axis-aligned directions, zero components, the zero vector; (d) origins at twice
    the BVH's bound (the per-ray linear-scan fallback); (e) one NaN, one infinite component."""
    M = dev2.info().bound
    assert M > 0
    rays = []
    for o in [(0.0, 1.0, 0.0), (4.0, 1.0, 0.0), (13.0, 2.0, 3.0), (-4.0, 0.2, 2.0), (0.3, 5.0, -0.7)]:
        for k in range(3):
            for sgn in (1.0, -1.0):
                d = np.zeros(3)
                d[k] = sgn
                rays.append(np.r_[o, d])                     # along an axis
                d2 = np.full(3, 0.5 * sgn)
                d2[k] = 0.0
                rays.append(np.r_[o, d2])                    # one zero component
        rays.append(np.r_[o, 0.0, 0.0, 0.0])                 # the zero vector
    n_c = len(rays)
    targets = [(0.0, 1.0, 0.0), (4.0, 1.0, 0.0), (-4.0, 1.0, 0.0), (0.0, 0.0, 0.0), (2.0, 0.2, 1.0)]
    for corner in [(2 * M, 2 * M, 2 * M), (-2 * M, 1.0, 0.0), (0.0, 2 * M, 0.0), (3.0, 1.0, -2 * M),
                   (2 * M, 0.5, 2 * M), (np.nextafter(M, INF), 1.0, 0.5)]:
        for tgt in targets:
            rays.append(np.r_[corner, np.subtract(tgt, corner)])
    n_d = len(rays) - n_c
    rays.append(np.r_[13.0, 2.0, 3.0, float("nan"), -0.1, -0.2])
    rays.append(np.r_[13.0, float("nan"), 3.0, -1.0, -0.1, -0.2])
    rays.append(np.r_[13.0, 2.0, 3.0, -INF, -0.1, -0.2])
    rays.append(np.r_[INF, 2.0, 3.0, -1.0, -0.1, -0.2])
    rays = np.array(rays)
    want = oracle_hits(O, L, rich2, rays)
    assert (want["index"][n_c:n_c + n_d] >= 0).sum() >= 10   # the far origins do see the scene
    assert (want["index"][n_c + n_d:] == -1).all()           # (e): the oracle says a miss
    return rays, want


@pytest.mark.parametrize("name,flags", FLAGS)
def test_hit_special_rays(L, torch, dev2, special, name, flags):
    rays, want = special
    assert_hits_equal(device_hits(L, torch, dev2, rays, flags=flags), want, name)


@pytest.mark.parametrize("name,flags", FLAGS)
def test_hit_finite_t_end(L, O, torch, dev2, rich2, rays_a, hits_a, name, flags):
    """(f) Interval.End at the hit's own root (strict: no longer that hit) and one ulp above it."""
    pick = np.nonzero(hits_a["index"] >= 0)[0][:200]
    assert len(pick) == 200
    flips = 0
    for i in pick:
        ray, t = rays_a[0][i], float(hits_a["t"][i])
        for t_end in (t, float(np.nextafter(t, INF))):
            want = oracle_hits(O, L, rich2, ray[None], t_end)
            got = device_hits(L, torch, dev2, ray[None], t_end=t_end, flags=flags)
            assert_hits_equal(got, want, f"{name} ray {i} t_end {t_end!r}")
        flips += int(want["index"][0] == hits_a["index"][i])
    assert flips == 200  # one ulp above the root the hit is back
    # ends at or below the interval start, and a huge one
    for t_end in (1e-6, 0.0, -1.0, -INF, 1e300):
        want = oracle_hits(O, L, rich2, rays_a[0][pick], t_end)
        assert_hits_equal(device_hits(L, torch, dev2, rays_a[0][pick], t_end=t_end, flags=flags), want,
                          f"{name} t_end {t_end}")


@pytest.mark.parametrize("name,flags", FLAGS)
def test_hit_ties_report_the_lower_index(L, O, torch, rich2, rays_a, secondary, name, flags):
    """(g) the first 40 small spheres appended again: equal roots, the earlier sphere wins."""
    small = np.nonzero(rich2["radius"] < 0.5)[0][:40]
    assert len(small) == 40
    sc = np.concatenate([rich2, rich2[small]])
    rays = np.concatenate([rays_a[0], secondary[0][:600]])
    want = oracle_hits(O, L, sc, rays)
    assert np.isin(want["index"], small).sum() >= 20  # duplicates are hit
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        got = device_hits(L, torch, dev, rays, flags=flags)
    finally:
        dev.release()
    assert (got["index"] < len(rich2)).all()
    assert_hits_equal(got, want, name)


@pytest.mark.parametrize("name,flags", FLAGS)
def test_hit_default_scene(L, O, torch, name, flags):
    """(h) 5 spheres: no BVH, every ray takes the linear scan."""
    sc = O.default_scene()
    st = camera(L, np.array([-2, 2, 1, 0, 0, -1, 0, 0, 0, 20.0, 0, 12.0 ** 0.5, 0.1]), 24, 16)
    rays, _ = oracle_camera_rays(O, st.as_array(), 24, range(16), 2, 0, 0.5, 3)
    want = oracle_hits(O, L, sc, rays)
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        assert dev.info().has_bvh == 0
        got = device_hits(L, torch, dev, rays, flags=flags)
    finally:
        dev.release()
    assert (want["index"] >= 0).sum() > 100
    assert_hits_equal(got, want, name)


@pytest.mark.parametrize("name,flags", FLAGS)
def test_hit_adversarial_scene(L, O, torch, name, flags):
    """(i) 1,200 random-radius spheres: overlaps, nesting, duplicates, a huge ground."""
    sc = adversarial_scene()
    st = camera(L, np.array([7.0, 3.0, 6.0, 0, 0, 0, 0, 1, 0, 45.0, 1.0, 9.0, 0.05]), 32, 24)
    prim, _ = oracle_camera_rays(O, st.as_array(), 32, range(24), 1, 0, 0.5, 9)
    first = oracle_hits(O, L, sc, prim)
    pts = first["point"][first["index"] >= 0]
    d = np.random.default_rng(2).normal(size=(len(pts), 3))
    rays = np.concatenate([prim, np.concatenate([pts, d], axis=1)])
    want = np.concatenate([first, oracle_hits(O, L, sc, rays[len(prim):])])
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        assert dev.info().has_bvh == 1
        got = device_hits(L, torch, dev, rays, flags=flags)
    finally:
        dev.release()
    assert_hits_equal(got, want, name)


def test_hit_n_zero_launches_nothing(L, dev2):
    dev2.hit_async(None, 0, None)
    dev2.ray_color_async(None, 0, 5, 1, None)


# -------------------------------------------------------- 3. ray colour ------
@pytest.fixture(scope="module")
def color_rays(L, O):
    st = camera(L, RICH_SETUP, 24, 16)
    return oracle_camera_rays(O, st.as_array(), 24, range(16), 2, 0, 0.5, 6)


@pytest.mark.parametrize("depth", [1, 12, 50])
@pytest.mark.parametrize("name,flags", FLAGS)
def test_ray_color_vs_oracle(L, O, torch, dev2, rich2, color_rays, depth, name, flags):
    rays, ids = color_rays
    want = [O.ray_color(rich2, DEFAULT_BG, r[:3], r[3:], depth, 6, int(i[0]), int(i[1])) for r, i in zip(rays, ids)]
    ref = np.array([w[0] for w in want])
    rseg = np.array([w[1] for w in want], dtype=np.uint32)
    rgb, seg = device_colors(L, torch, dev2, rays, depth, 6, ids, flags)
    assert np.array_equal(seg, rseg), f"{int((seg != rseg).sum())} paths took different decisions"
    err = float(np.abs(rgb - ref).max())
    print(f"ray colour depth {depth} {name}: L-inf {err:.3e}")
    assert err <= TOL, f"L-inf {err}"


def test_ray_color_without_ids(L, O, torch, dev2, rich2, color_rays):
    rays = color_rays[0][:300]
    want = [O.ray_color(rich2, DEFAULT_BG, r[:3], r[3:], 12, 9, i, 0) for i, r in enumerate(rays)]
    rgb, seg = device_colors(L, torch, dev2, rays, 12, 9, None)
    assert np.array_equal(seg, np.array([w[1] for w in want], dtype=np.uint32))
    err = float(np.abs(rgb - np.array([w[0] for w in want])).max())
    assert err <= TOL, f"L-inf {err}"
    # and the ids do matter: another pixel word draws other scatter directions
    other, _ = device_colors(L, torch, dev2, rays, 12, 9, np.stack([np.arange(300) + 7, np.zeros(300)], 1))
    assert not np.array_equal(other, rgb)


# ------------------------------------- 4. the pipeline equals the renderer ---
@pytest.mark.parametrize("r", [3, 1])
@pytest.mark.parametrize("name,flags", FLAGS)
def test_pipeline_equals_render_bit_for_bit(L, torch, dev2, r, name, flags):
    w, h, depth, seed = 40, 24, 20, 9
    st = camera(L, RICH_SETUP, w, h)
    p = L.make_params(w, h, depth, r, 0.5, seed, pass_=1, flags=L.FLAG_ORDERED_SUM | flags)
    out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    seg = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    dev2.render_async(st, p, out.data_ptr(), seg.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rays, ids = device_camera_rays(L, torch, st, p)
    n = h * w * r
    rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    qseg = torch.zeros(n, dtype=torch.int32, device="cuda")
    dev2.ray_color_async(rays.data_ptr(), n, depth, seed, rgb.data_ptr(), ids.data_ptr(), qseg.data_ptr(), flags,
                         torch.cuda.current_stream().cuda_stream)
    samples = rgb.cpu().numpy().reshape(h, w, r, 3)
    total = np.zeros((h, w, 3))
    for s in range(r):  # colorSum = Add(colorSum, color) in sample order (ray/tracer.go:143)
        total = total + samples[:, :, s]
    mean = total * (1.0 / r)
    assert np.array_equal(mean, out.cpu().numpy())
    assert np.array_equal(qseg.cpu().numpy().reshape(h, w, r).sum(axis=2), seg.cpu().numpy())


# ------------------------------------------------------ 5. beside a render ---
def test_hit_query_beside_a_render(L, torch, dev2, rays_a, hits_a):
    w, h = 96, 54
    st = camera(L, RICH_SETUP, w, h)
    p = L.make_params(w, h, 50, 64, 0.5, 2, output=L.OUT_RGB_F32)

    def render(stream):
        out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.current_stream().synchronize()
        dev2.render_async(st, p, out.data_ptr(), None, stream.cuda_stream)
        return out

    solo = render(torch.cuda.current_stream())
    torch.cuda.synchronize()
    rays = np.tile(rays_a[0], (40, 1))
    r = torch.from_numpy(rays).cuda()
    hits = torch.full((len(r), 8), float("nan"), dtype=torch.float64, device="cuda")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    both = render(sa)
    dev2.hit_async(r.data_ptr(), len(r), hits.data_ptr(), stream=sb.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(both, solo)
    got = hits.cpu().numpy().reshape(-1).view(L.HIT_DTYPE)
    assert_hits_equal(got, np.tile(hits_a, 40), "beside a render")
    assert_hits_equal(device_hits(L, torch, dev2, rays_a[0]), hits_a, "solo")


# ---------------------------------------------------- 6. the Python mirror ---
def _book_tracer(w, h, seed):
    from tray_amd import ray

    t = ray.New(w, h)
    c = ray.RichSceneCamera()
    t.Position, t.LookAt, t.Up = c.Position, c.LookAt, c.Up
    t.VerticalFoV, t.FocalLength, t.FocusDistance = c.VerticalFoV, c.FocalLength, c.FocusDistance
    t.Aperture = 0.0  # pinhole: the ray of a pixel is the ray through its centre
    t.NumRaysPerPixel, t.MaxDepth, t.Seed = 1, 20, seed
    return ray, t


def test_mirror_picking(L, O, rich2):
    ray, t = _book_tracer(160, 90, 4)
    t.Camera.Initialize(160, 90)
    scene = ray.Scene.from_array(rich2, ray.DefaultBackground())
    target = int(np.nonzero((rich2["center"] == (4.0, 1.0, 0.0)).all(axis=1))[0][0])
    assert rich2["material"][target] == L.METAL
    # the pixel whose centre the line from the camera to the sphere's centre crosses:
    # pixel00 + a pixel_x + b pixel_y = position + s (centre - position)
    st = t.Camera._state
    pos, p00 = np.array(st.position), np.array(st.pixel00)
    A = np.stack([np.array(st.pixel_x), np.array(st.pixel_y), -(rich2["center"][target] - pos)], axis=1)
    a, b, _ = np.linalg.solve(A, pos - p00)
    x, y = int(round(a)), int(round(b))
    assert 0 <= x < 160 and 0 <= y < 90
    rays, ids = t.CameraRays(y, y + 1)
    assert rays.shape == (160,) and np.array_equal(ids[:, 0], y * 160 + np.arange(160))
    hit = scene.Hit(rays["origin"][x], rays["direction"][x])
    assert hit.dtype == L.HIT_DTYPE and hit.shape == (1,)
    assert hit["index"][0] == target and hit["front_face"][0] == 1
    o, d = O.get_ray(st.as_array(), float(x), float(y))
    assert_hits_equal(hit, oracle_hits(O, L, rich2, np.r_[o, d][None]), "picking")
    # the device copy is kept while the scene does not change, and replaced when it does
    first = scene._uploaded[0][1]
    scene.Hit(rays["origin"], rays["direction"], interval=(1e-6, 5.0))
    assert scene._uploaded[0][1] is first
    scene.Objects.pop(1)  # a small sphere before the target: the list, and the target's place in it, change
    assert scene.Hit(rays["origin"][x], rays["direction"][x])["index"][0] == target - 1
    assert scene._uploaded[0][1] is not first


def test_mirror_ray_color_reproduces_render(rich2):
    ray, t = _book_tracer(48, 27, 5)
    scene = ray.Scene.from_array(rich2)
    t.Render(scene)  # defaults the background, initializes the camera
    rays, ids = t.CameraRays(0, 27)
    rgb, seg = scene.RayColor(rays["origin"], rays["direction"], t.MaxDepth, t.Seed, ids)
    assert np.array_equal(rgb.reshape(27, 48, 3), t.linear)
    assert np.array_equal(seg.reshape(27, 48), t.segments)
