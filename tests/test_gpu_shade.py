"""Material.Scatter, AmbientLight.Hit and the occlusion query (include/tray_shade.h)
on the device against the oracle's restatement of ray/materials.go and
ray/objects.go, and the wavefront built from them against tray_ray_color_async.

Contract: a scattered ray and its attenuation are the reference's bits, record
for record (the first check of the scatter step on its own, not through whole
paths); the sky colour is the reference's bits; occlusion is, by definition,
tray_scene_hit_async's index >= 0 for the same interval; and
GetRay -> loop { Hit -> Scatter | sky } composed by the caller is RayColor, bit
for bit: between the calls there is one correctly rounded FP64 multiply per
channel, in the megakernel's outer-first order.
"""
import ctypes

import numpy as np
import pytest

from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_parity import bg_struct, camera
from test_gpu_query import (H1, INF, PASS1, RADIUS1, ROWS1, SEED1, TOL, W1, _book_tracer, adversarial_scene, bits,
                            dev2, device_camera_rays, device_colors, device_hits, hits_a, oracle_camera_rays,
                            oracle_hits, rays_a, rich2, secondary, special, torch)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

FLAGS = [("bvh", 0), ("linear", 1)]
SKY = np.array([0.9, 0.2, 0.1, 0.1, 0.3, 0.8])  # a non-default AmbientLight: ColorA, ColorB
SEED_B = 77


# ------------------------------------------------------------------ helpers --
def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _rays_t(torch, rays):
    return torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)).cuda()


def _ids_t(torch, ids):
    return torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1, 2).view(np.int32)).cuda()


def device_scatter(L, torch, dev, rays, hits, seed, ids=None, bounce=0):
    """tray_scatter_async on host arrays -> SCATTER_DTYPE array (output pre-filled with NaN)."""
    r = _rays_t(torch, rays)
    h = torch.from_numpy(np.ascontiguousarray(hits).view(np.float64).reshape(-1, 8)).cuda()
    i = None if ids is None else _ids_t(torch, ids)
    out = torch.full((len(r), 10), float("nan"), dtype=torch.float64, device="cuda")
    dev.scatter_async(r.data_ptr(), h.data_ptr(), len(r), seed, out.data_ptr(), None if i is None else i.data_ptr(),
                      bounce, _stream(torch))
    return out.cpu().numpy().reshape(-1).view(L.SCATTER_DTYPE)


def device_sky(L, torch, bg, dirs):
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    r = _rays_t(torch, np.concatenate([np.zeros_like(d), d], axis=1))
    rgb = torch.full((len(r), 3), float("inf"), dtype=torch.float64, device="cuda")
    L.background_hit_async(bg_struct(L, bg), r.data_ptr(), len(r), rgb.data_ptr(), 0, _stream(torch))
    return rgb.cpu().numpy()


def device_occluded(torch, dev, rays, t_end=INF, ends=None, flags=0):
    """tray_scene_occluded_async on host arrays -> (n,) uint8, the buffer pre-filled with 0xFF."""
    r = _rays_t(torch, rays)
    e = None if ends is None else torch.from_numpy(np.ascontiguousarray(ends, dtype=np.float64)).cuda()
    out = torch.full((len(r),), 0xFF, dtype=torch.uint8, device="cuda")
    dev.occluded_async(r.data_ptr(), len(r), out.data_ptr(), t_end, None if e is None else e.data_ptr(), flags,
                       _stream(torch))
    return out.cpu().numpy()


def oracle_scatter(O, L, spheres, rays, hits, seed, ids, bounce):
    """O.scatter per record -> (SCATTER_DTYPE array, zero where not scattered)."""
    out = np.zeros(len(hits), dtype=L.SCATTER_DTYPE)
    bounce = np.broadcast_to(bounce, len(hits))
    for k, (r, h) in enumerate(zip(np.asarray(rays).reshape(-1, 6), hits)):
        ok, att, o, d = O.scatter(spheres[int(h["index"])], r[:3], r[3:], h["point"], h["normal"], int(h["front_face"]),
                                  seed, int(ids[k][0]), int(ids[k][1]), int(bounce[k]))
        if ok:
            out[k] = (att, (o, d), 1, 0)
    return out


def assert_scatter_equal(got, want, what):
    assert np.array_equal(got["scattered"], want["scattered"]), \
        f"{what}: {int((got['scattered'] != want['scattered']).sum())} records decided differently"
    assert not got["reserved"].any(), what
    on = want["scattered"] == 1
    for name, g, w in (("attenuation", got["attenuation"], want["attenuation"]),
                       ("origin", got["ray"]["origin"], want["ray"]["origin"]),
                       ("direction", got["ray"]["direction"], want["ray"]["direction"])):
        bad = np.nonzero((bits(g[on]) != bits(w[on])).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} records, first {bad[:1]}: " \
                              f"{g[on][bad[:1]]} for {w[on][bad[:1]]}"
    assert_all_zero(got[~on], what)


def assert_all_zero(records, what):
    assert not np.ascontiguousarray(records).view(np.uint8).any(), f"{what}: a record that is not scattered is not all zero"


def branch_of(spheres, ray, h, out):
    """Which branch of Material.Scatter the oracle took for this record, from its inputs and result."""
    s = spheres[int(h["index"])]
    if s["material"] == 1:
        return "lambertian"
    if s["material"] == 2:
        if not out["scattered"]:
            return "metal_absorbed"
        return "metal_fuzz" if s["param"] > 0 else "metal_mirror"
    front = int(h["front_face"])
    d = ray[3:] / np.sqrt(ray[3:] @ ray[3:])
    cos = min(float(-d @ h["normal"]), 1.0)
    ratio = 1.0 / s["param"] if front else s["param"]
    side = "front" if front else "back"
    if out["ray"]["direction"] @ h["normal"] < 0:
        return "refract_" + side
    return "total_internal" if ratio * np.sqrt(1.0 - cos * cos) > 1.0 else "schlick_" + side


# ----------------------------------------------------------------- fixtures --
@pytest.fixture(scope="module")
def set_a(L, O, rich2, rays_a):
    """Set A: the 396 camera rays of test_gpu_query's first case followed with the oracle
    (scene_hit -> scatter) for 6 bounces; every hit is one (ray, record, ids, bounce) tuple."""
    rays, recs, ids, bounces = [], [], [], []
    for ray, (pixel, word) in zip(*rays_a):
        o, d = ray[:3], ray[3:]
        for b in range(6):
            h = oracle_hits(O, L, rich2, np.r_[o, d][None])
            if h["index"][0] < 0:
                break
            rays.append(np.r_[o, d]), recs.append(h[0]), ids.append((pixel, word)), bounces.append(b)
            ok, _, o, d = O.scatter(rich2[int(h["index"][0])], o, d, h["point"][0], h["normal"][0],
                                    int(h["front_face"][0]), SEED1, int(pixel), int(word), b)
            if not ok:
                break
    rays, recs = np.array(rays), np.array(recs, dtype=L.HIT_DTYPE)
    ids, bounces = np.array(ids, dtype=np.uint32), np.array(bounces)
    return rays, recs, ids, bounces, oracle_scatter(O, L, rich2, rays, recs, SEED1, ids, bounces)


def scene_b():
    """Set B's scene: glass (RefIdx 1.5) at the origin, metal with fuzz 1.5 at (3, 0, 0), Lambertian at (-3, 0, 0)."""
    from oracle.oracle import SPHERE_DTYPE

    s = np.zeros(3, dtype=SPHERE_DTYPE)
    s["radius"] = 1.0
    s["center"] = [(0, 0, 0), (3, 0, 0), (-3, 0, 0)]
    s["material"] = [3, 2, 1]
    s["param"] = [1.5, 1.5, 0.0]
    s["albedo"] = [(0, 0, 0), (0.8, 0.8, 0.8), (0.5, 0.5, 0.5)]
    return s


@pytest.fixture(scope="module")
def set_b(L, O):
    """Set B: rays from inside the glass (about two thirds totally reflected) and rays onto
    the fuzz-1.5 metal (a good part absorbed): the two branches set A does not reach."""
    sc = scene_b()
    rng = np.random.default_rng(5)
    inside = np.concatenate([np.tile((0.9, 0.0, 0.0), (64, 1)), rng.normal(size=(64, 3))], axis=1)
    onto = np.concatenate([np.tile((3.0, 3.0, 0.0), (64, 1)), (0.0, -3.0, 0.0) + rng.uniform(-1, 1, (64, 3))], axis=1)
    rays = np.concatenate([inside, onto])
    h = oracle_hits(O, L, sc, rays)
    keep = h["index"] >= 0
    rays, recs = rays[keep], h[keep]
    ids = np.stack([1000 + np.arange(len(rays)), np.arange(len(rays)) % 7], axis=1).astype(np.uint32)
    bounces = np.arange(len(rays)) % 2 * 3  # bounce 0 and 3
    return sc, rays, recs, ids, bounces, oracle_scatter(O, L, sc, rays, recs, SEED_B, ids, bounces)


def scatter_by_bounce(L, torch, dev, rays, recs, ids, bounces, seed):
    """The device side of test 1: one call per bounce value."""
    got = np.zeros(len(recs), dtype=L.SCATTER_DTYPE)
    for b in np.unique(bounces):
        sel = bounces == b
        got[sel] = device_scatter(L, torch, dev, rays[sel], recs[sel], seed, ids[sel], int(b))
    return got


# ------------------------------------- 1. scatter against the oracle, bitwise --
def test_scatter_inputs_cover_every_branch(rich2, set_a, set_b):
    """The coverage guard, from the oracle's side: every branch of Material.Scatter has a record."""
    rays, recs, _, _, want = set_a
    seen_a = [branch_of(rich2, r, h, w) for r, h, w in zip(rays, recs, want)]
    sc, rays_b, recs_b, _, _, want_b = set_b
    seen_b = [branch_of(sc, r, h, w) for r, h, w in zip(rays_b, recs_b, want_b)]
    count = {k: (seen_a + seen_b).count(k) for k in set(seen_a + seen_b)}
    print(f"set A {len(seen_a)} records, set B {len(seen_b)}: {sorted(count.items())}")
    for branch in ("lambertian", "metal_mirror", "metal_fuzz", "metal_absorbed", "refract_front", "refract_back",
                   "total_internal"):
        assert count.get(branch, 0) >= 1, f"no record takes the {branch} branch"
    assert count.get("schlick_front", 0) + count.get("schlick_back", 0) >= 1, "no Schlick reflection"
    assert len(seen_a) >= 600 and max(set_a[3]) == 5


def test_scatter_set_a_bit_for_bit(L, torch, dev2, set_a):
    rays, recs, ids, bounces, want = set_a
    assert_scatter_equal(scatter_by_bounce(L, torch, dev2, rays, recs, ids, bounces, SEED1), want, "set A")


def test_scatter_set_b_bit_for_bit(L, torch, set_b):
    sc, rays, recs, ids, bounces, want = set_b
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        got = scatter_by_bounce(L, torch, dev, rays, recs, ids, bounces, SEED_B)
    finally:
        dev.release()
    assert (want["scattered"] == 0).any() and (want["scattered"] == 1).any()
    assert_scatter_equal(got, want, "set B")


def test_scatter_without_ids(L, O, torch, dev2, rich2, set_a):
    """ids NULL: pixel = position in the call, sample 0."""
    rays, recs, ids, bounces, with_ids = set_a
    first = np.nonzero(bounces == 0)[0][40:104]
    assert len(first) == 64
    no_ids = np.stack([np.arange(64), np.zeros(64)], axis=1).astype(np.uint32)
    want = oracle_scatter(O, L, rich2, rays[first], recs[first], SEED1, no_ids, 0)
    assert_scatter_equal(device_scatter(L, torch, dev2, rays[first], recs[first], SEED1, None, 0), want, "ids NULL")
    assert not np.array_equal(want["ray"]["direction"], with_ids["ray"]["direction"][first])  # the ids do matter


# ---------------------------------------------- 2. records that are not hits --
def test_scatter_of_records_that_are_no_hits(L, torch, dev2, rich2, rays_a, hits_a, secondary):
    sec_rays, sec_hits = secondary
    miss = np.nonzero(sec_hits["index"] < 0)[0][:100]  # the hit query's misses: index -1, all else zero
    hit = np.nonzero(hits_a["index"] >= 0)[0][:40]
    assert len(miss) == 100 and len(hit) == 40
    recs = np.concatenate([sec_hits[miss], hits_a[hit], hits_a[hit], hits_a[hit]])
    rays = np.concatenate([sec_rays[miss], rays_a[0][hit], rays_a[0][hit], rays_a[0][hit]])
    k = len(miss)
    recs["index"][k:k + 40] = len(rich2)          # one past the list
    recs["index"][k + 40:k + 80] = 2**31 - 1      # INT32_MAX
    recs["index"][k + 80:] = -(2**31)             # INT32_MIN
    got = device_scatter(L, torch, dev2, rays, recs, SEED1)  # the output buffer starts as NaN
    assert not got["scattered"].any()
    assert_all_zero(got, "no hit")


# ------------------------------------------- 3. a changed record is honoured --
def test_scatter_honours_a_changed_record(L, O, torch, dev2, rich2, set_a):
    rays, recs, ids, bounces, want = set_a
    glass = np.nonzero(rich2["material"][recs["index"]] == 3)[0][:32]
    assert len(glass) == 32
    flipped = recs[glass].copy()
    flipped["normal"] = -flipped["normal"]
    flipped["front_face"] = 1 - flipped["front_face"]
    flipped["point"] += 0.25  # and the scattered ray leaves the record's point, not the sphere's surface
    ref = oracle_scatter(O, L, rich2, rays[glass], flipped, SEED1, ids[glass], bounces[glass])
    assert not np.array_equal(ref["ray"]["direction"], want["ray"]["direction"][glass])
    assert np.array_equal(ref["ray"]["origin"][ref["scattered"] == 1], flipped["point"][ref["scattered"] == 1])
    got = scatter_by_bounce(L, torch, dev2, rays[glass], flipped, ids[glass], bounces[glass], SEED1)
    assert_scatter_equal(got, ref, "flipped records")


# -------------------------------------------------------------------- 4. sky --
def test_sky_bit_for_bit(L, O, torch, rays_a):
    from oracle.oracle import SPHERE_DTYPE

    axes = [s * np.eye(3)[k] for k in range(3) for s in (1.0, -1.0)]
    cam_dirs = rays_a[0][:, 3:]
    dirs = np.concatenate([cam_dirs, axes, cam_dirs[:20] * 1e-150 / 10.0, cam_dirs[:20] * 1e150 / 10.0,
                           [(0.0, 1e-150, 0.0), (1e150, -1e150, 1e150)]])
    far = np.zeros(1, dtype=SPHERE_DTYPE)  # a scene whose one sphere no test ray (from the origin) reaches
    far["center"], far["radius"], far["material"], far["albedo"] = (5e8, -7e8, 3e8), 1.0, 1, 0.5
    want = []
    for d in dirs:
        rgb, seg = O.ray_color(far, SKY, np.zeros(3), d, 1)
        assert seg == 1
        want.append(rgb)
    want = np.array(want)
    assert np.isfinite(want).all() and len({tuple(w) for w in want}) > 300
    got = device_sky(L, torch, SKY, dirs)
    assert np.array_equal(bits(got), bits(want)), f"max difference {np.abs(got - want).max()}"
    # straight up is ColorB, straight down ColorA
    assert np.array_equal(got[len(cam_dirs) + 2], SKY[3:]) and np.array_equal(got[len(cam_dirs) + 3], SKY[:3])


def test_sky_of_a_zero_direction_is_nan(L, O, torch):
    from oracle.oracle import SPHERE_DTYPE

    far = np.zeros(1, dtype=SPHERE_DTYPE)
    far["center"], far["radius"], far["material"] = (5e8, -7e8, 3e8), 1.0, 1
    want, _ = O.ray_color(far, SKY, np.zeros(3), np.zeros(3), 1)
    assert np.isnan(want).all()
    got = device_sky(L, torch, SKY, [(0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-0.0, 0.0, 0.0)])
    assert np.isnan(got[0]).all() and np.isnan(got[2]).all() and np.array_equal(got[1], SKY[3:])


# ------------------------------------ 5. the wavefront equals RayColor, bitwise --
def wavefront(L, torch, dev, bg, rays, ids, depth, seed, flags):
    """RayColor composed by the caller from the public calls and torch indexing:
    hit -> sky for the misses, scatter for the hits, until every path has ended."""
    n = len(rays)
    stream = _stream(torch)
    colour = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    seg = torch.zeros(n, dtype=torch.int32, device="cuda")
    live = torch.arange(n, device="cuda")
    cur, cur_ids = rays.clone(), ids.clone()
    thr = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    for bounce in range(depth):
        m = len(live)
        if m == 0:
            break
        hits = torch.empty((m, 8), dtype=torch.float64, device="cuda")
        dev.hit_async(cur.data_ptr(), m, hits.data_ptr(), INF, flags, stream)
        seg[live] += 1
        miss = hits.view(torch.int32)[:, 14] < 0
        sky_rays = cur[miss].contiguous()
        sky = torch.empty((len(sky_rays), 3), dtype=torch.float64, device="cuda")
        L.background_hit_async(bg, sky_rays.data_ptr(), len(sky_rays), sky.data_ptr(), 0, stream)
        colour[live[miss]] = thr[miss] * sky
        if bounce + 1 == depth:  # a hit at the last level is black (RayColor(depth 0))
            break
        on = ~miss
        live, cur, cur_ids, thr, hits = live[on], cur[on].contiguous(), cur_ids[on].contiguous(), thr[on], \
            hits[on].contiguous()
        m = len(live)
        out = torch.empty((m, 10), dtype=torch.float64, device="cuda")
        dev.scatter_async(cur.data_ptr(), hits.data_ptr(), m, seed, out.data_ptr(), cur_ids.data_ptr(), bounce, stream)
        ok = out.view(torch.int32)[:, 18] == 1  # not scattered: black, the path ends
        live, cur_ids = live[ok], cur_ids[ok].contiguous()
        thr = thr[ok] * out[ok, 0:3]  # outer-first, one multiply per channel
        cur = out[ok, 3:9].contiguous()
    return colour.cpu().numpy(), seg.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def wave_rays(L, torch):
    st = camera(L, RICH_SETUP, W1, H1)
    p = L.make_params(W1, H1, 10, 3, RADIUS1, SEED1, pass_=PASS1)
    rays, ids = device_camera_rays(L, torch, st, p)
    assert len(rays) == W1 * H1 * 3 == 1683
    return rays, ids


@pytest.mark.parametrize("depth", [1, 12, 50])
@pytest.mark.parametrize("name,flags", FLAGS)
def test_wavefront_equals_ray_color_bit_for_bit(L, torch, dev2, wave_rays, depth, name, flags):
    rays, ids = wave_rays
    n = len(rays)
    rgb = torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda")
    seg = torch.zeros(n, dtype=torch.int32, device="cuda")
    dev2.ray_color_async(rays.data_ptr(), n, depth, SEED1, rgb.data_ptr(), ids.data_ptr(), seg.data_ptr(), flags,
                         _stream(torch))
    colour, count = wavefront(L, torch, dev2, bg_struct(L, DEFAULT_BG), rays, ids, depth, SEED1, flags)
    want = rgb.cpu().numpy()
    assert np.array_equal(count, seg.cpu().numpy().view(np.uint32))
    assert np.array_equal(bits(colour), bits(want)), f"max difference {np.abs(colour - want).max()}"
    assert depth == 1 or count.max() > 3


def test_wavefront_vs_oracle(L, O, torch, dev2, rich2, wave_rays):
    """Against Go's recursion (inner-first products) the existing gate applies."""
    rays, ids = wave_rays
    pick = slice(0, 1683, 7)
    r, i = rays[pick].contiguous(), ids[pick].contiguous()
    colour, count = wavefront(L, torch, dev2, bg_struct(L, DEFAULT_BG), r, i, 12, SEED1, 0)
    want = [O.ray_color(rich2, DEFAULT_BG, a[:3], a[3:], 12, SEED1, int(b[0]), int(b[1]))
            for a, b in zip(r.cpu().numpy(), i.cpu().numpy().view(np.uint32))]
    assert np.array_equal(count, np.array([w[1] for w in want], dtype=np.uint32))
    err = float(np.abs(colour - np.array([w[0] for w in want])).max())
    print(f"wavefront depth 12 vs oracle: L-inf {err:.3e}")
    assert err <= TOL, f"L-inf {err}"


# ------------------------- 6. occlusion equals the closest hit's index >= 0 ---
def _default_scene_rays(L, O):
    sc = O.default_scene()
    st = camera(L, np.array([-2, 2, 1, 0, 0, -1, 0, 0, 0, 20.0, 0, 12.0 ** 0.5, 0.1]), 24, 16)
    rays, _ = oracle_camera_rays(O, st.as_array(), 24, range(16), 2, 0, 0.5, 3)
    return sc, rays


def _adversarial_rays(L, O):
    sc = adversarial_scene()
    st = camera(L, np.array([7.0, 3.0, 6.0, 0, 0, 0, 0, 1, 0, 45.0, 1.0, 9.0, 0.05]), 32, 24)
    prim, _ = oracle_camera_rays(O, st.as_array(), 32, range(24), 1, 0, 0.5, 9)
    first = oracle_hits(O, L, sc, prim)
    pts = first["point"][first["index"] >= 0]
    d = np.random.default_rng(2).normal(size=(len(pts), 3))
    return sc, np.concatenate([prim, np.concatenate([pts, d], axis=1)])


@pytest.fixture(scope="module")
def occlusion_cases(L, O, rich2, rays_a, secondary, special):
    """Per scene: (spheres, rays, the oracle's closest roots, per-ray ends, expected per-ray answers)."""
    cases = {"book": (rich2, np.concatenate([rays_a[0], secondary[0], special[0]])),
             "default": _default_scene_rays(L, O), "adversarial": _adversarial_rays(L, O)}
    out = {}
    for k, (name, (sc, rays)) in enumerate(sorted(cases.items())):
        closest = oracle_hits(O, L, sc, rays)
        root = np.where(closest["index"] >= 0, closest["t"], 1.0)
        choice = np.random.default_rng(30 + k).integers(0, 8, len(rays))
        choice[:8] = np.arange(8)
        table = np.stack([np.full(len(rays), INF), root, np.nextafter(root, INF), 0.5 * root, np.full(len(rays), 1e-6),
                          np.zeros(len(rays)), np.full(len(rays), -1.0), np.full(len(rays), np.nan)])
        ends = table[choice, np.arange(len(rays))]
        want = np.array([O.scene_hit(sc, r[:3], r[3:], 1e-6, e)[0] >= 0 for r, e in zip(rays, ends)])
        assert not want[~(ends > 1e-6)].any()  # NaN and ends <= 1e-6: an empty interval
        hit = closest["index"] >= 0
        assert want[hit & (choice == 2)].all() and want[hit & (choice == 0)].all() and (~want[~hit]).all()
        assert (hit & (choice == 1)).sum() > 10 and (want & (choice == 1)).sum() < (hit & (choice == 1)).sum()
        out[name] = (sc, rays, closest, ends, want)
    return out


@pytest.mark.parametrize("name,flags", FLAGS)
@pytest.mark.parametrize("scene", ["book", "default", "adversarial"])
def test_occlusion_equals_closest_hit(L, torch, occlusion_cases, scene, name, flags):
    sc, rays, closest, ends, want = occlusion_cases[scene]
    hit = np.nonzero(closest["index"] >= 0)[0]
    root = float(np.sort(closest["t"][hit])[len(hit) // 2])  # a root of one of the rays: half of the hits lie beyond it
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    try:
        assert dev.info().has_bvh == (0 if scene == "default" else 1)
        for t_end in (INF, root, float(np.nextafter(root, INF))):
            ref = device_hits(L, torch, dev, rays, t_end=t_end, flags=flags)["index"] >= 0
            got = device_occluded(torch, dev, rays, t_end=t_end, flags=flags)
            assert set(np.unique(got)) <= {0, 1}, f"{scene} {name} t_end {t_end!r}: a byte was not written"
            bad = np.nonzero(got.astype(bool) != ref)[0]
            assert bad.size == 0, f"{scene} {name} t_end {t_end!r}: {bad.size} rays differ, first {bad[:3]}"
            if t_end == INF:
                assert np.array_equal(ref, closest["index"] >= 0)
            else:
                assert ref.any() and not ref[hit].all()
        got = device_occluded(torch, dev, rays, t_end=INF, ends=ends, flags=flags)
    finally:
        dev.release()
    assert set(np.unique(got)) <= {0, 1}, f"{scene} {name} per-ray ends: a byte was not written"
    bad = np.nonzero(got.astype(bool) != want)[0]
    assert bad.size == 0, f"{scene} {name} per-ray ends: {bad.size} rays differ, first {bad[:3]}, ends {ends[bad[:3]]}"


# ------------------------------------------------------------------ 7. n = 0 --
def test_n_zero_launches_nothing(L, dev2):
    dev2.scatter_async(None, None, 0, 1, None)
    dev2.occluded_async(None, 0, None)
    dev2.occluded_async(None, 0, None, flags=L.FLAG_LINEAR_SCAN)
    L.background_hit_async(bg_struct(L, DEFAULT_BG), None, 0, None)


# ------------------------------------------------------ 8. the Python mirror --
@pytest.fixture(scope="module")
def mirror_scene(rich2):
    from tray_amd import ray

    return ray, ray.Scene.from_array(rich2, ray.DefaultBackground())


def test_mirror_scatter(L, mirror_scene, set_a):
    _, scene = mirror_scene
    rays, recs, ids, bounces, want = set_a
    pick = np.nonzero(bounces == 1)[0][:64]
    assert len(pick) == 64
    got = scene.Scatter(rays[pick, :3], rays[pick, 3:], recs[pick], SEED1, ids[pick], bounce=1)
    assert got.dtype == L.SCATTER_DTYPE and got.shape == (64,)
    assert_scatter_equal(got, want[pick], "Scene.Scatter")


def test_mirror_occluded(L, mirror_scene, occlusion_cases):
    _, scene = mirror_scene
    _, rays, closest, ends, want = occlusion_cases["book"]
    pick = slice(380, 444)  # camera rays and secondary rays
    got = scene.Occluded(rays[pick, :3], rays[pick, 3:])
    assert got.dtype == bool and got.shape == (64,)
    assert np.array_equal(got, closest["index"][pick] >= 0)
    assert np.array_equal(scene.Occluded(rays[pick, :3], rays[pick, 3:], t_end=ends[pick]), want[pick])
    t = float(closest["t"][pick][closest["index"][pick] >= 0][0])
    assert np.array_equal(scene.Occluded(rays[pick, :3], rays[pick, 3:], t_end=t),
                          scene.Hit(rays[pick, :3], rays[pick, 3:], interval=(1e-6, t))["index"] >= 0)


def test_mirror_ambient_light_hit(L, O, torch, mirror_scene, rays_a):
    ray, _ = mirror_scene
    dirs = rays_a[0][:64, 3:]
    got = ray.AmbientLight(tuple(SKY[:3]), tuple(SKY[3:])).Hit(dirs)
    assert got.shape == (64, 3) and got.dtype == np.float64
    assert np.array_equal(bits(got), bits(device_sky(L, torch, SKY, dirs)))
    lone = np.zeros(1, dtype=L.SPHERE_DTYPE)
    lone["center"], lone["radius"], lone["material"] = (5e8, -7e8, 3e8), 1.0, 1
    want = np.array([O.ray_color(lone, SKY, np.zeros(3), d, 1)[0] for d in dirs])
    assert np.array_equal(bits(got), bits(want))


def test_mirror_wavefront_of_the_readme_reproduces_ray_color(rich2):
    """README.md, "Ray queries": the loop as printed there, on a small frame."""
    ray, t = _book_tracer(32, 18, 5)
    t.NumRaysPerPixel = 2
    scene = ray.Scene.from_array(rich2, ray.DefaultBackground())
    t.Camera.Initialize(32, 18)
    rays, ids = t.CameraRays(0, t.height)
    want, _ = scene.RayColor(rays["origin"], rays["direction"], t.MaxDepth, t.Seed, ids)
    o, d, n = rays["origin"], rays["direction"], len(rays)
    thr, colour, live = np.ones((n, 3)), np.zeros((n, 3)), np.arange(n)
    for bounce in range(t.MaxDepth):
        hits = scene.Hit(o, d)
        miss = hits["index"] < 0
        colour[live[miss]] = thr[miss] * scene.Background.Hit(d[miss])
        s = scene.Scatter(o[~miss], d[~miss], hits[~miss], t.Seed, ids[~miss], bounce)
        on = s["scattered"] == 1
        live, ids, thr = live[~miss][on], ids[~miss][on], thr[~miss][on] * s["attenuation"][on]
        o, d = s["ray"]["origin"][on], s["ray"]["direction"][on]
    assert n == 32 * 18 * 2 and np.array_equal(bits(colour), bits(want))


def test_mirror_scatter_after_hit_on_the_picking_rays(L, O, rich2):
    """ray.Scene.Scatter(...) after ray.Scene.Hit(...) on the rays of test_mirror_picking's row."""
    ray, t = _book_tracer(160, 90, 4)
    t.Camera.Initialize(160, 90)
    scene = ray.Scene.from_array(rich2, ray.DefaultBackground())
    rays, ids = t.CameraRays(40, 41)
    hits = scene.Hit(rays["origin"], rays["direction"])
    got = scene.Scatter(rays["origin"], rays["direction"], hits, t.Seed, ids)
    on = hits["index"] >= 0
    assert on.sum() > 100 and len(set(hits["index"][on].tolist())) > 3
    assert_all_zero(got[~on], "misses")
    flat = np.concatenate([rays["origin"], rays["direction"]], axis=1)
    want = oracle_scatter(O, L, rich2, flat[on], hits[on], t.Seed, ids[on], 0)
    assert_scatter_equal(got[on], want, "Scene.Scatter after Scene.Hit")
    assert np.array_equal(got["ray"]["origin"][on & (got["scattered"] == 1)],
                          hits["point"][on & (got["scattered"] == 1)])
