"""include/tray_scene_update.h on the device: an update of an uploaded scene A with the centres and
radii of B must leave exactly what a fresh upload of B leaves, in every render and query, on seven
shapes of tests/query_shapes.py and under every motion of
tests/scene_update_cases.py; the node array must be tests/scene_update_ref.py's, byte for byte; a
refused update must leave nothing but its record; the call orders itself after the renders enqueued
before it; and Scene.Move and Tracer.RenderAnimation sit on top.

Frames are 40 x 24 at r = 4, depth 8, ray radius 0.5, seed 7 in FP64, compared as bit patterns (a NaN
equals a NaN). Every comparison of an updated scene with a fresh one comes with a condition on the
two fresh scenes, so that an update that does nothing cannot pass: at least 40 % of the frame's pixels
differ between A and B (but under the dome, where every path ends on a Lambertian surface and the frame
is black), and at least 40 % of the hit records of the frame's camera rays. The rays of the hit
comparison are those camera rays and the Scatter rays of their hits on B; query_shapes.assert_live
holds for all of them on B. (The scattered rays leave from B's surfaces, mostly into the sky: they find
the same hit in A and B more often than the camera rays do, 4 % of them differ on the chain against 41 %,
so the 40 % is asked of the camera rays.)"""
import numpy as np
import pytest

import query_shapes as Q
import scene_update_cases as C
import scene_update_ref as S
from conftest import DEFAULT_BG
from test_gpu_adaptive import device_pixels
from test_gpu_aov import assert_aov_equal, device_aov
from test_gpu_parity import TOL, bg_struct, camera
from test_gpu_query import (INF, assert_hits_equal, device_camera_rays, device_hits, oracle_hits,
                            torch)  # noqa: F401 (fixture)
from test_gpu_shade import device_occluded, device_scatter
from test_gpu_temporal import assert_state, device_step

pytestmark = pytest.mark.gpu

W, H = Q.W, Q.H
R, DEPTH, RADIUS, SEED = 4, 8, 0.5, 7
NAN = float("nan")


def params(L, flags=0, pass_=0):
    return L.make_params(W, H, DEPTH, R, RADIUS, SEED, flags=flags, pass_=pass_)


def render(L, torch, dev, st, flags=0, pass_=0, stream=None):
    """tray_render_async into a NaN-filled FP64 frame -> (H, W, 3)."""
    out = torch.full((H, W, 3), NAN, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev.render_async(st, params(L, flags, pass_), out.data_ptr(), None,
                     stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_same(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    bad = np.argwhere((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b)))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[0]}: {a[tuple(bad[0])]!r} for " \
                          f"{b[tuple(bad[0])]!r}"


def update_async(L, torch, dev, geometry, stream=None):
    """tray_scene_update_async from a device tensor on the current stream (or `stream`) -> the record."""
    g = torch.from_numpy(np.ascontiguousarray(geometry, dtype=np.float64)).cuda()
    rec = torch.zeros(4, dtype=torch.float64, device="cuda")
    torch.cuda.current_stream().synchronize()
    dev.update_async(g.data_ptr(), len(geometry), rec.data_ptr(),
                     stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(L.SCENE_UPDATE_RECORD_DTYPE)[0]


def fresh(L, shape, spheres):
    """A new upload under the shape's knobs (no facts asserted: B need not be on A's boundary)."""
    with L.debug_knobs(**shape.knobs):
        return L.DeviceScene(spheres, bg_struct(L, DEFAULT_BG), 0)


class Case:
    pass


@pytest.fixture(scope="module", params=C.CASES, ids=lambda p: f"{p[0]}-{p[1]}")
def case(request, L, O, torch):
    """A uploaded with the shape's facts asserted and rendered once (so its candidate lists and work
    order are warm), then updated to B on the same stream; B uploaded afresh beside it."""
    c = Case()
    name, motion = request.param
    c.what, c.shape = f"{name} {motion}", C.SHAPES[name]
    c.A = c.shape.build(O)
    c.B = C.MOTIONS[motion](c.A)
    c.n = len(c.A)
    assert c.B.dtype == c.A.dtype and len(c.B) == c.n
    for f in ("material", "albedo", "param"):
        assert np.array_equal(c.A[f], c.B[f])
    c.geoA, c.geoB = C.geometry(c.A), C.geometry(c.B)
    c.st = camera(L, c.shape.setup, W, H)
    c.dev = Q.upload(L, c.shape, c.A, bg_struct(L, DEFAULT_BG))
    c.fresh = None
    try:
        c.info = c.dev.info()
        c.nodes0 = c.dev.nodes()
        c.leaves, c.slots = c.dev.leaves()
        assert len(c.nodes0) == c.info.n_nodes and len(c.leaves) == c.info.n_leaves
        assert len(c.slots) == (c.n if c.info.has_bvh else 0)
        c.frameA = render(L, torch, c.dev, c.st)
        c.rays_t, c.ids_t = device_camera_rays(L, torch, c.st, params(L))
        c.cam_rays = c.rays_t.cpu().numpy()
        c.ids = c.ids_t.cpu().numpy().view(np.uint32)
        c.hitsA = device_hits(L, torch, c.dev, c.cam_rays)
        c.rec = update_async(L, torch, c.dev, c.geoB)
        c.fresh = fresh(L, c.shape, c.B)
        yield c
    finally:
        c.dev.release()
        if c.fresh is not None:
            c.fresh.release()


def test_record_and_info(L, case):
    c = case
    n_refused, first, extent = S.check(c.geoB, c.info.bound if c.info.has_bvh else INF)  # no tree: no check
    assert (n_refused, first) == (0, -1), f"{c.what}: the reference refuses the motion"
    assert (c.rec["applied"], c.rec["n_refused"], c.rec["first_refused"], c.rec["reserved"]) == (1, 0, -1, 0), c.what
    assert c.rec["extent"] == extent and c.rec["bound"] == (c.info.bound if c.info.has_bvh else 0.0), c.what
    assert Q.facts(c.dev.info()) == Q.facts(c.info), f"{c.what}: tray_scene_get_info changed"
    assert c.dev.info().lds_resident == c.info.lds_resident


def test_frames(L, O, torch, case):
    """The default frame pins the boxes (and the candidate lists and work order, warm from A's frame),
    the linear-scan frame the sphere and material records; and the default frame is the oracle's."""
    c = case
    freshB = render(L, torch, c.fresh, c.st)
    changed = C.fraction_differing(c.frameA.reshape(-1, 3), freshB.reshape(-1, 3))
    print(f"{c.what}: {changed:.3f} of the pixels differ between A and B")
    if c.shape.name == "dome":
        assert not c.frameA.any() and not freshB.any()  # black: the hit records carry this shape
    else:
        assert changed >= 0.4, f"{c.what}: only {changed:.3f} of the pixels differ between A and B"
    assert_same(render(L, torch, c.dev, c.st), freshB, f"{c.what} frame")
    assert_same(render(L, torch, c.dev, c.st), freshB, f"{c.what} frame again (its lists and order now warm)")
    assert_same(render(L, torch, c.dev, c.st, flags=L.FLAG_LINEAR_SCAN),
                render(L, torch, c.fresh, c.st, flags=L.FLAG_LINEAR_SCAN), f"{c.what} TRAY_FLAG_LINEAR_SCAN frame")
    assert_same(render(L, torch, c.dev, c.st, pass_=3), render(L, torch, c.fresh, c.st, pass_=3), f"{c.what} pass 3")
    ref, _ = O.render(c.B, DEFAULT_BG, c.st.as_array(), W, H, R, DEPTH, RADIUS, SEED)
    err = float(np.abs(freshB - ref).max())
    print(f"{c.what}: L-inf against the oracle {err:.3e}")
    assert err <= TOL, f"{c.what}: L-inf {err} against the oracle"


def test_hits_and_occlusion(L, O, torch, case):
    c = case
    wantB = oracle_hits(O, L, c.B, c.cam_rays)
    changed = C.hits_differing(c.hitsA, wantB)
    print(f"{c.what}: {changed:.3f} of the camera rays' hit records differ between A and B")
    assert changed >= 0.4, f"{c.what}: only {changed:.3f} of the hit records differ between A and B"
    hit = wantB["index"] >= 0
    sc = device_scatter(L, torch, c.fresh, c.cam_rays[hit], wantB[hit], SEED, c.ids[hit])
    ok = sc["scattered"] == 1
    assert ok.sum() > 100
    rays = np.concatenate([c.cam_rays, np.concatenate([sc["ray"]["origin"][ok], sc["ray"]["direction"][ok]], axis=1)])
    want = np.concatenate([wantB, oracle_hits(O, L, c.B, rays[len(c.cam_rays):])])
    Q.assert_live(c.shape, c.n, c.info.bound, rays[:, :3], want["index"], "camera and scattered rays on B")
    # Scene.Scatter reads the material records the update rewrote (radius, 1 / R)
    again = device_scatter(L, torch, c.dev, c.cam_rays[hit], wantB[hit], SEED, c.ids[hit])
    assert again.tobytes() == sc.tobytes(), f"{c.what}: Scatter differs from the fresh upload's"
    for name, flags in (("tree", 0), ("scan", L.FLAG_LINEAR_SCAN)):
        got = device_hits(L, torch, c.dev, rays, flags=flags)
        assert_hits_equal(got, device_hits(L, torch, c.fresh, rays, flags=flags), f"{c.what} {name} against a fresh upload")
        assert_hits_equal(got, want, f"{c.what} {name} against the oracle")
        root = np.where(want["index"] >= 0, want["t"], 1.0)
        for label, kw in (("+inf", dict(t_end=INF)), ("own root", dict(ends=root)),
                          ("one ulp above", dict(ends=np.nextafter(root, INF)))):
            a = device_occluded(torch, c.dev, rays, flags=flags, **kw)
            b = device_occluded(torch, c.fresh, rays, flags=flags, **kw)
            assert np.array_equal(a, b), f"{c.what} {name} occluded {label}"
        assert np.array_equal(device_occluded(torch, c.dev, rays, flags=flags).astype(bool), want["index"] >= 0)


def test_query_side_kernels(L, torch, case):
    """The three kinds of query-side traversal (query_shapes.KINDS): the feature buffers (plain), the
    pixel list (pixels) and one temporal step from an empty state (temporal)."""
    c = case
    for name, flags in (("tree", 0), ("scan", L.FLAG_LINEAR_SCAN)):
        p = params(L, flags)
        got, want = device_aov(L, torch, c.dev, c.st, p), device_aov(L, torch, c.fresh, c.st, p)
        assert (want["index"] >= 0).any()
        assert_aov_equal(got, want, f"{c.what} {name} feature buffers")
        lst = np.arange(3, W * H, 7)
        got, gseg = device_pixels(L, torch, c.dev, c.st, p, lst, 2)
        want, wseg = device_pixels(L, torch, c.fresh, c.st, p, lst, 2)
        assert_same(got, want, f"{c.what} {name} pixel list")
        assert np.array_equal(gseg, wseg), f"{c.what} {name} pixel list segments"
        tp = L.temporal_params(flags=flags)
        frame = np.random.default_rng(11).random((H, W, 3))
        got, grec = device_step(L, torch, c.dev, c.st, None, tp, frame, None, W, H)
        want, wrec = device_step(L, torch, c.fresh, c.st, None, tp, frame, None, W, H)
        assert_state(got, want, f"{c.what} {name} temporal step")
        assert grec == wrec and (want["index"] >= 0).any()


def test_nodes_are_the_reference_refit(L, case):
    c = case
    now = c.dev.nodes()
    if not c.info.has_bvh:
        assert len(now) == 0 and len(c.nodes0) == 0
        return
    want = S.refit(c.nodes0, c.leaves, c.slots, c.geoB, c.info.bound)
    assert now.dtype == L.NODE_DTYPE and now.tobytes() == want.tobytes(), \
        f"{c.what}: {int((now['box'] != want['box']).sum())} box planes differ from the reference refit"
    assert np.array_equal(now["ref"], c.nodes0["ref"]) and np.array_equal(now["pad"], c.nodes0["pad"])
    unused = c.nodes0["ref"] == S.NONE
    assert (now["box"][:, :, 0, :].transpose(0, 2, 1)[unused] == np.inf).all()
    assert (now["box"][:, :, 1, :].transpose(0, 2, 1)[unused] == -np.inf).all()
    assert now.tobytes() != c.nodes0.tobytes(), f"{c.what}: the motion moved no box"
    leaves, slots = c.dev.leaves()
    assert np.array_equal(leaves, c.leaves) and np.array_equal(slots, c.slots)


def test_back_to_a_restores_the_upload(L, torch, case):
    """A -> B -> A: the uploaded bytes (the builder's own) and A's frame. Leaves the scene at A, so it
    runs last; the identity update that follows must change nothing either."""
    c = case
    rec = c.dev.update(c.geoA)
    assert rec.applied == 1 and rec.n_refused == 0
    assert c.dev.nodes().tobytes() == c.nodes0.tobytes(), f"{c.what}: the nodes are not the uploaded ones"
    assert_same(render(L, torch, c.dev, c.st), c.frameA, f"{c.what} frame back at A")
    assert_hits_equal(device_hits(L, torch, c.dev, c.cam_rays), c.hitsA, f"{c.what} hits back at A")
    rec = update_async(L, torch, c.dev, c.geoA)
    assert rec["applied"] == 1
    assert c.dev.nodes().tobytes() == c.nodes0.tobytes(), f"{c.what}: an identity update changed the nodes"
    assert_same(render(L, torch, c.dev, c.st, flags=L.FLAG_LINEAR_SCAN),
                render(L, torch, c.dev, c.st), f"{c.what} scan against tree at A")
    assert_same(render(L, torch, c.dev, c.st), c.frameA, f"{c.what} frame after the identity update")
    c.rec = update_async(L, torch, c.dev, c.geoB)  # back at B for whatever runs after this


# ------------------------------------------------------------------ refusal --
@pytest.fixture(scope="module")
def dome(L, O, torch):
    c = Case()
    c.shape = C.SHAPES["dome"]
    c.A = c.shape.build(O)
    c.geo = C.geometry(c.A)
    c.st = camera(L, c.shape.setup, W, H)
    c.dev = Q.upload(L, c.shape, c.A, bg_struct(L, DEFAULT_BG))
    try:
        assert c.dev.info().bound == 5000.0
        c.nodes0 = c.dev.nodes()
        c.rays, _ = device_camera_rays(L, torch, c.st, params(L))
        c.rays = c.rays.cpu().numpy()
        c.hits0 = device_hits(L, torch, c.dev, c.rays)
        c.frame0 = render(L, torch, c.dev, c.st, flags=L.FLAG_LINEAR_SCAN)
        yield c
    finally:
        c.dev.release()


def _small(c):
    return int(C.small_of(c.A)[7])


REFUSED = {
    "one_ulp_over": lambda g, i: g.__setitem__(i, (5000.0, 0.3, 0.0, 2.0 ** -40)),
    "nan_centre": lambda g, i: g.__setitem__((i, 1), NAN),
    "infinite_radius": lambda g, i: g.__setitem__((i, 3), INF),
    "two_offenders": lambda g, i: (g.__setitem__((i + 9, 2), -6000.0), g.__setitem__((i, 0), NAN)),
}


@pytest.mark.parametrize("which", sorted(REFUSED))
def test_refused_update_leaves_the_scene_alone(L, torch, dome, which):
    c = dome
    i = _small(c)
    g = c.geo.copy()
    REFUSED[which](g, i)
    want = S.check(g, 5000.0)
    assert want[0] == (2 if which == "two_offenders" else 1) and want[1] == i
    for rec in (update_async(L, torch, c.dev, g), c.dev.update(g)):
        rec = {k: rec[k] if isinstance(rec, np.void) else getattr(rec, k) for k in L.SCENE_UPDATE_RECORD_DTYPE.names}
        assert rec["applied"] == 0 and (rec["n_refused"], rec["first_refused"]) == want[:2], (which, rec)
        assert rec["extent"] == want[2] and rec["bound"] == 5000.0 and rec["reserved"] == 0, (which, rec)
        assert c.dev.nodes().tobytes() == c.nodes0.tobytes(), f"{which}: a refused update wrote nodes"
        assert_hits_equal(device_hits(L, torch, c.dev, c.rays), c.hits0, f"{which}: hits after the refusal")
        assert_hits_equal(device_hits(L, torch, c.dev, c.rays, flags=L.FLAG_LINEAR_SCAN), c.hits0,
                          f"{which}: the list after the refusal")
        assert_same(render(L, torch, c.dev, c.st, flags=L.FLAG_LINEAR_SCAN), c.frame0, f"{which}: frame after the refusal")


def test_on_the_bound_is_applied(L, O, torch, dome):
    """hi == M exactly: a small sphere at x = 4999 with R = 1. Then back, for the tests that share the scene."""
    c = dome
    i = _small(c)
    g = c.geo.copy()
    g[i] = (4999.0, 0.3, 0.0, 1.0)
    assert S.check(g, 5000.0) == (0, -1, 5000.0)
    rec = c.dev.update(g)
    assert (rec.applied, rec.n_refused, rec.first_refused, rec.extent, rec.bound) == (1, 0, -1, 5000.0, 5000.0)
    B = c.A.copy()
    B["center"][i], B["radius"][i] = g[i, :3], g[i, 3]
    moved = c.dev.nodes()
    assert moved.tobytes() != c.nodes0.tobytes() and float(moved["box"].max()) > 5000.0  # padded outward
    dev = fresh(L, c.shape, B)
    try:
        assert_hits_equal(device_hits(L, torch, c.dev, c.rays), device_hits(L, torch, dev, c.rays), "on the bound")
        rays = np.array([[4990.0, 0.3, 0.0, 1.0, 0.0, 0.0], [4999.0, 50.0, 0.0, 0.0, -1.0, 0.0]])  # at the moved sphere
        got = device_hits(L, torch, c.dev, rays)
        assert (got["index"] == i).all()
        assert_hits_equal(got, oracle_hits(O, L, B, rays), "rays at the sphere on the bound")
    finally:
        dev.release()
    assert c.dev.update(c.geo).applied == 1
    assert c.dev.nodes().tobytes() == c.nodes0.tobytes()


def test_no_tree_takes_a_nan(L, O, torch):
    """chain15 has no tree: nothing is checked, as at the upload; the frame is a fresh upload's."""
    shape = C.SHAPES["chain15"]
    A = shape.build(O)
    B = C.chain(A)
    B["center"][4, 1] = NAN
    st = camera(L, shape.setup, W, H)
    dev, other = Q.upload(L, shape, A, bg_struct(L, DEFAULT_BG)), fresh(L, shape, B)
    try:
        render(L, torch, dev, st)
        rec = update_async(L, torch, dev, C.geometry(B))
        assert (rec["applied"], rec["n_refused"], rec["first_refused"], rec["bound"]) == (1, 0, -1, 0.0)
        assert rec["extent"] == S.check(C.geometry(B), INF)[2]
        assert len(dev.nodes()) == 0 and dev.info().has_bvh == 0
        assert_same(render(L, torch, dev, st), render(L, torch, other, st), "chain15 with a NaN centre")
    finally:
        dev.release()
        other.release()


def test_wrong_count_is_an_argument_error(L, torch, dome):
    c = dome
    g = torch.zeros((c.dev.n + 1, 4), dtype=torch.float64, device="cuda")
    rec = torch.zeros(4, dtype=torch.float64, device="cuda")
    for n in (c.dev.n - 1, c.dev.n + 1, 0, -1):
        with pytest.raises(L.TrayError) as e:
            c.dev.update_async(g.data_ptr(), n, rec.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert not rec.cpu().numpy().any() and c.dev.nodes().tobytes() == c.nodes0.tobytes()


# ----------------------------------------------------------------- ordering --
def test_update_waits_for_the_renders_before_it(L, O, torch):
    """A contract check, run once: a render of A on one stream, the update to B and a render on another,
    no host synchronisation in between. The first frame is A's, the second B's."""
    shape = C.SHAPES["leaf2"]
    A = shape.build(O)
    B = C.lift(A)
    st = camera(L, shape.setup, W, H)
    devA, devB = fresh(L, shape, A), fresh(L, shape, B)
    dev = fresh(L, shape, A)
    try:
        wantA, wantB = render(L, torch, devA, st), render(L, torch, devB, st)
        assert C.fraction_differing(wantA.reshape(-1, 3), wantB.reshape(-1, 3)) >= 0.4
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        first = torch.full((H, W, 3), NAN, dtype=torch.float64, device="cuda")
        second = torch.full((H, W, 3), NAN, dtype=torch.float64, device="cuda")
        g = torch.from_numpy(C.geometry(B)).cuda()
        rec = torch.zeros(4, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dev.render_async(st, params(L), first.data_ptr(), None, s1.cuda_stream)
        dev.update_async(g.data_ptr(), len(B), rec.data_ptr(), s2.cuda_stream)
        dev.render_async(st, params(L), second.data_ptr(), None, s2.cuda_stream)
        torch.cuda.synchronize()
        assert rec.cpu().numpy().view(L.SCENE_UPDATE_RECORD_DTYPE)[0]["applied"] == 1
        assert_same(first.cpu().numpy(), wantA, "the render enqueued before the update")
        assert_same(second.cpu().numpy(), wantB, "the render enqueued after the update")
    finally:
        for d in (dev, devA, devB):
            d.release()


# ----------------------------------------------------------- Python surface --
def _book(O):
    from tray_amd import ray

    spheres = O.rich_scene(2)
    return ray, spheres, ray.Scene.from_array(spheres, ray.DefaultBackground())


def test_scene_move_updates_in_place(L, O, torch):
    ray, spheres, scene = _book(O)
    st = camera(L, Q.SHAPES[0].setup, W, H)
    rays = device_camera_rays(L, torch, st, params(L))[0].cpu().numpy()
    before = scene.Hit(rays[:, :3], rays[:, 3:])
    dev = scene._uploaded[0][1]
    B = C.lift(spheres)
    assert scene.Move(B["center"]) is True
    assert scene._uploaded[0][1] is dev
    assert np.array_equal(scene.to_array()["center"], B["center"]) and np.array_equal(scene.to_array()["radius"], B["radius"])
    got = scene.Hit(rays[:, :3], rays[:, 3:])
    assert scene._uploaded[0][1] is dev, "Scene.Hit uploaded again after Scene.Move"
    want = ray.Scene.from_array(B, ray.DefaultBackground()).Hit(rays[:, :3], rays[:, 3:])
    assert_hits_equal(got, want, "Scene.Move then Scene.Hit")
    assert C.hits_differing(before, want) >= 0.4
    # radii too
    J = C.jitter(spheres)
    assert scene.Move(J["center"], J["radius"]) is True and scene._uploaded[0][1] is dev
    assert_hits_equal(scene.Hit(rays[:, :3], rays[:, 3:]),
                      ray.Scene.from_array(J, ray.DefaultBackground()).Hit(rays[:, :3], rays[:, 3:]), "with radii")
    # refused: a sphere leaves the ground's 2000
    far = J.copy()
    far["center"][5] = (3000.0, 0.2, 0.0)
    assert scene.Move(far["center"], far["radius"]) is False
    assert 0 not in scene._uploaded and not dev.handle
    got = scene.Hit(rays[:, :3], rays[:, 3:])
    assert scene._uploaded[0][1] is not dev
    assert_hits_equal(got, ray.Scene.from_array(far, ray.DefaultBackground()).Hit(rays[:, :3], rays[:, 3:]),
                      "after a refused Scene.Move")
    assert scene._uploaded[0][1].info().bound > 3000.0


def test_render_animation_equals_fresh_uploads(L, O, torch):
    ray, spheres, scene = _book(O)
    rng = np.random.default_rng(5)
    m = C.small_of(spheres)
    geos, stages = [], []
    cur = spheres.copy()
    for _ in range(3):  # three lifts, one after the other
        cur = cur.copy()
        cur["center"][m, 1] += rng.uniform(0.0, 3.0, len(m))
        stages.append(cur)
        geos.append(C.geometry(cur))

    def tracer():
        t = ray.New(W, H)
        t.Camera = ray.RichSceneCamera()
        t.NumRaysPerPixel, t.MaxDepth, t.RayRadius, t.Seed = R, DEPTH, RADIUS, SEED
        return t

    t = tracer()
    frames = t.RenderAnimation(scene, np.array(geos))
    assert t.applied == [1, 1, 1] and len(frames) == 3
    assert C.geometry(scene.to_array()).tobytes() == geos[-1].tobytes()
    st = camera(L, Q.SHAPES[0].setup, W, H)
    for k, s in enumerate(stages):
        dev = L.DeviceScene(s, bg_struct(L, DEFAULT_BG), 0)
        try:
            linear = render(L, torch, dev, st, pass_=k)
        finally:
            dev.release()
        rgba = np.zeros((H, W, 4), dtype=np.uint8)
        L.check(L.lib().tray_to_srgba(linear.ctypes.data, H * W, rgba.ctypes.data))
        assert np.array_equal(frames[k], rgba), f"frame {k} is not the fresh upload's pass {k}"
        if k == 2:
            assert_same(t.linear, linear, "the last linear frame")
    assert not np.array_equal(frames[0], frames[2])
    # a device tensor, a refused frame in the middle (a sphere beyond the ground's 2000), the filter on
    far = geos[1].copy()
    far[5, :3] = (3000.0, 0.2, 0.0)
    scene2 = ray.Scene.from_array(spheres, ray.DefaultBackground())
    t2 = tracer()
    out = t2.RenderAnimation(scene2, torch.from_numpy(np.array([geos[0], far, geos[2]])).cuda())
    assert t2.applied == [1, 0, 1]
    assert np.array_equal(out[0], frames[0]) and np.array_equal(out[2], frames[2])
    moved = stages[1].copy()
    moved["center"][5] = far[5, :3]
    dev = L.DeviceScene(moved, bg_struct(L, DEFAULT_BG), 0)
    try:
        linear = render(L, torch, dev, st, pass_=1)
    finally:
        dev.release()
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    L.check(L.lib().tray_to_srgba(linear.ctypes.data, H * W, rgba.ctypes.data))
    assert np.array_equal(out[1], rgba), "the refused frame is not the fresh upload's"
    t3 = tracer()
    den = t3.RenderAnimation(ray.Scene.from_array(spheres, ray.DefaultBackground()), np.array(geos[:2]), denoise=True)
    assert t3.applied == [1, 1] and den[1].shape == (H, W, 4) and not np.array_equal(den[1], frames[1])


def test_cli_bounce(capsys, tmp_path):
    """python -m tray_amd -bounce 3: every frame moved in place, the last one saved."""
    from tray_amd import __main__ as cli
    from tray_amd import png

    path = str(tmp_path / "bounce.png")
    assert cli.main(["-width", str(W), "-height", str(H), "-r", str(R), "-d", str(DEPTH), "-seed", "2", "-bounce", "3",
                     "-save", path]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out == [f"frame {k}: moved in place" for k in range(3)]
    last = png.decode_png(open(path, "rb").read())
    assert last.shape == (H, W, 4) and len(np.unique(last[..., :3])) > 16  # a picture, not a blank
