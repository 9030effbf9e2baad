"""include/tray_temporal_motion.h on the device: the step on a scene whose spheres moved against its
numpy restatement (tests/temporal_motion_ref.py) as bit patterns, on a scene moved in place and on a
fresh upload of the same geometry; its two reductions to the static steps; the one argument error that
needs a real scene; the quality condition over an animation; Tracer.RenderAnimation(temporal=True)
and the CLI. The restatement's centre-ray hits come from tray_scene_hit_async on the moved scene.
Every output lives between guard words."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_update_cases as C
import temporal_motion_ref as M
import temporal_ref as R
from conftest import DEFAULT_BG, RICH_SETUP, ROOT
from test_gpu_parity import bg_struct, camera
from test_gpu_progressive import GUARD, Guarded
from test_gpu_query import bits, rich2, torch  # noqa: F401 (fixtures)
from test_gpu_temporal import (CAP, DEFAULT_SETUP, Planes, _tracer, assert_state, dev_book, device_hits,  # noqa: F401
                               device_step, pair_of, random_history)
from test_gpu_temporal_variance import VarPlanes, random_m2, same_bits_or_nan, stream_of, var_step

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
UNWRITTEN = 7.0  # what the motion plane holds before the call
# The default scene's camera (tracer.go:52-58) with a vertical field of view of 90 degrees for its 20:
# `lift` raises the default scene's two moved spheres by 2.4, above the narrow frame (and above one of 60 degrees).
WIDE_SETUP = np.array(DEFAULT_SETUP, dtype=np.float64)
WIDE_SETUP[9] = 90.0


def own_copy(O, rich2, scene):
    """The scene with one visible glass sphere's radius negated (a hollow sphere, as the reference's
    own default scene once had): the fixtures have no negative radius. On the default scene that is the
    outer glass sphere (list index 2, R = 0.5 -> -0.5), which also puts it among the spheres the
    motions move (radius < 0.5), so that a moved sphere is in view; on the book cover the first small
    glass sphere the 33 x 17 camera sees."""
    if scene == "default":
        s = O.default_scene().copy()
        assert s["material"][2] == 3 and s["radius"][2] == 0.5
        s["radius"][2] = -0.5
        return s, 2
    s = rich2.copy()
    cam = O.camera_initialize(RICH_SETUP, 33, 17)[1]
    seen = np.unique(R.oracle_hits(O, s, cam, 33, 17)[0])
    g = int(next(i for i in seen if i >= 0 and s["material"][i] == 3 and s["radius"][i] < 0.5))
    s["radius"][g] = -s["radius"][g]
    return s, g


class Moved:
    pass


@pytest.fixture(scope="module", params=[(s, m) for s in ("default", "book") for m in ("jitter", "lift", "perm")],
                ids=lambda p: f"{p[0]}-{p[1]}")
def moved(request, L, O, torch, rich2):
    """A (uploaded and kept), A moved to B by tray_scene_update_async, and B uploaded afresh."""
    c = Moved()
    c.scene, c.motion = request.param
    c.A, c.glass = own_copy(O, rich2, c.scene)
    c.B = C.MOTIONS[c.motion](c.A)
    if c.B["radius"][c.glass] == c.A["radius"][c.glass]:
        c.B["radius"][c.glass] *= 1.125  # lift and perm keep the radii: one changes here
    c.geoA, c.geoB = C.geometry(c.A), C.geometry(c.B)
    c.is_moved = (c.geoA != c.geoB).any(axis=1)
    assert c.is_moved.any() and not c.is_moved.all() and (c.geoB[:, 3] < 0).any()
    assert (c.geoA[:, 3] != c.geoB[:, 3]).any()
    bg = bg_struct(L, DEFAULT_BG)
    c.setup = WIDE_SETUP if c.scene == "default" else RICH_SETUP
    c.devA, c.devU, c.devF = (L.DeviceScene(s, bg, 0) for s in (c.A, c.A, c.B))
    try:
        assert c.devU.info().has_bvh == (0 if c.scene == "default" else 1)
        g = torch.from_numpy(c.geoB).cuda()
        rec = torch.zeros(4, dtype=torch.float64, device="cuda")
        c.devU.update_async(g.data_ptr(), len(c.geoB), rec.data_ptr(), stream_of(torch))
        torch.cuda.synchronize()
        assert rec.cpu().numpy().view(L.SCENE_UPDATE_RECORD_DTYPE)[0]["applied"] == 1
        yield c
    finally:
        for d in (c.devA, c.devU, c.devF):
            d.release()


def as_var_state(L, planes):
    st = planes.st
    if isinstance(st, L.TemporalVarState):
        return st
    return L.TemporalVarState(st.colour, None, st.age, st.index, st.depth, st.width, st.height)


def motion_step(L, torch, dev, cam, prev, prev_geometry, tp, frame, history, w, h, m2, n=None):
    """One tray_temporal_motion_step_async into fresh guarded planes: (state dict, variance or None,
    (fresh, age_sum), motion plane). The history, the frame and the previous geometry must come back
    untouched."""
    make = VarPlanes if m2 else Planes
    out = make(L, torch, w, h)
    hist = make(L, torch, w, h, history) if history is not None else None
    ft = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    record = Guarded(torch, 2)
    var = Guarded(torch, w * h * 3) if m2 else None
    motion = Guarded(torch, w * h * 2, fill=UNWRITTEN)
    pg = np.ascontiguousarray(prev_geometry, dtype=np.float64)
    geo = Guarded(torch, max(pg.size, 1))
    geo.t[GUARD:GUARD + pg.size] = torch.from_numpy(pg.reshape(-1)).cuda()
    L.temporal_motion_step_async(dev.handle, cam, prev if hist is not None else None, geo.ptr,
                                 len(pg) if n is None else n, tp, ft.data_ptr(),
                                 as_var_state(L, hist) if hist is not None else None, as_var_state(L, out),
                                 var.ptr if m2 else None, motion.ptr, record.ptr, stream_of(torch))
    torch.cuda.synchronize()
    if hist is not None:
        got = hist.get()
        for name in got:
            assert np.array_equal(got[name].view(np.uint8), np.ascontiguousarray(history[name]).view(np.uint8)), name
    assert np.array_equal(bits(ft.cpu().numpy()), bits(frame)), "the frame was written"
    assert np.array_equal(bits(geo.get()[:pg.size]), bits(pg.reshape(-1))), "the previous geometry was written"
    rec = record.get().view(np.uint64)
    return out.get(), (var.get((h, w, 3)) if m2 else None), (int(rec[0]), int(rec[1])), motion.get((h, w, 2))


@pytest.mark.parametrize("which", ["static", "orbit"])
@pytest.mark.parametrize("w,h", [(33, 17), (1, 1), (64, 36)])
def test_step_equals_the_restatement_bit_for_bit(L, torch, moved, w, h, which):
    """All planes (colour, m2, age, index, depth, variance, motion) and the record against the
    restatement on the current hits of the moved scene; with and without m2; TRAY_FLAG_LINEAR_SCAN the
    same bits; the scene moved in place and the fresh upload the same bits."""
    c = moved
    s_prev, s_cur = pair_of(c.setup, which)
    prev, cam = camera(L, s_prev, w, h), camera(L, s_cur, w, h)
    rng = np.random.default_rng(w * 1000 + h + len(which))
    frame = rng.random((h, w, 3))
    frame[h // 2, w // 2, 1] = NAN
    tp = L.temporal_params(max_history=CAP)
    prev_hits = device_hits(L, torch, c.devA, prev, w, h)
    hits = device_hits(L, torch, c.devU, cam, w, h)
    fresh_hits = device_hits(L, torch, c.devF, cam, w, h)
    assert np.array_equal(hits[0], fresh_hits[0]) and np.array_equal(bits(hits[1]), bits(fresh_hits[1]))
    for m2 in (False, True):
        history = random_history(np.random.default_rng(5), prev_hits, w, h, tp.depth_tolerance)
        if m2:
            history["m2"] = random_m2(np.random.default_rng(6), w, h)
        what = f"{c.scene} {c.motion} {w}x{h} {which} m2 {m2}"
        want, want_var, want_rec, want_motion = M.step(cam.as_array(), prev.as_array(), frame, hits, history, c.geoB,
                                                       c.geoA, m2, CAP, tp.depth_tolerance, tp.snap)
        first = None
        for dev, where in ((c.devU, "moved in place"), (c.devF, "uploaded afresh")):
            for flags in (0, L.FLAG_LINEAR_SCAN):
                tpf = L.temporal_params(max_history=CAP, flags=flags)
                got, var, rec, motion = motion_step(L, torch, dev, cam, prev, c.geoA, tpf, frame, history, w, h, m2)
                here = f"{what}, {where}, flags {flags}"
                assert_state(got, want, here)
                assert rec == want_rec == (int((got["age"] == 1).sum()), int(got["age"].astype(np.int64).sum())), here
                same_bits_or_nan(motion, want_motion, here + " motion")
                if m2:
                    same_bits_or_nan(got["m2"], want["m2"], here + " m2")
                    same_bits_or_nan(var, want_var, here + " variance")
                if first is None:
                    first = got
                for name in got:  # the four runs: the same bits (a NaN's payload included)
                    assert np.array_equal(got[name].view(np.uint8), first[name].view(np.uint8)), (here, name)
        if w * h == 1:
            continue
        # what the case must contain
        on_moved = np.where(hits[0] >= 0, c.is_moved[np.maximum(hits[0], 0)], False)
        folded = want["age"] > 1
        z, u, v, ok = M.project(cam.as_array(), prev.as_array(), w, h, hits[0], np.where(hits[0] >= 0, hits[1], INF),
                                c.geoB, c.geoA)
        bilinear = ok & ~R.snapped_mask(u, v, tp.snap) & folded
        counts = (int((folded & on_moved).sum()), int((folded & (hits[0] >= 0) & ~on_moved).sum()),
                  int((~folded).sum()), int(bilinear.sum()))
        print(f"{what}: folded on moved spheres {counts[0]}, on unmoved spheres {counts[1]}, fresh {counts[2]}, "
              f"bilinear {counts[3]}")
        assert min(counts) > 0, (what, counts)


def test_equal_geometries_give_the_static_steps_bits(L, torch, dev_book, rich2):
    """The book cover at 64 x 36 over an orbit step with prev_geometry equal to the scene's: every plane
    and the record of tray_temporal_step_async without m2 and of tray_temporal_var_step_async with;
    the motion plane is (u - x, v - y) of the static projection; a null history leaves it unwritten."""
    w, h = 64, 36
    prev, cam = (camera(L, s, w, h) for s in pair_of(RICH_SETUP, "orbit"))
    geo = C.geometry(rich2)
    rng = np.random.default_rng(8)
    frame = rng.random((h, w, 3))
    tp = L.temporal_params(max_history=CAP)
    hits = device_hits(L, torch, dev_book, cam, w, h)
    history = random_history(np.random.default_rng(5), device_hits(L, torch, dev_book, prev, w, h), w, h,
                             tp.depth_tolerance)
    got, none, rec, motion = motion_step(L, torch, dev_book, cam, prev, geo, tp, frame, history, w, h, False)
    want, want_rec = device_step(L, torch, dev_book, cam, prev, tp, frame, history, w, h)
    assert none is None and rec == want_rec and 0 < rec[0] < w * h
    for name in want:
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name
    z, u, v, ok = R.project(cam.as_array(), prev.as_array(), w, h, *hits)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    assert np.array_equal(np.isnan(motion).all(axis=-1), ~ok) and ok.any() and not ok.all()
    assert np.array_equal(bits(motion[ok]), bits(np.stack([u - x, v - y], axis=-1)[ok]))
    history["m2"] = random_m2(np.random.default_rng(6), w, h)
    got, var, rec, motion2 = motion_step(L, torch, dev_book, cam, prev, geo, tp, frame, history, w, h, True)
    want, want_var, want_rec = var_step(L, torch, dev_book, cam, prev, tp, frame, history, w, h)
    assert rec == want_rec
    for name in want:
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name
    assert np.array_equal(var.view(np.uint8), want_var.view(np.uint8))
    assert np.array_equal(motion2.view(np.uint8), motion.view(np.uint8))
    for m2 in (False, True):  # the first frame, and max_history = 1: prev_geometry ignored, no motion written
        first, _, rec, untouched = motion_step(L, torch, dev_book, cam, None, np.zeros((0, 4)), tp, frame, None, w, h,
                                               m2, n=len(geo))
        assert rec == (w * h, w * h) and (untouched == UNWRITTEN).all()
        assert np.array_equal(bits(first["colour"]), bits(frame))
        one, _, rec, untouched = motion_step(L, torch, dev_book, cam, prev, geo, L.temporal_params(max_history=1),
                                             frame, history, w, h, m2)
        assert rec == (w * h, w * h) and (untouched == UNWRITTEN).all()


def test_a_sphere_count_other_than_the_scenes_is_refused(L, torch, dev_book, rich2):
    """The one argument error that looks at the scene: before anything is enqueued, nothing written."""
    w, h = 33, 17
    cam = camera(L, RICH_SETUP, w, h)
    geo = C.geometry(rich2)
    frame = np.zeros((h, w, 3))
    for n in (len(geo) - 1, len(geo) + 1, 0, -1):
        with pytest.raises(L.TrayError) as e:
            motion_step(L, torch, dev_book, cam, cam, geo, L.temporal_params(), frame,
                        dict(colour=frame, age=np.ones((h, w), np.int32), index=np.zeros((h, w), np.int32),
                             depth=np.ones((h, w))), w, h, False, n=n)
        assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT and "n_spheres" in str(e.value), n


# ---- Tracer.RenderAnimation(temporal=True) ----------------------------------------------------

def book_tracer(w, h, r):
    t, ray = _tracer(w, h, r)
    t.Camera = ray.RichSceneCamera()
    return t, ray


def compose_animation(L, torch, spheres, geos, cams, w, h, r, seed):
    """RenderAnimation(temporal=True) spelled out with EVERY frame's geometry uploaded afresh: (the RGBA
    frames, the last linear frame, the last ages, the per-frame (fresh, age_sum))."""
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    stream = stream_of(torch)
    tp = L.temporal_params()

    def planes():
        t = dict(colour=torch.empty((h, w, 3), **f64), age=torch.empty((h, w), **i32),
                 index=torch.empty((h, w), **i32), depth=torch.empty((h, w), **f64))
        return t, L.TemporalVarState(t["colour"].data_ptr(), None, t["age"].data_ptr(), t["index"].data_ptr(),
                                     t["depth"].data_ptr(), w, h)

    states = [planes(), planes()]
    frame = torch.empty((h, w, 3), **f64)
    geo = torch.from_numpy(np.ascontiguousarray(geos)).cuda()
    records = torch.zeros((len(geos), 2), dtype=torch.int64, device="cuda")
    rgba = torch.empty((len(geos), h, w, 4), dtype=torch.uint8, device="cuda")
    for k in range(len(geos)):
        s = spheres.copy()
        s["center"], s["radius"] = geos[k][:, :3], geos[k][:, 3]
        dev = L.DeviceScene(s, bg_struct(L, DEFAULT_BG), 0)
        try:
            dev.render_async(cams[k], L.make_params(w, h, 50, r, 0.5, seed, pass_=k), frame.data_ptr(), None, stream)
            out = states[k & 1]
            L.temporal_motion_step_async(dev.handle, cams[k], cams[k - 1] if k else None,
                                         geo[k - 1].data_ptr() if k else None, len(s), tp, frame.data_ptr(),
                                         states[(k - 1) & 1][1] if k else None, out[1], None, None,
                                         records[k].data_ptr(), stream)
            L.linear_to_srgba_async(out[0]["colour"].data_ptr(), h * w, rgba[k].data_ptr(), 0, stream)
            torch.cuda.synchronize()
        finally:
            dev.release()
    last = states[(len(geos) - 1) & 1][0]
    return rgba.cpu().numpy(), last["colour"].cpu().numpy(), last["age"].cpu().numpy(), \
        [(int(a), int(b)) for a, b in records.cpu().numpy()]


def test_render_animation_temporal(L, torch, rich2):
    """At 64 x 36, r = 4, over ray.Bounce: repeats bit for bit; equals the calls composed here with every
    frame uploaded afresh; a frame whose geometry leaves the scene's bound is re-uploaded (applied 0)
    and the frames after it still fold; equal geometries under given cameras are RenderSequence's
    bits; cameras without temporal only replace the camera."""
    w, h, n = 64, 36, 5
    t, ray = book_tracer(w, h, 4)
    scene = ray.RichScene(2)
    spheres = scene.to_array().copy()
    geos = ray.Bounce(scene, n)
    frames = t.RenderAnimation(scene, geos, temporal=True)
    assert t.applied == [1] * n and len(frames) == n and t.fresh[0] == w * h
    assert all(0 < f < w * h for f in t.fresh[1:]) and all(b > a for a, b in zip(t.mean_age, t.mean_age[1:]))
    assert C.geometry(scene.to_array()).tobytes() == geos[-1].tobytes()
    cam = ray.RichSceneCamera()
    cam.Initialize(w, h)
    rgba, linear, age, recs = compose_animation(L, torch, spheres, geos, [cam._state] * n, w, h, 4, 2)
    assert all(np.array_equal(a, b) for a, b in zip(frames, rgba))
    assert np.array_equal(bits(t.linear), bits(linear)) and np.array_equal(t.age, age)
    assert t.fresh == [r[0] for r in recs] and t.mean_age == [r[1] / (w * h) for r in recs]
    t2, _ = book_tracer(w, h, 4)
    again = t2.RenderAnimation(ray.RichScene(2), torch.from_numpy(geos).cuda(), temporal=True)  # a device tensor
    assert all(np.array_equal(a, b) for a, b in zip(frames, again)) and np.array_equal(bits(t2.linear), bits(t.linear))
    assert np.array_equal(t2.age, t.age) and t2.fresh == t.fresh
    # a refused frame in the middle: a small sphere beyond the ground's 2000
    far = geos.copy()
    small = int(np.nonzero(geos[0][:, 3] < 0.5)[0][0])
    far[2, small, :3] = (3000.0, 0.2, 0.0)
    t3, _ = book_tracer(w, h, 4)
    out = t3.RenderAnimation(ray.RichScene(2), far, temporal=True)
    assert t3.applied == [1, 1, 0, 1, 1]
    rgba, linear, age, recs = compose_animation(L, torch, spheres, far, [cam._state] * n, w, h, 4, 2)
    assert all(np.array_equal(a, b) for a, b in zip(out, rgba)) and np.array_equal(bits(t3.linear), bits(linear))
    assert all(b > a for a, b in zip(t3.mean_age, t3.mean_age[1:])) and t3.fresh[3] < w * h / 2, t3.mean_age
    # variance and refill ride along: the plain run's colour without refill, every pixel at 1 + R frames with
    t4, _ = book_tracer(w, h, 4)
    t4.RenderAnimation(ray.RichScene(2), geos, temporal=True, variance=True)
    assert np.array_equal(bits(t4.linear), bits(t.linear)) and t4.refilled == [0] * n and t4.fresh == t.fresh
    t5, _ = book_tracer(w, h, 4)
    t5.RenderAnimation(ray.RichScene(2), geos, temporal=True, refill=3, denoise=True)
    assert t5.refilled[0] == w * h and all(0 < x < w * h for x in t5.refilled[1:]) and t5.age.min() >= 4
    assert np.isfinite(t5.variance).all() and t5.filtered.shape == (h, w, 3)
    assert t5.pixel_passes == n * w * h + 3 * sum(t5.refilled)
    # equal geometries under a moving camera: RenderSequence
    still = np.repeat(C.geometry(spheres)[None], n, axis=0)
    orbit = lambda: [ray.Orbit(ray.RichSceneCamera(), k * ray.ORBIT_STEP_DEGREES) for k in range(n)]  # noqa: E731
    t6, _ = book_tracer(w, h, 4)
    t6.RenderAnimation(ray.RichScene(2), still, temporal=True, cameras=orbit())
    t7, _ = book_tracer(w, h, 4)
    t7.RenderSequence(ray.RichScene(2), orbit())
    assert np.array_equal(bits(t6.linear), bits(t7.linear)) and np.array_equal(t6.age, t7.age)
    assert t6.fresh == t7.fresh and t6.mean_age == t7.mean_age
    # without temporal: today's path; the same camera given explicitly changes nothing
    t8, _ = book_tracer(w, h, 4)
    plain = t8.RenderAnimation(ray.RichScene(2), geos[:2])
    t9, _ = book_tracer(w, h, 4)
    given = t9.RenderAnimation(ray.RichScene(2), geos[:2], cameras=[ray.RichSceneCamera(), ray.RichSceneCamera()])
    assert all(np.array_equal(a, b) for a, b in zip(plain, given)) and np.array_equal(bits(t8.linear), bits(t9.linear))
    assert not hasattr(t8, "fresh") and t8.applied == [1, 1]


def test_an_animation_beats_its_last_frame_alone(L, torch, rich2):
    """The 160 x 90 book cover at r = 4 over ray.Bounce(scene, 8): the accumulated last frame is closer
    (MSE) to an independent r = 4096 frame of the last geometry than that geometry's single r = 4
    frame is. Printed without a condition: the same ratio over the pixels of moved spheres, and over
    the pixels fresh in the last frame with and without refill=3. (Measured once on an MI355X: 0.764
    whole frame, 0.559 on moved spheres, 1.000 and, with refill=3, 0.249 on the fresh pixels; the CPU
    sweep tools/temporal_motion_sweep.py gives 0.67-0.74 whole frame at three smaller sizes.)"""
    w, h, n = 160, 90, 8
    t, ray = book_tracer(w, h, 4)
    scene = ray.RichScene(2)
    geos = ray.Bounce(scene, n)
    t.RenderAnimation(scene, geos, temporal=True)
    last = scene.to_array()
    assert C.geometry(last).tobytes() == geos[-1].tobytes()
    cam = ray.RichSceneCamera()
    cam.Initialize(w, h)
    bg = bg_struct(L, DEFAULT_BG)
    truth = L.render(last, bg, cam._state, L.make_params(w, h, 50, 4096, 0.5, 77), 0)[0]
    single = L.render(last, bg, cam._state, L.make_params(w, h, 50, 4, 0.5, 2, pass_=n - 1), 0)[0]
    t3, _ = book_tracer(w, h, 4)
    t3.RenderAnimation(ray.RichScene(2), geos, temporal=True, refill=3)
    dev = L.DeviceScene(last, bg, 0)
    try:
        index = device_hits(L, torch, dev, cam._state, w, h)[0]
    finally:
        dev.release()
    on_moved = np.where(index >= 0, (geos[-1] != geos[0]).any(axis=1)[np.maximum(index, 0)], False)
    fresh = t.age == 1

    def ratio(linear, mask=None):
        mask = np.ones((h, w), dtype=bool) if mask is None else mask
        return float(((linear - truth)[mask] ** 2).mean()) / float(((single - truth)[mask] ** 2).mean())

    whole = ratio(t.linear)
    print(f"bounce of {n}: MSE ratio against the last frame alone {whole:.4f} whole frame, "
          f"{ratio(t.linear, on_moved):.4f} on the {int(on_moved.sum())} pixels of moved spheres, "
          f"{ratio(t.linear, fresh):.4f} on the {int(fresh.sum())} pixels fresh in the last frame and "
          f"{ratio(t3.linear, fresh):.4f} there with refill=3 (whole frame {ratio(t3.linear):.4f}); "
          f"fresh {t.fresh}, mean age {t.mean_age}, refilled {t3.refilled}")
    assert on_moved.any() and fresh.any() and t.fresh[0] == w * h
    assert whole < 1


def test_cli_bounce_temporal(L, tmp_path):
    out = str(tmp_path / "bounce.png")
    r = subprocess.run([sys.executable, "-m", "tray_amd", "-width", "64", "-height", "36", "-r", "4", "-bounce", "3",
                        "-temporal", "-variance", "-refill", "-save", out], capture_output=True, text=True, cwd=ROOT,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and all(line.startswith(f"frame {k}: fresh ") for k, line in enumerate(lines)), r.stdout
    assert lines[0] == f"frame 0: fresh 1.0000 mean age 1.000 refilled {64 * 36}"
    later = [int(line.rsplit(" ", 1)[1]) for line in lines[1:]]
    assert all(x < 64 * 36 for x in later) and sum(later) > 0, r.stdout
    assert os.path.getsize(out) > 0 and open(out, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
