"""include/tray_temporal.h on the device: the reprojection step against its numpy restatement
(tests/temporal_ref.py) as bit patterns, the static camera against tray_accum_fold_async, the first
frame and the history cap, the quality condition over an orbit, and Tracer.RenderSequence with the
CLI. The restatement's centre-ray hits come from tray_scene_hit_async on the same rays."""
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_ref as R
from conftest import DEFAULT_BG, RICH_SETUP, ROOT
from test_gpu_parity import bg_struct, camera
from test_gpu_progressive import GUARD, Guarded
from test_gpu_query import bits, rich2, torch  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
DEFAULT_SETUP = np.array([-2.0, 2.0, 1.0, 0, 0, -1.0, 0, 1, 0, 20.0, 1.0, 12.0 ** 0.5, 0.1])  # tracer.go:52-58
CAP = 8  # max_history of the bit-pattern cases: the random ages run past it


@pytest.fixture(scope="module")
def dev_book(L, rich2, torch):
    dev = L.DeviceScene(rich2, bg_struct(L, DEFAULT_BG), 0)
    assert dev.info().has_bvh == 1
    yield dev
    dev.release()


@pytest.fixture(scope="module")
def dev_default(L, O, torch):
    dev = L.DeviceScene(O.default_scene(), bg_struct(L, DEFAULT_BG), 0)
    assert dev.info().has_bvh == 0
    yield dev
    dev.release()


def pair_of(setup, which):
    """(previous setup, current setup) of a camera pair."""
    cur = np.array(setup, dtype=np.float64)
    if which == "orbit":
        cur = R.orbit_setup(setup, 1.0)
    elif which == "dolly":
        cur[0:3] = cur[0:3] + 0.1 * (cur[3:6] - cur[0:3])
    elif which == "turned":
        cur = R.orbit_setup(setup, 120.0)
    return np.array(setup, dtype=np.float64), cur


def device_hits(L, torch, dev, cam, w, h, flags=0):
    """tray_scene_hit_async on the centre rays of the restatement: (index, t)."""
    o, d = R.centre_rays(cam.as_array(), w, h)
    rays = np.concatenate([np.broadcast_to(o, d.shape), d], axis=-1).reshape(-1, 6)
    rt = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    hits = torch.zeros((w * h, 8), dtype=torch.float64, device="cuda")
    dev.hit_async(rt.data_ptr(), w * h, hits.data_ptr(), flags=flags, stream=torch.cuda.current_stream().cuda_stream)
    rec = hits.cpu().numpy().reshape(-1).view(L.HIT_DTYPE)
    return rec["index"].reshape(h, w).astype(np.int32), rec["t"].reshape(h, w).copy()


class Planes:
    """A tray_temporal_state of guarded device planes, optionally filled from host arrays."""

    def __init__(self, L, torch, w, h, host=None):
        px = w * h
        self.w, self.h = w, h
        self.colour, self.depth = Guarded(torch, px * 3), Guarded(torch, px)
        self.age, self.index = Guarded(torch, (px + 1) // 2), Guarded(torch, (px + 1) // 2)
        if host is not None:
            for g, a in ((self.colour, host["colour"]), (self.depth, host["depth"])):
                g.t[GUARD:GUARD + g.n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).cuda()
            for g, a in ((self.age, host["age"]), (self.index, host["index"])):
                g.t[GUARD:GUARD + g.n].view(torch.int32)[:px] = torch.from_numpy(
                    np.ascontiguousarray(a, dtype=np.int32).reshape(-1)).cuda()
        self.st = L.TemporalState(self.colour.ptr, self.age.ptr, self.index.ptr, self.depth.ptr, w, h)

    def get(self):
        px, w, h = self.w * self.h, self.w, self.h
        return dict(colour=self.colour.get((h, w, 3)), depth=self.depth.get((h, w)),
                    age=self.age.get().view(np.int32)[:px].reshape(h, w),
                    index=self.index.get().view(np.int32)[:px].reshape(h, w))


def device_step(L, torch, dev, cam, prev, tp, frame, history, w, h, stream=None):
    """One tray_temporal_step_async into fresh guarded planes: (state dict, (fresh, age_sum))."""
    out = Planes(L, torch, w, h)
    hist = Planes(L, torch, w, h, history) if history is not None else None
    ft = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    record = Guarded(torch, 2)
    L.temporal_step_async(dev.handle, cam, prev if hist is not None else None, tp, ft.data_ptr(),
                          hist.st if hist is not None else None, out.st, record.ptr,
                          stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if hist is not None:
        got = hist.get()  # the guards of the history, and that it was not written
        for name in got:
            assert np.array_equal(got[name].view(np.uint8), np.ascontiguousarray(history[name]).view(np.uint8)), name
    assert np.array_equal(bits(ft.cpu().numpy()), bits(frame)), "the frame was written"
    rec = record.get().view(np.uint64)
    return out.get(), (int(rec[0]), int(rec[1]))


def assert_state(got, want, what):
    for name in ("index", "age"):
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, f"{what}: {name} differs at {len(bad)} pixels, first {bad[0]}: " \
                              f"{got[name][tuple(bad[0])]} for {want[name][tuple(bad[0])]}"
    for name in ("depth", "colour"):  # a NaN is a NaN: its sign and payload are not the contract's
        bad = np.argwhere((bits(got[name]) != bits(want[name])) & ~(np.isnan(got[name]) & np.isnan(want[name])))
        assert bad.size == 0, f"{what}: {name} differs at {len(bad)} elements, first {bad[0]}: " \
                              f"{got[name][tuple(bad[0])]!r} for {want[name][tuple(bad[0])]!r}"


def random_history(rng, prev_hits, w, h, tolerance):
    """The previous camera's true hits under random colours, with what the taps must refuse mixed in:
    NaN colours, zero and negative ages, ages at and past the cap, other indices, and depths just
    inside and just outside the relative tolerance."""
    index, depth = prev_hits[0].copy(), prev_hits[1].copy()
    colour = rng.random((h, w, 3))
    age = rng.integers(1, CAP + 5, size=(h, w)).astype(np.int32)
    kind = rng.integers(0, 12, size=(h, w))
    colour[kind == 0, rng.integers(0, 3)] = NAN
    age[kind == 1] = 0
    age[kind == 2] = -3
    age[kind == 3] = CAP
    index[kind == 4] += 1
    index[(kind == 5) & (index >= 0)] = -1
    for k, f in ((6, 1 + tolerance * 0.999), (7, 1 + tolerance * 1.001), (8, 1 - tolerance * 0.999),
                 (9, 1 - tolerance * 1.001)):
        depth[kind == k] = depth[kind == k] * f
    colour[0, 0] = (INF, 0.5, -INF) if w * h > 1 else colour[0, 0]
    return dict(colour=colour, age=age, index=index, depth=depth)


@pytest.mark.parametrize("which", ["orbit", "dolly", "turned"])
@pytest.mark.parametrize("w,h", [(33, 17), (1, 1), (64, 36)])
@pytest.mark.parametrize("scene", ["default", "book"])
def test_step_equals_the_restatement_bit_for_bit(L, torch, dev_default, dev_book, scene, w, h, which):
    """All four planes and the record, for the BVH (book cover) and the scan (default scene), an open
    and a closed lens (the step does not sample the lens) and TRAY_FLAG_LINEAR_SCAN."""
    dev, setup = (dev_default, DEFAULT_SETUP) if scene == "default" else (dev_book, RICH_SETUP)
    s_prev, s_cur = pair_of(setup, which)
    rng = np.random.default_rng(w * 1000 + h + len(which))
    tp = L.temporal_params(max_history=CAP)
    frame = rng.random((h, w, 3))
    frame[h // 2, w // 2, 1] = NAN
    results = []
    for aperture in (float(setup[12]), 0.0):
        s_prev[12] = s_cur[12] = aperture
        prev, cam = camera(L, s_prev, w, h), camera(L, s_cur, w, h)
        hits = device_hits(L, torch, dev, cam, w, h)
        history = random_history(np.random.default_rng(5), device_hits(L, torch, dev, prev, w, h), w, h,
                                 tp.depth_tolerance)
        want, want_rec = R.step(cam.as_array(), prev.as_array(), frame, hits, history, CAP, tp.depth_tolerance,
                                tp.snap)
        got, rec = device_step(L, torch, dev, cam, prev, tp, frame, history, w, h)
        assert_state(got, want, f"{scene} {w}x{h} {which} aperture {aperture}")
        assert rec == want_rec == (int((got["age"] == 1).sum()), int(got["age"].astype(np.int64).sum()))
        assert got["age"].min() >= 1 and got["age"].max() <= CAP
        results.append((got, rec))
        scan, scan_rec = device_step(L, torch, dev, cam, prev, L.temporal_params(max_history=CAP,
                                                                                 flags=L.FLAG_LINEAR_SCAN),
                                     frame, history, w, h)
        assert_state(scan, got, "TRAY_FLAG_LINEAR_SCAN")
        assert scan_rec == rec
    assert_state(results[1][0], results[0][0], "the lens changed the step")
    px = w * h
    fresh = results[0][1][0]
    print(f"{scene} {w}x{h} {which}: fresh {fresh} of {px}, age sum {results[0][1][1]}")
    if which != "turned" and px > 1:
        assert 0 < fresh < px, "the case exercises neither the fold nor the fresh path"
    if which == "dolly" and px > 1:
        z, u, v, ok = R.project(cam.as_array(), prev.as_array(), w, h, *hits)
        assert (ok & ~R.snapped_mask(u, v, tp.snap)).any(), "no bilinear tap"


def book_frames(L, torch, dev, st, w, h, r, passes, seed=2):
    frames = torch.empty((passes, h, w, 3), dtype=torch.float64, device="cuda")
    for k in range(passes):
        p = L.make_params(w, h, 50, r, 0.5, seed, pass_=k)
        dev.render_async(st, p, frames[k].data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return frames


def test_static_camera_equals_the_accumulator_bit_for_bit(L, torch, dev_book):
    """K = 6 steps under one camera: every pixel takes its own history with weight 1, so the colour is
    tray_accum_fold_async's mean over the same frames, every age is 6 and nothing is fresh after the
    first step."""
    w, h, K = 64, 36, 6
    st = camera(L, RICH_SETUP, w, h)
    frames = book_frames(L, torch, dev_book, st, w, h, 4, K)
    host = frames.cpu().numpy()
    mean = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda")
    m2 = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda")
    acc = L.Accum(mean.data_ptr(), m2.data_ptr(), w, h, 0, 0)
    L.accum_fold_async(acc, frames.data_ptr(), K, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tp = L.temporal_params()
    assert tp.max_history > K
    state = None
    for k in range(K):
        state, rec = device_step(L, torch, dev_book, st, st, tp, host[k], state, w, h)
        assert rec == ((w * h, w * h) if k == 0 else (0, (k + 1) * w * h)), (k, rec)
    assert (state["age"] == K).all()
    assert np.array_equal(bits(state["colour"]), bits(mean.cpu().numpy()))


def test_first_frame_and_the_cap(L, torch, dev_book):
    w, h = 33, 17
    prev, cam = (camera(L, s, w, h) for s in pair_of(RICH_SETUP, "orbit"))
    rng = np.random.default_rng(9)
    frame = rng.random((h, w, 3))
    hits = device_hits(L, torch, dev_book, cam, w, h)
    first, rec = device_step(L, torch, dev_book, cam, None, L.temporal_params(), frame, None, w, h)
    assert np.array_equal(bits(first["colour"]), bits(frame)) and (first["age"] == 1).all()
    assert rec == (w * h, w * h)
    assert np.array_equal(first["index"], hits[0]) and np.array_equal(
        bits(first["depth"]), bits(np.where(hits[0] >= 0, hits[1], INF)))
    history = random_history(rng, device_hits(L, torch, dev_book, prev, w, h), w, h, 0.1)
    capped, rec = device_step(L, torch, dev_book, cam, prev, L.temporal_params(max_history=1), frame, history, w, h)
    assert_state(capped, first, "max_history = 1")
    assert rec == (w * h, w * h)


def _tracer(w, h, r, seed=2):
    from tray_amd import ray

    t = ray.New(w, h)
    t.NumRaysPerPixel, t.MaxDepth, t.Seed = r, 50, seed
    return t, ray


def _orbit(ray, n, step=None):
    step = ray.ORBIT_STEP_DEGREES if step is None else step
    return [ray.Orbit(ray.RichSceneCamera(), k * step) for k in range(n)]


def test_an_orbit_beats_its_last_frame_alone(L, torch, rich2):
    """The 160 x 90 book cover at r = 4 over an 8-frame orbit at the CLI's default step: the
    accumulated last frame is closer (MSE) to an independent r = 4096 frame of the last camera than
    that camera's single r = 4 frame is; and on every frame after the first disocclusions exist and
    history survives."""
    w, h, n = 160, 90, 8
    t, ray = _tracer(w, h, 4)
    scene = ray.RichScene(2)
    t.RenderSequence(scene, _orbit(ray, n))
    last = _orbit(ray, n)[-1]
    last.Initialize(w, h)
    bg = bg_struct(L, DEFAULT_BG)
    truth = L.render(rich2, bg, last._state, L.make_params(w, h, 50, 4096, 0.5, 77), 0)[0]
    single = L.render(rich2, bg, last._state, L.make_params(w, h, 50, 4, 0.5, 2, pass_=n - 1), 0)[0]
    mse_seq, mse_one = float(((t.linear - truth) ** 2).mean()), float(((single - truth) ** 2).mean())
    print(f"orbit of {n} at {ray.ORBIT_STEP_DEGREES} deg: MSE {mse_seq:.4e} against {mse_one:.4e} for the single "
          f"frame, ratio {mse_seq / mse_one:.4f}; fresh {t.fresh}, mean age {t.mean_age}")
    assert mse_seq < mse_one
    assert t.fresh[0] == w * h
    for f in t.fresh[1:]:
        assert 0 < f < w * h / 2, t.fresh


def test_render_sequence_repeats_and_its_fields_agree(L, torch, rich2):
    w, h, n = 64, 36, 3
    t, ray = _tracer(w, h, 4)
    scene = ray.RichScene(2)
    a = t.RenderSequence(scene, _orbit(ray, n))
    linear, age = t.linear.copy(), t.age.copy()
    assert len(a) == n and all(f.shape == (h, w, 4) and f.dtype == np.uint8 for f in a)
    assert len(t.fresh) == len(t.mean_age) == n and t.fresh[0] == w * h and t.mean_age[0] == 1.0
    assert t.mean_age[-1] == float(age.astype(np.int64).sum()) / (w * h) and t.fresh[-1] == int((age == 1).sum())
    assert age.min() >= 1 and age.max() <= n
    t2, _ = _tracer(w, h, 4)
    b = t2.RenderSequence(scene, _orbit(ray, n))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(bits(t2.linear), bits(linear))
    assert np.array_equal(a[-1], t.imageData)
    d = t2.RenderSequence(scene, _orbit(ray, n), denoise=True, max_history=2)
    assert len(d) == n and t2.age.max() <= 2 and not np.array_equal(d[-1], a[-1])


def test_cli_orbit(L, rich2, tmp_path):
    out = str(tmp_path / "orbit.png")
    r = subprocess.run([sys.executable, "-m", "tray_amd", "-width", "64", "-height", "36", "-r", "4", "-orbit", "3",
                        "-save", out], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and all(line.startswith(f"frame {k}: fresh ") for k, line in enumerate(lines)), r.stdout
    assert lines[0] == "frame 0: fresh 1.0000 mean age 1.000"
    assert os.path.getsize(out) > 0 and open(out, "rb").read(8) == b"\x89PNG\r\n\x1a\n"


def test_two_sequences_in_flight_on_two_streams_give_the_solo_bits(L, torch, dev_book):
    """Two three-step chains (ping-pong states, different camera pairs), solo and then both in flight
    on two streams without a host wait in between."""
    w, h, K = 64, 36, 3
    tp = L.temporal_params()
    chains = []
    for j in range(2):
        cams = [camera(L, R.orbit_setup(RICH_SETUP, (j + 1) * 1.5 * k), w, h) for k in range(K)]
        frames = book_frames(L, torch, dev_book, cams[0], w, h, 4, K, seed=3 + j)
        chains.append((cams, frames))

    def alloc():  # on the current stream: waited for before anything is enqueued on another
        return [Planes(L, torch, w, h), Planes(L, torch, w, h)], torch.zeros((K, 2), dtype=torch.int64, device="cuda")

    def enqueue(cams, frames, states, records, stream):
        for k in range(K):
            L.temporal_step_async(dev_book.handle, cams[k], cams[k - 1] if k else None, tp, frames[k].data_ptr(),
                                  states[(k - 1) & 1].st if k else None, states[k & 1].st, records[k].data_ptr(),
                                  stream)
        return states[(K - 1) & 1], records

    solo = []
    for cams, frames in chains:
        st, rec = enqueue(cams, frames, *alloc(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        solo.append((st.get(), rec.cpu().numpy()))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    buffers = [alloc(), alloc()]
    torch.cuda.synchronize()
    both = [enqueue(cams, frames, *buf, s.cuda_stream) for (cams, frames), buf, s in zip(chains, buffers, streams)]
    torch.cuda.synchronize()
    for (st, rec), (want, want_rec) in zip(both, solo):
        assert_state(st.get(), want, "two streams")
        assert np.array_equal(rec.cpu().numpy(), want_rec)
    assert 0 < solo[0][1][-1, 0] < w * h
