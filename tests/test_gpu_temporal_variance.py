"""include/tray_temporal_variance.h on the device: the step against tray_temporal_step_async (colour,
age, index, depth and the record as bit patterns) and against its numpy restatement
(tests/temporal_variance_ref.py: m2 and the variance), the static camera against the accumulator, the
cap, the variance of listed pixels, the refill chain through the C calls, Tracer.RenderSequence
against a host-driven composition of the same calls, the CLI, and the two quality conditions. Every
output lives between guard words."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import adaptive_ref as A
import temporal_ref as R
import temporal_variance_ref as V
from conftest import DEFAULT_BG, RICH_SETUP, ROOT
from test_gpu_parity import bg_struct, camera
from test_gpu_progressive import GUARD, Guarded
from test_gpu_query import bits, rich2, torch  # noqa: F401 (fixtures)
from test_gpu_temporal import (CAP, DEFAULT_SETUP, Planes, _orbit, _tracer, assert_state, book_frames,  # noqa: F401
                               dev_book, dev_default, device_hits, pair_of, random_history)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
PLAIN = ("colour", "age", "index", "depth")


class VarPlanes(Planes):
    """A tray_temporal_var_state of guarded device planes, optionally filled from host arrays."""

    def __init__(self, L, torch, w, h, host=None):
        super().__init__(L, torch, w, h, host)
        self.m2 = Guarded(torch, w * h * 3)
        if host is not None:
            self.m2.t[GUARD:GUARD + self.m2.n] = torch.from_numpy(
                np.ascontiguousarray(host["m2"], dtype=np.float64).reshape(-1)).cuda()
        self.plain = self.st
        self.st = L.TemporalVarState(self.colour.ptr, self.m2.ptr, self.age.ptr, self.index.ptr, self.depth.ptr, w, h)

    def get(self):
        got = super().get()
        got["m2"] = self.m2.get((self.h, self.w, 3))
        return got


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def var_step(L, torch, dev, cam, prev, tp, frame, history, w, h, variance=True):
    """One tray_temporal_var_step_async into fresh guarded planes: (state dict, variance or None,
    (fresh, age_sum)). The history and the frame must come back untouched."""
    out = VarPlanes(L, torch, w, h)
    hist = VarPlanes(L, torch, w, h, history) if history is not None else None
    ft = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    record = Guarded(torch, 2)
    var = Guarded(torch, w * h * 3) if variance else None
    L.temporal_var_step_async(dev.handle, cam, prev if hist is not None else None, tp, ft.data_ptr(),
                              hist.st if hist is not None else None, out.st, var.ptr if variance else None, record.ptr,
                              stream_of(torch))
    torch.cuda.synchronize()
    if hist is not None:
        got = hist.get()
        for name in got:
            assert np.array_equal(got[name].view(np.uint8), np.ascontiguousarray(history[name]).view(np.uint8)), name
    assert np.array_equal(bits(ft.cpu().numpy()), bits(frame)), "the frame was written"
    rec = record.get().view(np.uint64)
    return out.get(), (var.get((h, w, 3)) if variance else None), (int(rec[0]), int(rec[1]))


def plain_step(L, torch, dev, cam, prev, tp, frame, history, w, h):
    """tray_temporal_step_async on the same inputs (the history without its m2)."""
    out = Planes(L, torch, w, h)
    hist = Planes(L, torch, w, h, history) if history is not None else None
    ft = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    record = Guarded(torch, 2)
    L.temporal_step_async(dev.handle, cam, prev if hist is not None else None, tp, ft.data_ptr(),
                          hist.st if hist is not None else None, out.st, record.ptr, stream_of(torch))
    torch.cuda.synchronize()
    rec = record.get().view(np.uint64)
    return out.get(), (int(rec[0]), int(rec[1]))


def same_bits_or_nan(got, want, what):
    """Bit patterns, except that where the result is a NaN, that it is a NaN is what is compared."""
    bad = np.argwhere((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want)))
    assert bad.size == 0, f"{what}: differs at {len(bad)} elements, first {bad[0]}: " \
                          f"{got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}"


def random_m2(rng, w, h):
    m2 = rng.random((h, w, 3)) * 0.1
    if w * h > 1:
        m2[0, 0] = (INF, NAN, 0.25)  # travels with its colour, decides nothing
        m2[h - 1, w - 1, 1] = -INF
    return m2


@pytest.mark.parametrize("which", ["orbit", "dolly", "turned"])
@pytest.mark.parametrize("w,h", [(33, 17), (1, 1), (64, 36)])
@pytest.mark.parametrize("scene", ["default", "book"])
def test_step_equals_the_plain_step_and_the_restatement(L, torch, dev_default, dev_book, scene, w, h, which):
    """Three chained steps between two cameras (there, back and there again), with the BVH or the scan
    and with TRAY_FLAG_LINEAR_SCAN: colour, age, index, depth and the record have the bits of
    tray_temporal_step_async on the same inputs; m2 and the variance those of the restatement; a null
    variance changes no other output."""
    dev, setup = (dev_default, DEFAULT_SETUP) if scene == "default" else (dev_book, RICH_SETUP)
    s_prev, s_cur = pair_of(setup, which)
    cams = [camera(L, s_prev, w, h), camera(L, s_cur, w, h)]
    rng = np.random.default_rng(w * 1000 + h + len(which))
    frames = rng.random((3, h, w, 3))
    frames[1, h // 2, w // 2, 1] = NAN
    frames[2, 0, 0, 2] = INF
    finals = []
    for flags in (0, L.FLAG_LINEAR_SCAN):
        tp = L.temporal_params(max_history=CAP, flags=flags)
        hits = [device_hits(L, torch, dev, c, w, h, flags) for c in cams]
        history = random_history(np.random.default_rng(5), hits[0], w, h, tp.depth_tolerance)
        history["m2"] = random_m2(np.random.default_rng(6), w, h)
        fresh = []
        for k in range(3):
            cam, prev = cams[(k + 1) & 1], cams[k & 1]
            got, var, rec = var_step(L, torch, dev, cam, prev, tp, frames[k], history, w, h)
            what = f"{scene} {w}x{h} {which} flags {flags} step {k}"
            want, want_rec = plain_step(L, torch, dev, cam, prev, tp, frames[k], history, w, h)
            for name in PLAIN:
                assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), (what, name)
            assert rec == want_rec, what
            ref, ref_var, ref_rec = V.step(cam.as_array(), prev.as_array(), frames[k], hits[(k + 1) & 1], history,
                                           CAP, tp.depth_tolerance, tp.snap)
            assert_state(got, ref, what)
            assert rec == ref_rec, what
            same_bits_or_nan(got["m2"], ref["m2"], what + " m2")
            same_bits_or_nan(var, ref_var, what + " variance")
            if k == 0:
                bare, none, bare_rec = var_step(L, torch, dev, cam, prev, tp, frames[k], history, w, h, variance=False)
                assert none is None and bare_rec == rec
                for name in PLAIN + ("m2",):
                    assert np.array_equal(bare[name].view(np.uint8), got[name].view(np.uint8)), (what, name)
            fresh.append(rec[0])
            history = got
        finals.append(got)
        fresh_now = got["age"] == 1
        assert (got["m2"][fresh_now] == 0).all() and np.isposinf(var[fresh_now]).all()
        if which != "turned" and w * h > 1:
            assert 0 < fresh[0] < w * h, fresh
            assert np.isfinite(got["m2"]).sum() > got["m2"].size // 2 and (got["m2"] > 0).any()
    for name in PLAIN + ("m2",):
        same_bits_or_nan(finals[1][name].astype(np.float64), finals[0][name].astype(np.float64),
                         "TRAY_FLAG_LINEAR_SCAN " + name)


def test_static_camera_equals_the_accumulator_bit_for_bit(L, torch, dev_book):
    """K = 6 steps under one camera at 33 x 17: m2 is tray_accum_fold_async's, the variance
    tray_accum_fold_metric_async's, bit for bit."""
    w, h, K = 33, 17, 6
    st = camera(L, RICH_SETUP, w, h)
    frames = book_frames(L, torch, dev_book, st, w, h, 4, K)
    host = frames.cpu().numpy()
    tp = L.temporal_params()
    assert tp.max_history > K
    state = None
    for k in range(K):
        state, var, rec = var_step(L, torch, dev_book, st, st, tp, host[k], state, w, h)
        assert rec == ((w * h, w * h) if k == 0 else (0, (k + 1) * w * h)), (k, rec)
        mean, m2, variance = (Guarded(torch, w * h * 3) for _ in range(3))
        acc = L.Accum(mean.ptr, m2.ptr, w, h, 0, 0)
        L.accum_fold_metric_async(acc, frames.data_ptr(), k + 1, L.accum_metric_params(), variance.ptr, None, 0,
                                  stream_of(torch))
        torch.cuda.synchronize()
        assert np.array_equal(bits(state["colour"]), bits(mean.get((h, w, 3)))), k
        assert np.array_equal(bits(state["m2"]), bits(m2.get((h, w, 3)))), k
        assert np.array_equal(bits(var), bits(variance.get((h, w, 3)))), k
    assert (state["age"] == K).all() and (state["m2"] > 0).any()
    m2_only = Guarded(torch, w * h * 3)
    mean = Guarded(torch, w * h * 3)
    acc = L.Accum(mean.ptr, m2_only.ptr, w, h, 0, 0)
    L.accum_fold_async(acc, frames.data_ptr(), K, 0, stream_of(torch))
    torch.cuda.synchronize()
    assert np.array_equal(bits(state["m2"]), bits(m2_only.get((h, w, 3))))


@pytest.mark.parametrize("max_history,steps", [(4, 8), (2, 4)])
def test_the_cap_on_the_device(L, torch, dev_book, max_history, steps):
    """A static camera past max_history: the age stops there and m2 follows the (n0 - 1) / (A - 1)
    rule; max_history = 2 builds m2 from a zeroed history. Against the restatement's chain."""
    w, h = 33, 17
    st = camera(L, RICH_SETUP, w, h)
    hits = device_hits(L, torch, dev_book, st, w, h)
    frames = np.random.default_rng(max_history).random((steps, h, w, 3))
    tp = L.temporal_params(max_history=max_history)
    state = ref = None
    for k in range(steps):
        before = state
        state, var, rec = var_step(L, torch, dev_book, st, st, tp, frames[k], state, w, h)
        ref, ref_var, ref_rec = V.step(st.as_array(), st.as_array(), frames[k], hits, ref, max_history)
        assert (state["age"] == min(k + 1, max_history)).all() and rec == ref_rec
        for name in ("colour", "m2"):
            assert np.array_equal(bits(state[name]), bits(ref[name])), (k, name)
        assert np.array_equal(bits(var), bits(ref_var)), k
        if k >= max_history:  # the rule itself, from the device's own previous state
            n0 = max_history - 1
            m = before["m2"] * (np.float64(n0 - 1) / np.float64(max_history - 1))
            t = frames[k] - before["colour"]
            assert np.array_equal(bits(state["m2"]), bits(m + t * (frames[k] - state["colour"]))), k
            if max_history == 2:  # the history's m2 did not survive: this step's term alone
                assert np.array_equal(state["m2"], t * (frames[k] - state["colour"]))


def test_an_age_past_max_history_is_scaled_on_the_device(L, torch, dev_book):
    """As after a refill: ages of 7 and 40 under max_history = 4, an orbit step (bilinear taps of mixed
    ages included)."""
    w, h = 33, 17
    prev, cam = (camera(L, s, w, h) for s in pair_of(RICH_SETUP, "orbit"))
    rng = np.random.default_rng(21)
    tp = L.temporal_params(max_history=4)
    history = random_history(rng, device_hits(L, torch, dev_book, prev, w, h), w, h, tp.depth_tolerance)
    history["age"] = rng.choice(np.array([1, 2, 3, 4, 7, 40], dtype=np.int32), size=(h, w))
    history["m2"] = rng.random((h, w, 3))
    frame = rng.random((h, w, 3))
    got, var, rec = var_step(L, torch, dev_book, cam, prev, tp, frame, history, w, h)
    ref, ref_var, ref_rec = V.step(cam.as_array(), prev.as_array(), frame, device_hits(L, torch, dev_book, cam, w, h),
                                   history, 4, tp.depth_tolerance, tp.snap)
    assert_state(got, ref, "ages past the cap")
    assert rec == ref_rec and got["age"].max() == 4 and 0 <= rec[0] < w * h
    same_bits_or_nan(got["m2"], ref["m2"], "m2")
    same_bits_or_nan(var, ref_var, "variance")


def test_variance_of_listed_pixels(L, torch, dev_book):
    """tray_temporal_var_variance_async: the whole frame equals the step's plane; a list updates
    exactly the listed pixels (guard words and unlisted pixels byte-identical), skips an out-of-range
    entry, and an empty list writes nothing."""
    for w, h in ((33, 17), (1, 1), (64, 36)):
        prev, cam = (camera(L, s, w, h) for s in pair_of(RICH_SETUP, "orbit"))
        rng = np.random.default_rng(w)
        tp = L.temporal_params(max_history=CAP)
        history = random_history(rng, device_hits(L, torch, dev_book, prev, w, h), w, h, tp.depth_tolerance)
        history["m2"] = random_m2(rng, w, h)
        state, step_var, _ = var_step(L, torch, dev_book, cam, prev, tp, rng.random((h, w, 3)), history, w, h)
        planes = VarPlanes(L, torch, w, h, state)
        whole = Guarded(torch, w * h * 3)
        L.temporal_var_variance_async(planes.st, None, 0, whole.ptr, 0, stream_of(torch))
        torch.cuda.synchronize()
        same_bits_or_nan(whole.get((h, w, 3)), step_var, f"{w}x{h} whole frame")
        # the state moves on in some pixels (as a fold would move it); the list names those and more
        px = w * h
        moved = np.unique(rng.integers(0, px, size=max(px // 5, 1))).astype(np.uint32)
        after = {k: v.copy() for k, v in state.items()}
        after["m2"].reshape(px, 3)[moved] = rng.random((len(moved), 3))
        after["age"].reshape(px)[moved] += 3
        planes = VarPlanes(L, torch, w, h, after)
        entries = np.concatenate([moved[::-1], np.array([px, 2 ** 32 - 1], dtype=np.uint32)])
        lst = torch.from_numpy(entries.view(np.int32)).cuda()
        plane = Guarded(torch, px * 3)
        plane.t[GUARD:GUARD + plane.n] = torch.from_numpy(step_var.reshape(-1)).cuda()
        L.temporal_var_variance_async(planes.st, lst.data_ptr(), len(entries), plane.ptr, 0, stream_of(torch))
        torch.cuda.synchronize()
        got = plane.get((h, w, 3))
        want = V.list_variance(after, entries, step_var)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{w}x{h} list"
        untouched = np.ones(px, dtype=bool)
        untouched[moved] = False
        assert np.array_equal(got.reshape(px, 3)[untouched].view(np.uint8),
                              step_var.reshape(px, 3)[untouched].view(np.uint8))
        assert np.isfinite(got.reshape(px, 3)[moved]).all()
        planes.get()  # the state's guards; and it was not written:
        for name, value in planes.get().items():
            assert np.array_equal(value.view(np.uint8), np.ascontiguousarray(after[name]).view(np.uint8)), name
        L.temporal_var_variance_async(planes.st, lst.data_ptr(), 0, whole.ptr, 0, stream_of(torch))  # an empty list
        torch.cuda.synchronize()
        same_bits_or_nan(whole.get((h, w, 3)), step_var, f"{w}x{h} empty list")


def test_refill_chain_through_the_c_calls(L, torch, dev_book):
    """Section 4 at 33 x 17 with R = 3 on frame f = 1 of an orbit: the listed pixels' (colour, m2, age)
    equal adaptive_ref's fold of the list renderer's values, unlisted pixels keep their bytes, every
    list entry held fewer than 4 frames or neighbours such a pixel, the passes are f * 4 + 1 ..
    f * 4 + 3 (each listed pixel against tray_render_async | TRAY_FLAG_ORDERED_SUM at that pass), and
    the list's variance refresh gives the whole-frame variance."""
    w, h, Rf, f = 33, 17, 3, 1
    px = w * h
    prev, cam = (camera(L, s, w, h) for s in pair_of(RICH_SETUP, "orbit"))
    tp = L.temporal_params()
    stream = stream_of(torch)

    def params(pass_, flags=0):
        return L.make_params(w, h, 50, 4, 0.5, 2, flags=flags, pass_=pass_)

    # a history that has seen the previous camera for a while, with a patch that was fresh two frames
    # ago and a block without history
    history = None
    for k in range(5):
        history, _, _ = var_step(L, torch, dev_book, prev, prev, tp,
                                 book_frames(L, torch, dev_book, prev, w, h, 4, 1, seed=30 + k)[0].cpu().numpy(),
                                 history, w, h)
    history["age"][4:7, 5:9] = 2
    history["age"][10:14, 18:22] = 0
    frame = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    dev_book.render_async(cam, params(f * (1 + Rf)), frame.data_ptr(), None, stream)
    torch.cuda.synchronize()
    before, var0, rec = var_step(L, torch, dev_book, cam, prev, tp, frame.cpu().numpy(), history, w, h)
    assert rec[0] > 0
    planes = VarPlanes(L, torch, w, h, before)
    variance = Guarded(torch, px * 3)
    variance.t[GUARD:GUARD + variance.n] = torch.from_numpy(var0.reshape(-1)).cuda()
    ast = planes.st.adaptive()
    ap = L.adaptive_params(tolerance=V.REFILL_TOLERANCE, min_passes=1 + Rf, max_passes=int(tp.max_history), dilate=1)
    nbytes = L.adaptive_workspace_bytes(w, h)
    work = torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda")
    active = Guarded(torch, (px + 1) // 2)
    arecord = Guarded(torch, 4)
    L.adaptive_select_async(ast, ap, active.ptr, arecord.ptr, work.data_ptr(), nbytes, None, 0, stream)
    n_active = int(arecord.get().view(L.ADAPTIVE_RECORD_DTYPE)[0]["n_active"])  # the 32-byte readback
    listed = active.get().view(np.uint32)[:n_active].copy()
    sel = V.refill_list(before, Rf, int(tp.max_history))
    assert np.array_equal(listed, sel["pixels"]) and 0 < n_active < px
    young = before["age"] < 1 + Rf
    near = np.zeros((h + 2, w + 2), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            near[dy:dy + h, dx:dx + w] |= young
    assert near[1:-1, 1:-1].reshape(-1)[listed].all() and young.reshape(-1)[listed].any()
    assert (before["age"][young] > 1).any() and (before["age"][young] == 1).any()
    values = Guarded(torch, Rf * n_active * 3)
    dev_book.render_pixels_async(cam, params(f * (1 + Rf) + 1), active.ptr, n_active, values.ptr, Rf, stream=stream)
    L.adaptive_fold_async(ast, active.ptr, n_active, values.ptr, Rf, 0, stream)
    L.temporal_var_variance_async(planes.st, active.ptr, n_active, variance.ptr, 0, stream)
    torch.cuda.synchronize()
    vals = values.get((Rf, n_active, 3))
    for k in range(Rf):  # the passes: f * 4 + 1 + k, as the ordered-sum render of the whole frame
        full = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        dev_book.render_async(cam, params(f * (1 + Rf) + 1 + k, L.FLAG_ORDERED_SUM), full.data_ptr(), None, stream)
        torch.cuda.synchronize()
        assert np.array_equal(bits(vals[k]), bits(full.cpu().numpy().reshape(px, 3)[listed])), k
    after = planes.get()
    want = V.refill_fold(before, listed, vals)
    for name in ("colour", "m2", "age", "index", "depth"):
        assert np.array_equal(after[name].view(np.uint8), np.ascontiguousarray(want[name]).view(np.uint8)), name
    unlisted = np.ones(px, dtype=bool)
    unlisted[listed] = False
    for name in ("colour", "m2"):
        assert np.array_equal(bits(after[name]).reshape(px, 3)[unlisted], bits(before[name]).reshape(px, 3)[unlisted])
    assert np.array_equal(after["age"].reshape(px), before["age"].reshape(px) + Rf * ~unlisted)
    got_var = variance.get((h, w, 3))
    assert np.array_equal(bits(got_var), bits(A.variance(after["m2"], after["age"])))
    assert np.array_equal(bits(got_var).reshape(px, 3)[unlisted], bits(var0).reshape(px, 3)[unlisted])
    assert np.isfinite(got_var.reshape(px, 3)[listed]).all() and np.isposinf(var0).any()


def compose_sequence(L, torch, dev, cams, w, h, r, seed, refill, denoise, stream, max_history=None):
    """RenderSequence(variance=True, refill, denoise) spelled out in the C calls: (the RGBA frames, the
    last linear frame, the last variance, the last ages, the per-frame list lengths)."""
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    tp = L.temporal_params(**({} if max_history is None else dict(max_history=max_history)))

    def planes():
        t = dict(colour=torch.empty((h, w, 3), **f64), m2=torch.empty((h, w, 3), **f64), age=torch.empty((h, w), **i32),
                 index=torch.empty((h, w), **i32), depth=torch.empty((h, w), **f64))
        return t, L.TemporalVarState(t["colour"].data_ptr(), t["m2"].data_ptr(), t["age"].data_ptr(),
                                     t["index"].data_ptr(), t["depth"].data_ptr(), w, h)

    states = [planes(), planes()]
    frame, variance, shown = (torch.empty((h, w, 3), **f64) for _ in range(3))
    aov = [torch.empty((h, w, 3), **f64), torch.empty((h, w, 3), **f64), torch.empty((h, w), **f64)]
    ap = L.adaptive_params(tolerance=1e150, min_passes=1 + refill, max_passes=int(tp.max_history), dilate=1)
    nbytes = L.adaptive_workspace_bytes(w, h)
    work = torch.empty((nbytes // 8,), **f64)
    active = torch.empty((h * w,), **i32)
    arecord = torch.empty((4,), **f64)
    values = torch.empty((max(refill, 1) * h * w * 3,), **f64)
    dp = L.denoise_variance_params(w, h)
    dbytes = L.denoise_variance_workspace_bytes(dp)
    dwork = torch.empty((max(dbytes, 8) // 8,), **f64)
    rgba = torch.empty((len(cams), h, w, 4), dtype=torch.uint8, device="cuda")
    refilled = []
    for k, cam in enumerate(cams):
        p = L.make_params(w, h, 50, r, 0.5, seed, pass_=k * (1 + refill))
        dev.render_async(cam, p, frame.data_ptr(), None, stream)
        out = states[k & 1]
        L.temporal_var_step_async(dev.handle, cam, cams[k - 1] if k else None, tp, frame.data_ptr(),
                                  states[(k - 1) & 1][1] if k else None, out[1], variance.data_ptr(), None, stream)
        if refill:
            ast = out[1].adaptive()
            L.adaptive_select_async(ast, ap, active.data_ptr(), arecord.data_ptr(), work.data_ptr(), nbytes, None, 0,
                                    stream)
            n = int(arecord.cpu().numpy().view(L.ADAPTIVE_RECORD_DTYPE)[0]["n_active"])
            refilled.append(n)
            if n:
                dev.render_pixels_async(cam, L.make_params(w, h, 50, r, 0.5, seed, pass_=k * (1 + refill) + 1),
                                        active.data_ptr(), n, values.data_ptr(), refill, stream=stream)
                L.adaptive_fold_async(ast, active.data_ptr(), n, values.data_ptr(), refill, 0, stream)
                L.temporal_var_variance_async(out[1], active.data_ptr(), n, variance.data_ptr(), 0, stream)
        src = out[0]["colour"]
        if denoise:
            dev.render_aov_async(cam, p, aov[0].data_ptr(), aov[1].data_ptr(), aov[2].data_ptr(), stream=stream)
            L.denoise_variance_async(src.data_ptr(), variance.data_ptr(), dp, shown.data_ptr(), dwork.data_ptr(),
                                     dbytes, aov[0].data_ptr(), aov[1].data_ptr(), aov[2].data_ptr(), device=0,
                                     stream=stream)
            src = shown
        L.linear_to_srgba_async(src.data_ptr(), h * w, rgba[k].data_ptr(), 0, stream)
    last = states[(len(cams) - 1) & 1][0]
    return (rgba.cpu().numpy(), last["colour"].cpu().numpy(), variance.cpu().numpy(), last["age"].cpu().numpy(),
            refilled)


def test_render_sequence_equals_the_composed_calls(L, torch, rich2, dev_book):
    """RenderSequence(variance=True, refill=3, denoise=True) at 64 x 36 over 4 cameras against the same
    calls driven from here; then two such sequences in flight on two streams give the solo bits."""
    w, h, n = 64, 36, 4
    t, ray = _tracer(w, h, 4)
    scene = ray.RichScene(2)
    frames = t.RenderSequence(scene, _orbit(ray, n), denoise=True, variance=True, refill=3)
    cams = [camera(L, R.orbit_setup(RICH_SETUP, k * ray.ORBIT_STEP_DEGREES), w, h) for k in range(n)]
    rgba, linear, variance, age, refilled = compose_sequence(L, torch, dev_book, cams, w, h, 4, 2, 3, True,
                                                             stream_of(torch))
    assert np.array_equal(frames[-1], rgba[-1]) and all(np.array_equal(a, b) for a, b in zip(frames, rgba))
    assert np.array_equal(bits(t.linear), bits(linear)) and np.array_equal(bits(t.variance), bits(variance))
    assert np.array_equal(t.age, age) and t.refilled == refilled and refilled[0] == w * h
    assert all(x < w * h for x in refilled[1:]) and sum(refilled[1:]) > 0, refilled
    assert t.pixel_passes == n * w * h + 3 * sum(refilled)
    assert t.age.min() >= 4 and np.isfinite(t.variance).all()  # every pixel holds 1 + R frames or more
    assert np.array_equal(bits(t.variance), bits(A.variance(t.m2, t.age)))
    assert t.filtered.shape == (h, w, 3) and not np.array_equal(t.filtered, t.linear)
    # variance alone: the colour and the ages of the plain sequence, bit for bit
    t2, _ = _tracer(w, h, 4)
    t2.RenderSequence(scene, _orbit(ray, n))
    t3, _ = _tracer(w, h, 4)
    t3.RenderSequence(scene, _orbit(ray, n), variance=True)
    assert np.array_equal(bits(t3.linear), bits(t2.linear)) and np.array_equal(t3.age, t2.age)
    assert t3.fresh == t2.fresh and t3.mean_age == t2.mean_age and t3.refilled == [0] * n
    assert np.array_equal(bits(t3.variance), bits(A.variance(t3.m2, t3.age)))
    # two sequences, two streams, two threads
    jobs = [(_orbit(ray, n), 3), (_orbit(ray, n, 2.5), 1)]
    solo = []
    for cameras, refill in jobs:
        ts, _ = _tracer(w, h, 4)
        solo.append((ts.RenderSequence(scene, cameras, denoise=True, refill=refill), ts.linear.copy(), ts.variance))
    both, errors = [None, None], []

    def run(j):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                tj, _ = _tracer(w, h, 4)
                both[j] = (tj.RenderSequence(scene, jobs[j][0], denoise=True, refill=jobs[j][1]), tj.linear.copy(),
                           tj.variance)
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(e)

    scene._device_scene(0)  # uploaded before the threads share it
    threads = [threading.Thread(target=run, args=(j,)) for j in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for got, want in zip(both, solo):
        assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0]))
        assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[2]), bits(want[2]))


def test_cli_orbit_variance_refill(L, rich2, tmp_path):
    out = str(tmp_path / "orbit.png")
    r = subprocess.run([sys.executable, "-m", "tray_amd", "-width", "64", "-height", "36", "-r", "4", "-orbit", "3",
                        "-variance", "-refill", "3", "-denoise", "-save", out], capture_output=True, text=True,
                       cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and all(line.startswith(f"frame {k}: fresh ") for k, line in enumerate(lines)), r.stdout
    assert lines[0] == f"frame 0: fresh 1.0000 mean age 1.000 refilled {64 * 36}"
    later = [int(line.rsplit(" ", 1)[1]) for line in lines[1:]]
    assert all(x < 64 * 36 for x in later) and sum(later) > 0, r.stdout
    assert os.path.getsize(out) > 0 and open(out, "rb").read(8) == b"\x89PNG\r\n\x1a\n"


@pytest.fixture(scope="module")
def truth_of(L, rich2):
    """An independent r = 4096 frame of a camera at 160 x 90, as test_gpu_temporal builds its reference."""
    def render(cam):
        cam.Initialize(160, 90)
        return L.render(rich2, bg_struct(L, DEFAULT_BG), cam._state, L.make_params(160, 90, 50, 4096, 0.5, 77), 0)[0]
    return render


def test_refill_lowers_the_error_of_the_fresh_pixels(L, torch, rich2, truth_of):
    """8a. The 160 x 90 book cover at r = 4 over an 8-frame orbit of 1 degree: over the pixels that are
    fresh in the last frame of the run without refill, the MSE against an r = 4096 frame with refill=3
    is below the MSE without (expected near one quarter: 16 samples for 4). Both filtered frames'
    MSEs relative to the unfiltered frame are printed without a condition (at a mean age near 7 the
    two filters are not far apart)."""
    w, h, n = 160, 90, 8
    scene = None
    runs = {}
    for refill in (0, 3):
        t, ray = _tracer(w, h, 4)
        scene = scene or ray.RichScene(2)
        t.RenderSequence(scene, _orbit(ray, n), denoise=True, variance=True, refill=refill)
        runs[refill] = t
    truth = truth_of(_orbit(ray, n)[-1])
    fresh = runs[0].age == 1
    assert 0 < fresh.sum() < w * h / 2
    mse = {R_: float(((t.linear - truth)[fresh] ** 2).mean()) for R_, t in runs.items()}
    whole = {R_: float(((t.linear - truth) ** 2).mean()) for R_, t in runs.items()}
    print(f"fresh pixels {int(fresh.sum())}: MSE {mse[3]:.4e} with refill=3 against {mse[0]:.4e} without, ratio "
          f"{mse[3] / mse[0]:.4f}; whole frame {whole[3]:.4e} against {whole[0]:.4e}, ratio {whole[3] / whole[0]:.4f}; "
          f"refilled {runs[3].refilled}, pixel-passes {runs[3].pixel_passes} against {runs[0].pixel_passes}")
    assert mse[3] < mse[0]
    t = runs[0]
    tp, _ = _tracer(w, h, 4)
    tp.RenderSequence(scene, _orbit(ray, n), denoise=True)  # the plain filter on the same accumulated frame
    assert np.array_equal(bits(tp.linear), bits(t.linear))
    rel_plain = float(((tp.filtered - truth) ** 2).mean()) / whole[0]
    rel_var = float(((t.filtered - truth) ** 2).mean()) / whole[0]
    rel_var3 = float(((runs[3].filtered - truth) ** 2).mean()) / whole[3]
    print(f"orbit, mean age {t.mean_age[-1]:.2f}: filtered MSE relative to unfiltered: plain {rel_plain:.4f}, "
          f"variance-guided {rel_var:.4f} (fresh pixels carry an infinite variance); with refill=3 (every variance "
          f"finite) variance-guided {rel_var3:.4f}")


def test_variance_guided_filter_beats_the_plain_one_on_a_still_camera(L, torch, rich2, truth_of):
    """8b. A still camera for 32 frames (128 samples in every pixel): denoise=True with variance=True has
    a lower MSE against the r = 4096 frame than denoise=True without."""
    w, h, n = 160, 90, 32
    t, ray = _tracer(w, h, 4)
    scene = ray.RichScene(2)
    still = [ray.RichSceneCamera() for _ in range(n)]
    t.RenderSequence(scene, still, denoise=True, variance=True)
    assert (t.age == n).all()
    truth = truth_of(ray.RichSceneCamera())
    t2, _ = _tracer(w, h, 4)
    t2.RenderSequence(scene, still, denoise=True)
    assert np.array_equal(bits(t2.linear), bits(t.linear))  # one accumulated frame, two filters
    base = float(((t.linear - truth) ** 2).mean())
    mse_plain = float(((t2.filtered - truth) ** 2).mean())
    mse_var = float(((t.filtered - truth) ** 2).mean())
    print(f"still camera, {n} frames: MSE unfiltered {base:.4e}; relative to it: plain filter {mse_plain / base:.4f}, "
          f"variance-guided {mse_var / base:.4f}")
    assert mse_var < mse_plain
