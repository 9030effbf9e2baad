"""The guided a-trous denoiser (include/tray_denoise.h) on the device.

Contract: every value is a fixed sequence of correctly rounded FP64 operations in
the header's order, so every comparison here is of bit patterns, against the
numpy restatement tests/denoise_ref.py (written from the header). `out` is
pre-filled with NaN so that an unwritten pixel shows, the workspace lies between
guard words that must come back unchanged, and its inside is pre-filled with NaN
too (a level that read what no level wrote would show).
"""
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref as R
from conftest import DEFAULT_BG, RICH_SETUP, ROOT
from test_gpu_parity import bg_struct, camera
from test_gpu_query import bits, rich2, torch  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 64  # doubles on each side of the workspace
GUARD_WORD = -0x5A5A5A5A5A5A5A5B  # as int64
NAN = float("nan")


# ------------------------------------------------------------------ helpers --
def synthetic(rows, width, seed=11, special=True):
    """Colour, albedo, normal, depth with smooth regions, edges and (special) every awkward
    value the header names: zero, negative, infinite and NaN depths, NaN and infinite colours,
    NaN normals, zero and NaN albedo (the 2^-10 floor)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:rows, :width]
    region = ((xx * 3) // max(width, 1) + 2 * ((yy * 2) // max(rows, 1))).astype(np.int64)  # up to 6 flat regions
    base = rng.random((6, 3))
    albedo = 0.1 + 0.9 * base[region % 6]
    colour = albedo * (0.5 + 0.1 * rng.normal(size=(rows, width, 3)))
    normal = np.zeros((rows, width, 3))
    normal[..., 2] = 1.0
    normal[region % 2 == 1] = (0.6, 0.0, 0.8)
    normal = normal + 0.01 * rng.normal(size=normal.shape)
    depth = 2.0 + region + 0.01 * rng.random((rows, width))
    if special and rows * width >= 400:
        depth[: rows // 4, : width // 3] = 0.0  # a sky region: u = 0
        pick = lambda k: (rng.integers(0, rows, k), rng.integers(0, width, k))  # noqa: E731
        depth[pick(5)] = -1.5
        depth[pick(5)] = np.inf
        depth[pick(5)] = np.nan
        colour[pick(4)] = np.nan
        y, x = pick(3)
        colour[y, x, 1] = np.nan  # one channel only
        colour[pick(2)] = np.inf
        normal[pick(4)] = np.nan
        albedo[pick(6)] = 0.0
        y, x = pick(3)
        albedo[y, x, 2] = 2.0 ** -11
        albedo[pick(2)] = np.nan
    return colour, albedo, normal, depth


class Call:
    """One tray_denoise_async call in three steps, so that several can be in flight: the constructor
    uploads the inputs, pre-fills `out` and the workspace and writes the guard words (no
    synchronisation); enqueue() only enqueues on `stream`; result() must follow a synchronisation and
    returns the host result after verifying the guard words."""

    def __init__(self, L, torch, colour, albedo=None, normal=None, depth=None, **params):
        self.L, self.torch = L, torch
        rows, width = colour.shape[:2]
        self.p = L.denoise_params(width, rows, **params)
        self.need = L.denoise_workspace_bytes(self.p)
        assert self.need % 8 == 0
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
        self.inputs = [dev(colour), dev(albedo), dev(normal), dev(depth)]
        self.out = torch.full((rows, width, 3), NAN, dtype=torch.float64, device="cuda")
        self.work = torch.full((2 * GUARD + self.need // 8,), NAN, dtype=torch.float64, device="cuda")
        guards = self.work.view(torch.int64)
        guards[:GUARD] = GUARD_WORD
        guards[GUARD + self.need // 8:] = GUARD_WORD

    def enqueue(self, stream=None):
        c, a, n, z = self.inputs
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.L.denoise_async(c.data_ptr(), self.p, self.out.data_ptr(),
                             self.work.data_ptr() + 8 * GUARD if self.need else None, self.need, ptr(a), ptr(n),
                             ptr(z), 0, (stream or self.torch.cuda.current_stream()).cuda_stream)

    def result(self):
        g = self.work.view(self.torch.int64).cpu().numpy()
        assert (g[:GUARD] == GUARD_WORD).all() and (g[GUARD + self.need // 8:] == GUARD_WORD).all(), \
            "guard words changed"
        return self.out.cpu().numpy()


def device_denoise(L, torch, colour, albedo=None, normal=None, depth=None, stream=None, **params):
    """One call alone: set up, synchronise, enqueue on `stream`, synchronise, host result."""
    call = Call(L, torch, colour, albedo, normal, depth, **params)
    torch.cuda.synchronize()
    call.enqueue(stream)
    torch.cuda.synchronize()
    return call.result()


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at {i}: "
                             f"{got[i]!r} ({bits(got)[i]:#x}) for {want[i]!r} ({bits(want)[i]:#x})")


# --------------------------------- 1. synthetic images against the restatement ---
# 37x23: no multiple of the 32x8 tile or of 64, and at 5 iterations the +-32 taps leave the image
# from most pixels; 1x1, 1x40, 40x1: every tap but the centre's row or column is outside; 70x45
# at 1 iteration (no workspace: straight into out) and at 8 (spacing 128 > the image: 1-pixel
# sub-images, both ping-pong buffers several times). 100x40 has more than one tile each way
# at spacing 1 and 2 (sub-images of 100x40 and 50x20 against 32x8 tiles).
CASES = [(23, 37, 5), (1, 1, 5), (1, 40, 5), (40, 1, 5), (45, 70, 1), (45, 70, 2), (45, 70, 8), (40, 100, 3)]


@pytest.mark.parametrize("rows,width,iterations", CASES)
def test_synthetic_images_bit_for_bit(L, torch, rows, width, iterations):
    colour, albedo, normal, depth = synthetic(rows, width)
    for flags in (1, 0):
        kw = dict(iterations=iterations, flags=flags, sigma_color=0.75, sigma_normal=0.5, sigma_depth=0.25)
        want = R.denoise(colour, albedo, normal, depth, **kw)
        got = device_denoise(L, torch, colour, albedo, normal, depth, **kw)
        assert_same_bits(got, want, f"{width}x{rows} {iterations} iterations flags {flags}")
        if rows * width >= 400:  # the case proves what it says: it filtered, and NaNs stayed where they were
            assert np.array_equal(np.isnan(got), np.isnan(colour)) and np.isnan(colour).any()
            assert not np.array_equal(got[np.isfinite(colour)], colour[np.isfinite(colour)])


GUIDES = {"no_albedo": ("normal", "depth"), "no_normal": ("albedo", "depth"), "no_depth": ("albedo", "normal"),
          "none": (), "all": ("albedo", "normal", "depth")}


@pytest.mark.parametrize("which", sorted(GUIDES))
def test_each_guide_null_and_the_flag_on_and_off(L, torch, which):
    colour, albedo, normal, depth = synthetic(23, 37, seed=5)
    have = {k: v for k, v in dict(albedo=albedo, normal=normal, depth=depth).items() if k in GUIDES[which]}
    results = {}
    for flags in ((0, 1) if "albedo" in have else (0,)):
        kw = dict(iterations=3, flags=flags, sigma_color=0.75, sigma_normal=0.5, sigma_depth=0.25)
        want = R.denoise(colour, have.get("albedo"), have.get("normal"), have.get("depth"), **kw)
        results[flags] = got = device_denoise(L, torch, colour, **have, **kw)
        assert_same_bits(got, want, f"guides {which} flags {flags}")
    if len(results) == 2:
        assert not np.array_equal(bits(results[0]), bits(results[1]))
    if "albedo" not in have:  # the flag needs it: refused, nothing written
        with pytest.raises(L.TrayError) as e:
            device_denoise(L, torch, colour, **have, iterations=3, flags=1)
        assert e.value.code == L.TRAY_ERR_INVALID_ARGUMENT


def test_default_parameters_on_a_synthetic_image(L, torch):
    colour, albedo, normal, depth = synthetic(45, 70, seed=9)
    got = device_denoise(L, torch, colour, albedo, normal, depth)
    assert_same_bits(got, R.denoise(colour, albedo, normal, depth), "default parameters")


# ----------------------------------------------- 2. the book cover on the device ---
@pytest.fixture(scope="module")
def dev_book(L, rich2, torch):
    dev = L.DeviceScene(rich2, bg_struct(L, DEFAULT_BG), 0)
    yield dev
    dev.release()


def book_frame(L, torch, dev, w, h, r, pass_=0, aov=True):
    """tray_render_async (F64) and tray_render_aov_async of the w x h book cover, seed 2, d = 50."""
    st = camera(L, RICH_SETUP, w, h)
    p = L.make_params(w, h, 50, r, 0.5, 2, pass_=pass_)
    stream = torch.cuda.current_stream().cuda_stream
    colour = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda")
    dev.render_async(st, p, colour.data_ptr(), None, stream)
    g = {}
    if aov:
        g = {"albedo": torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda"),
             "normal": torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda"),
             "depth": torch.full((h, w), NAN, dtype=torch.float64, device="cuda")}
        dev.render_aov_async(st, p, g["albedo"].data_ptr(), g["normal"].data_ptr(), g["depth"].data_ptr(),
                             stream=stream)
    torch.cuda.synchronize()
    return colour.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}


@pytest.fixture(scope="module")
def book64(L, torch, dev_book):
    colour, g = book_frame(L, torch, dev_book, 64, 36, 16)
    return colour, g, R.denoise(colour, g["albedo"], g["normal"], g["depth"])


def test_book_cover_64x36_bit_for_bit(L, torch, book64):
    colour, g, want = book64
    assert np.isfinite(colour).all() and (g["depth"] == 0).any() and (g["depth"] > 0).any()
    got = device_denoise(L, torch, colour, g["albedo"], g["normal"], g["depth"])
    assert_same_bits(got, want, "book cover 64x36 r = 16")
    assert not np.array_equal(got, colour)


def test_non_default_stream(L, torch, book64):
    colour, g, want = book64
    got = device_denoise(L, torch, colour, g["albedo"], g["normal"], g["depth"], stream=torch.cuda.Stream())
    assert_same_bits(got, want, "non-default stream")


def test_two_calls_in_flight_on_two_streams(L, torch, book64):
    """Two calls enqueued back to back on two streams, each with a workspace of its own and nothing
    between them that waits: every buffer of both calls is set up first and the device synchronised
    once, then A goes on s1 and B on s2, then one synchronisation. On the 64x36 book cover both must
    equal the restatement. On a 1280x720 frame (5 launches of 50 to 80 us each, so A is still
    running while B is enqueued and starts) the two differ in their inputs, and each must equal the
    same call made alone before: the restatement would take numpy a minute at that size, and that
    the device equals it is what the other tests show."""
    colour, g, want = book64
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = Call(L, torch, colour, g["albedo"], g["normal"], g["depth"])
    b = Call(L, torch, colour, g["albedo"], g["normal"], g["depth"])
    torch.cuda.synchronize()
    a.enqueue(s1)
    b.enqueue(s2)
    torch.cuda.synchronize()
    assert_same_bits(a.result(), want, "stream 1 of 2")
    assert_same_bits(b.result(), want, "stream 2 of 2")

    big_a = synthetic(720, 1280, seed=21)
    big_b = synthetic(720, 1280, seed=22)
    alone_a = device_denoise(L, torch, *big_a)
    alone_b = device_denoise(L, torch, *big_b)
    assert not np.array_equal(bits(alone_a), bits(alone_b))
    a, b = Call(L, torch, *big_a), Call(L, torch, *big_b)
    assert a.work.data_ptr() != b.work.data_ptr() and a.need == 2 * 720 * 1280 * 24
    torch.cuda.synchronize()
    a.enqueue(s1)
    b.enqueue(s2)
    torch.cuda.synchronize()
    assert_same_bits(a.result(), alone_a, "1280x720, stream 1 of 2")
    assert_same_bits(b.result(), alone_b, "1280x720, stream 2 of 2")


def _tracer(w, h, r, seed=2, depth=50):
    from tray_amd import ray

    t = ray.New(w, h)
    t.Camera = ray.RichSceneCamera()
    t.NumRaysPerPixel, t.MaxDepth, t.Seed = r, depth, seed
    return ray, t


def test_tracer_denoise_equals_the_c_call(L, torch, rich2, book64):
    colour, g, want = book64
    ray, t = _tracer(64, 36, 16)
    aov = t.RenderAOV(ray.Scene.from_array(rich2))
    for name in ("albedo", "normal", "depth"):
        assert np.array_equal(bits(aov[name]), bits(g[name])), name
    assert_same_bits(t.Denoise(colour, aov), want, "Tracer.Denoise")
    kw = dict(iterations=2, flags=0, sigma_color=0.25)
    assert_same_bits(t.Denoise(colour, {"depth": aov["depth"]}, **kw),
                     R.denoise(colour, None, None, g["depth"], **kw), "Tracer.Denoise with overrides")
    part = t.Denoise(colour[4:20], {k: aov[k][4:20] for k in ("albedo", "normal", "depth")}, yStart=4, yEnd=20)
    assert_same_bits(part, R.denoise(colour[4:20], g["albedo"][4:20], g["normal"][4:20], g["depth"][4:20]), "rows 4..20")
    with pytest.raises(ValueError):
        t.Denoise(colour, aov, tile_rows=2)
    assert t.Denoise(colour[:0], {}, yStart=3, yEnd=3, flags=0).shape == (0, 64, 3)


def test_render_denoised_equals_the_composition(L, torch, rich2):
    """RenderDenoised = Render's linear frame -> RenderAOV -> Denoise -> tray_to_srgba, byte for byte."""
    w, h, r = 48, 27, 8
    ray, t = _tracer(w, h, r)
    scene = ray.Scene.from_array(rich2)
    got = t.RenderDenoised(scene).copy()
    linear = t.linear.copy()
    ray2, t2 = _tracer(w, h, r)
    t2.Render(ray2.Scene.from_array(rich2))
    den = t2.Denoise(t2.linear, t2.RenderAOV(ray2.Scene.from_array(rich2)))
    assert_same_bits(linear, den, "RenderDenoised's linear frame")
    rgba = np.zeros((h, w, 4), dtype=np.uint8)
    L.check(L.lib().tray_to_srgba(den.ctypes.data, h * w, rgba.ctypes.data))
    assert got.shape == (h, w, 4) and got.dtype == np.uint8 and np.array_equal(got, rgba)
    assert not np.array_equal(got, t2.imageData)  # and it is not the unfiltered frame


def test_cli_writes_the_denoised_png(L, rich2, tmp_path):
    from tray_amd import png

    save, prefix = str(tmp_path / "frame.png"), str(tmp_path / "guide")
    r = subprocess.run([sys.executable, "-m", "tray_amd", "-width", "48", "-height", "27", "-r", "8", "-d", "50",
                        "-denoise", "-save", save, "-aov", prefix], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ray, t = _tracer(48, 27, 8)  # the CLI's defaults: seed 2 for the scene and the draws
    want = t.RenderDenoised(ray.RichScene(2))
    for path in (save, prefix + "_denoised.png"):
        img = png.decode_png(open(path, "rb").read())
        assert img.shape == (27, 48, 4) and np.array_equal(img, want), path


# --------------------------------------------------------- 3. quality condition ---
def test_mse_against_an_independent_target_falls(L, torch, dev_book):
    """Book cover 160x90, seed 2, d = 50: the noisy frame is r = 16 at pass 0, the target r = 4096
    at pass 1 (independent samples). MSE(denoised, target) < MSE(noisy, target), with the default
    parameters. A condition, not a tuned number; the ratio is printed."""
    w, h = 160, 90
    noisy, g = book_frame(L, torch, dev_book, w, h, 16)
    target, _ = book_frame(L, torch, dev_book, w, h, 4096, pass_=1, aov=False)
    den = device_denoise(L, torch, noisy, g["albedo"], g["normal"], g["depth"])
    before, after = float(np.mean((noisy - target) ** 2)), float(np.mean((den - target) ** 2))
    print(f"MSE noisy {before:.6e} denoised {after:.6e} ratio {after / before:.4f}")
    assert np.isfinite(den).all() and after < before
