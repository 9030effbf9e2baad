"""The plain-frame instance's schedule: its leaf, shade and refill phases run by one
cost rule (`phase_fires`, tray_kernel.hpp) instead of three fixed lane counts. That only reorders when
lanes are served: the chunk sums are order-free and a path's decisions are its own, so the frames
must equal, bit for bit, those of the generic instance, which keeps the fixed counts (the
"plain_instance" knob at 0 forces it in the same process), and pass 0 the oracle's within the suite's bar (L-inf <= 1e-4, Scene.Hit counts
equal). The plain instance has no segment buffer (asking for one is what makes a launch generic), so
the counts are those of the generic launch whose colours the plain one repeats bit for bit.

The rule itself is checked on the host over every (waiting, traversing) pair of a wave."""
import ctypes

import numpy as np
import pytest

from conftest import DEFAULT_BG, RICH_SETUP
from test_gpu_begin_step import oracle
from test_gpu_parity import TOL, bg_struct, camera, check
from test_gpu_plain_instance import forced_generic, two_launches

gpu = pytest.mark.gpu

DEPTH, SPP, RADIUS, SEED = 12, 64, 0.5, 2


def book_cover(O):
    sc = O.rich_scene(2)
    sc.setflags(write=False)
    return sc


def old_and_new(L, O, knobs, key, sc, w, h, spp, depth, passes, plain=True):
    """Renders (w, h) through the generic instance (fixed counts) and through whatever the library
    picks; checks the bits, pass 0 against the oracle, and the generic launch's Scene.Hit counts."""
    p = L.make_params(w, h, depth, spp, RADIUS, SEED, output=L.OUT_RGB_F64)
    old, _ = forced_generic(L, knobs, sc, p, passes, False, w, h)
    new, _, took = two_launches(L, sc, p, passes, False, w, h)
    assert took == ([0, 1] if plain else [0, 0])  # the counting launch, then the one with its work order
    for f in (old[1], new[0], new[1]):
        assert f.shape == (passes, h, w, 3) and np.array_equal(f, old[0])
    st = camera(L, RICH_SETUP, w, h)
    ref, rseg = oracle(O, key, sc, st, w, h, spp, depth, RADIUS, SEED)
    err = float(np.max(np.abs(new[1][0] - ref)))
    assert err <= TOL, err
    _, seg = L.render(sc, bg_struct(L, DEFAULT_BG), st, p, 0, segments=True)
    assert np.array_equal(seg, rseg)


@gpu
@pytest.mark.parametrize("passes", [1, 3])
def test_new_schedule_equals_old_and_oracle(L, O, knobs, passes):
    old_and_new(L, O, knobs, "triggers_cover", book_cover(O), 64, 36, SPP, DEPTH, passes)


@gpu
@pytest.mark.parametrize("passes", [1, 3])
def test_less_than_a_wave_per_chunk_pair(L, O, knobs, passes):
    """8 x 8, r = 64: 64 chunks for 16 workgroups' waves, so a wave holds at most a chunk or two and
    mostly runs its phases because nothing else is in flight (the drain, the last refills)."""
    old_and_new(L, O, knobs, "triggers_cover", book_cover(O), 8, 8, SPP, DEPTH, passes)


def glass_scene(L, n_glass):
    """The ground and n_glass Dielectric spheres in the camera's view."""
    sc = np.zeros(1 + n_glass, dtype=L.SPHERE_DTYPE)
    sc["center"][0], sc["radius"][0] = (0.0, -1000.0, 0.0), 1000.0
    sc["albedo"][0], sc["material"][0] = (0.5, 0.5, 0.5), L.LAMBERTIAN
    for k in range(n_glass):
        sc["center"][1 + k] = (0.0, 1.0, 0.0) if n_glass == 1 else (1.5 * (k % 4) - 2.0, 0.6, 1.5 * (k // 4) - 2.0)
        sc["radius"][1 + k] = 1.0 if n_glass == 1 else 0.6
        sc["albedo"][1 + k], sc["param"][1 + k], sc["material"][1 + k] = (1.0, 1.0, 1.0), 1.5, L.DIELECTRIC
    return sc


@gpu
def test_ground_and_one_dielectric_sphere(L, O, knobs):
    """Interior rays and deep paths in every wave (depth 50); it must terminate and equal the
    oracle. Two spheres are below the tree's minimum, so this frame takes the linear scan."""
    sc = glass_scene(L, 1)
    w, h = 32, 18
    st = camera(L, RICH_SETUP, w, h)
    p = L.make_params(w, h, 50, SPP, RADIUS, SEED)
    rgb, seg = L.render(sc, bg_struct(L, DEFAULT_BG), st, p, 0, segments=True)
    check(rgb, seg, *oracle(O, "one_glass", sc, st, w, h, SPP, 50, RADIUS, SEED))
    old_and_new(L, O, knobs, "one_glass", sc, w, h, SPP, 50, 1, plain=False)


@gpu
def test_ground_and_sixteen_dielectric_spheres(L, O, knobs):
    """The same through the tree and the plain instance: 16 glass spheres, every path deep, few
    lanes traversing at a time."""
    sc = glass_scene(L, 16)
    dev = L.DeviceScene(sc, bg_struct(L, DEFAULT_BG), 0)
    info = dev.info()
    dev.release()
    assert info.has_bvh == 1 and info.n_global == 1 and info.leaf_max == 1
    old_and_new(L, O, knobs, "glass16", sc, 32, 18, SPP, 50, 1)


@gpu
def test_r16_instance_keeps_its_constants(L, O, knobs):
    """r = 16 runs a generic instance (sums per pixel-pass): the fixed counts, the oracle's frame."""
    old_and_new(L, O, knobs, "triggers_cover", book_cover(O), 32, 18, 16, DEPTH, 1, plain=False)


def test_trigger_rule_on_the_host(L):
    """phase_fires over every (waiting, traversing) pair: never for no lane, always when nothing
    else is in flight, monotone in both arguments."""
    for phase in L.TRIGGER_PHASES:
        fires = np.array([[L.phase_trigger(phase, w, t) for t in range(65)] for w in range(65)])
        assert not fires[0].any()          # nothing waits: no pass
        assert fires[1:, 0].all()          # nothing traverses: any waiting lane runs the pass
        assert (fires[1:] >= fires[:-1]).all()        # more waiting lanes never stop a pass
        assert (fires[:, 1:] <= fires[:, :-1]).all()  # more traversing lanes never start one
        assert not fires[1:, 1:].all() and fires[1:, 1:].any()  # and it is a batch rule, not a constant
    for bad in ((3, 1, 1), (-1, 1, 1), (0, 65, 0), (0, 0, 65)):
        out = ctypes.c_int32(0)
        assert L.lib().tray_debug_phase_trigger(*bad, ctypes.byref(out)) == L.TRAY_ERR_INVALID_ARGUMENT
