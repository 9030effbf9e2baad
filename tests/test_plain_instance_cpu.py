"""The host predicate that sends a launch through the megakernel's plain-frame instance
(tray_kernel.hip `plain_frame_launch`), reached without a device through
tray_debug_plain_instance, which fills the kernel parameters on the host and asks the predicate
launch_render asks. The plain instance has every option of `PlainFrame` compiled in, so the
predicate must hold only when all of them do: each option is checked on both sides."""
import pytest

# The launch the product runs frame after frame (C2): every option as PlainFrame fixes it.
PLAIN = dict(facts=("bvh", "candidates", "work_order"), rays_per_pixel=64, tile_rows=0, n_global=1, n_nodes=130,
             leaf_max=1, acc=1, lds_mode=1)


def ask(L, **kw):
    a = dict(PLAIN)
    a.update(kw)
    return L.plain_instance(**a)


def test_the_plain_launch_qualifies(L):
    assert ask(L) is True
    assert ask(L, lds_mode=2) is True  # nodes and leaf table in LDS
    assert ask(L, rays_per_pixel=256, n_nodes=1) is True  # any r with one sum per chunk, a tree of one node
    assert ask(L, tile_rows=-1) is True  # tray_params rejects it; the kernel reads <= 0 as contiguous


@pytest.mark.parametrize("add", ["stats", "progress", "stack_spill", "segments", "counting"])
def test_a_fact_that_must_be_absent(L, add):
    assert ask(L, facts=PLAIN["facts"] + (add,)) is False


@pytest.mark.parametrize("drop", ["bvh", "candidates", "work_order"])
def test_a_fact_that_must_be_present(L, drop):
    assert ask(L, facts=tuple(f for f in PLAIN["facts"] if f != drop)) is False


@pytest.mark.parametrize("kw", [dict(rays_per_pixel=1), dict(tile_rows=1), dict(tile_rows=8), dict(n_global=0),
                                dict(n_global=2), dict(n_nodes=0), dict(leaf_max=2), dict(leaf_max=4), dict(acc=0),
                                dict(acc=2), dict(lds_mode=0)])
def test_a_value_on_the_other_side(L, kw):
    assert ask(L, **kw) is False


def test_the_knob_forces_the_generic_instance(L, knobs):
    knobs(plain_instance=0)
    assert ask(L) is False
    knobs(plain_instance=1)
    assert ask(L) is True
    L.clear_debug_knobs()
    assert ask(L) is True


def test_every_option_has_a_case_here(L):
    """PlainFrame's options (tray_device.hpp) against the cases above, so a new option gets a case."""
    import os
    import re

    from conftest import ROOT

    text = open(os.path.join(ROOT, "tray_amd", "csrc", "tray_device.hpp")).read()
    body = re.search(r"struct LaunchAsk \{(.*?)\n\};", text, re.S).group(1)
    options = set(re.findall(r"static constexpr bool (k\w+) = false;", body))
    covered = {"kNoSegments": "segments", "kNoCount": "counting", "kCand": "candidates", "kMultiSample": "rays_per_pixel",
               "kContigRows": "tile_rows", "kOrdered": "work_order", "kOneGlobal": "n_global", "kHasNodes": "n_nodes",
               "kSingleLeaf": "leaf_max"}
    assert options == set(covered)
    assert set(L.PLAIN_FACTS) >= {v for v in covered.values() if v in ("segments", "counting", "candidates",
                                                                        "work_order")}
