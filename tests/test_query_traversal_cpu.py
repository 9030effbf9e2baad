"""The one host decision "does this launch traverse the tree, or does every ray take the linear
scan" of the kernels that find their hits outside the megakernel (query_takes_tree,
tray_query_device.hpp), reached without a device through tray_debug_query_traversal. The traversal
stacks need stack_cap x 1 KiB of LDS per workgroup, stack_cap = tray_scene_info's stack_depth + 3,
and must fit into 64 KiB beside what the kernel holds there itself. The boundaries are pinned as the
launchers have them, so that tests/test_gpu_query_shapes.py can tell on which side of one a launch
ran; both sides give the same bits."""
import pytest

SLACK = 3  # kStackSlack (tray_kernel.hpp): stack_cap - stack_depth
# kind: the last stack_cap that takes the tree; the rule
LAST_TREE = {"plain": 64,      # stacks <= 64 KiB
             "pixels": 56,     # + 8 KiB of parked colours
             "temporal": 63}   # + 64 B of the record's reduction


def tree(L, kind, stack_cap):
    return L.query_traversal(kind, stack_cap - SLACK)


@pytest.mark.parametrize("kind", sorted(LAST_TREE))
def test_the_boundary_of_each_kind(L, kind):
    last = LAST_TREE[kind]
    assert tree(L, kind, last) is True
    assert tree(L, kind, last + 1) is False
    # one threshold per kind: the tree everywhere below it, the scan everywhere above
    assert all(tree(L, kind, cap) for cap in range(SLACK, last + 1))
    assert not any(tree(L, kind, cap) for cap in range(last + 1, 200))


def test_the_kinds_are_the_headers(L):
    import os
    import re

    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "tray_debug.h")).read()
    named = {n.lower(): int(v) for n, v in re.findall(r"#define TRAY_QUERY_KIND_(\w+) (\d+)", text)}
    assert named == L.QUERY_KINDS and set(named) == set(LAST_TREE)


def test_stack_depth_is_scene_infos(L):
    """The argument is tray_scene_info's stack_depth, three slots below the stacks' size: the book
    cover's shallow tree is far from every threshold."""
    assert all(L.query_traversal(kind, 0) for kind in LAST_TREE)
    assert L.query_traversal("plain", 61) and not L.query_traversal("plain", 62)


def test_bad_arguments(L):
    import ctypes

    out = ctypes.c_int32(7)
    lib = L.lib()
    assert lib.tray_debug_query_traversal(0, 10, None) == L.TRAY_ERR_INVALID_ARGUMENT
    for kind in (-1, 3):
        assert lib.tray_debug_query_traversal(kind, 10, ctypes.byref(out)) == L.TRAY_ERR_INVALID_ARGUMENT
    assert lib.tray_debug_query_traversal(0, -1, ctypes.byref(out)) == L.TRAY_ERR_INVALID_ARGUMENT
    assert out.value == 7  # untouched by a refused call
