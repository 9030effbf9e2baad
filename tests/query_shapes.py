"""The shape matrix of tests/test_gpu_query_shapes.py: the scenes on which every kernel that finds its
hits through query_hit / query_occluded (tray_query_device.hpp) is run, with the knobs to set before
the upload and the tray_scene_info facts the upload must then report. The facts are asserted, so a
change of the BVH builder cannot move a case off the boundary it stands for without a test saying so.

What varies: spheres per leaf (1, 2, 4), out-of-tree spheres (0, 1, 2), no tree at all, the smallest
tree, and the depth of the traversal stack on both sides of each of the three thresholds at which a
launch gives up the tree for the linear scan (tests/test_query_traversal_cpu.py pins them).

The deep stacks come from a chain of spheres shrinking geometrically along a line towards a limit
point (the SAH peels them off one by one): sphere i has centre (sum of q^j for j <= i, 0.3 sin i, 0)
and radius 0.45 q^i, q = 0.8. q^i is built by repeated multiplication and the sum by repeated
addition, one rounding each, so the scene has the same bits wherever it is built. The radii stay
normal numbers; R * R underflows to 0 at the far end of the longer chains, which is legitimate input
for the oracle and the device alike. The stack sizes below are tray_bvh.cpp's for these chains with
one sphere per leaf (a stand-alone host build of it printed them).
"""
import math

import numpy as np

from conftest import RICH_SETUP

W, H = 40, 24  # every frame of the matrix
SLACK = 3      # kStackSlack: the stacks hold tray_scene_info's stack_depth + 3 slots
KINDS = ("plain", "pixels", "temporal")  # tray_amd._lib.QUERY_KINDS
ALL_TREE = dict(plain=True, pixels=True, temporal=True)
Q = 0.8
LIMIT = 1.0 / (1.0 - Q)  # the chain's limit point (5, 0, 0); its bound M is one ulp above 5
# The chains' camera: inside [-M, M]^3, beside the thick end, looking along the chain at its limit
# point, aperture 0.05. The chain is self-similar about that point (sphere i lies 4 q^i from it with
# radius 0.45 q^i), so from anywhere about a dozen spheres are wider than a pixel; this place was
# chosen with the oracle on the CPU so that 36 % of the 40 x 24 camera rays hit one (15 spheres in
# all with the secondary rays), and the orbit and dolly steps of the temporal cases stay inside.
CHAIN_SETUP = np.array([0.2, 0.5, 0.8, LIMIT, 0, 0, 0, 1, 0, 24.0, 4.9, 4.9, 0.05])


def chain(n):
    from oracle.oracle import SPHERE_DTYPE

    s = np.zeros(n, dtype=SPHERE_DTYPE)
    p, x = 1.0, 0.0
    for i in range(n):
        x = x + p
        s[i]["center"] = (x, 0.3 * math.sin(float(i)), 0.0)
        s[i]["radius"] = 0.45 * p
        p = p * Q
    s["material"] = 1 + np.arange(n) % 3  # the three kinds in turn
    s["albedo"] = 0.7
    s["param"] = np.where(s["material"] == 3, 1.5, 0.2)  # refraction index 1.5, fuzz 0.2
    return s


def book_with_duplicates(O):
    """The book cover with its first 40 small spheres appended again (test_hit_ties_report_the_lower_index):
    equal roots inside a leaf and across leaves; the earlier sphere must win every one."""
    book = O.rich_scene(2)
    small = np.nonzero(book["radius"] < 0.5)[0][:40]
    assert len(small) == 40
    return np.concatenate([book, book[small]])


def book_under_a_dome(O):
    """test_bvh_global_spheres's scene: the ground, listed first, and an enclosing dome the camera sits
    inside, listed last, both kept out of the tree."""
    from oracle.oracle import SPHERE_DTYPE

    base = O.rich_scene(3)
    s = np.zeros(len(base) + 1, dtype=SPHERE_DTYPE)
    s[:len(base)] = base
    s[-1]["center"], s[-1]["radius"], s[-1]["material"] = (0, 0, 0), 5000.0, 1
    s[-1]["albedo"] = (0.9, 0.8, 0.7)
    return s


class Shape:
    def __init__(self, name, build, setup, knobs=None, has_bvh=1, leaf_max=None, packed=False, globals_=(),
                 bound=None, stack_cap=None, tree=None, originals=None):
        self.name, self.build, self.setup, self.knobs = name, build, setup, dict(knobs or {})
        self.has_bvh = has_bvh
        self.leaf_max = leaf_max      # tray_scene_info's leaf_max
        self.packed = packed          # n_leaves < n_spheres - n_global: some leaf holds several spheres
        self.globals_ = globals_      # the out-of-tree spheres' list indices (negative: from the end)
        self.bound = bound            # tray_scene_info's bound, where the case depends on it
        self.stack_cap = stack_cap    # stack_depth + SLACK, where the case stands on a threshold
        self.tree = tree              # per kind: does the launch traverse the tree? None without one
        self.originals = originals    # the spheres listed before the duplicates, where there are any

    def __repr__(self):
        return self.name


def _chain_shape(n, stack_cap, **tree):
    return Shape(f"chain{n}", lambda O: chain(n), CHAIN_SETUP, knobs=dict(bvh_leaf=1), leaf_max=1, stack_cap=stack_cap,
                 tree=tree)


SHAPES = [
    Shape("leaf2", book_with_duplicates, RICH_SETUP, knobs=dict(bvh_leaf=2), leaf_max=2, packed=True, globals_=(0,),
          tree=ALL_TREE, originals=486),
    Shape("leaf4", book_with_duplicates, RICH_SETUP, knobs=dict(bvh_leaf=4), leaf_max=4, packed=True, globals_=(0,),
          tree=ALL_TREE, originals=486),
    # 1,939 spheres, no knob: the library's own choice is 2-sphere leaves (test_bvh_lds_layouts)
    Shape("dense", lambda O: O.rich_scene(7, 22), RICH_SETUP, leaf_max=2, packed=True, globals_=(0,), tree=ALL_TREE),
    Shape("dome", book_under_a_dome, RICH_SETUP, leaf_max=1, globals_=(0, -1), bound=5000.0, tree=ALL_TREE),
    # the smallest tree (one or two levels of nodes: empty child slots) and one sphere fewer: none
    _chain_shape(16, 14, **ALL_TREE),
    Shape("chain15", lambda O: chain(15), CHAIN_SETUP, knobs=dict(bvh_leaf=1), has_bvh=0),
    _chain_shape(600, 55, plain=True, pixels=True, temporal=True),     # the deepest every kind traverses
    _chain_shape(1000, 58, plain=True, pixels=False, temporal=True),   # the pixel list alone scans
    _chain_shape(1500, 63, plain=True, pixels=False, temporal=True),   # the temporal step's last tree value
    _chain_shape(2000, 64, plain=True, pixels=False, temporal=False),  # exactly 64 KiB of stacks
    _chain_shape(2500, 65, plain=False, pixels=False, temporal=False),  # everything scans
]


def upload(L, shape, spheres, bg):
    """tray_scene_upload under the shape's knobs (they apply at the upload only), with the facts the
    shape stands for asserted on tray_scene_info and on the library's own tree-or-scan decision.
    Returns the DeviceScene; the caller releases it."""
    with L.debug_knobs(**shape.knobs):
        dev = L.DeviceScene(spheres, bg, 0)
    try:
        check_facts(L, shape, dev.info(), len(spheres))
    except BaseException:
        dev.release()
        raise
    return dev


def check_facts(L, shape, info, n):
    what = f"{shape.name}: {facts(info)}"
    assert info.n_spheres == n and info.has_bvh == shape.has_bvh, what
    if not shape.has_bvh:
        return
    assert info.leaf_max == shape.leaf_max, what
    assert info.n_global == len(shape.globals_), what
    assert (info.n_leaves < n - info.n_global) == shape.packed, what
    if shape.bound is not None:
        assert info.bound == shape.bound, what
    if shape.stack_cap is not None:
        assert info.stack_depth + SLACK == shape.stack_cap, what
    assert traversal(L, info) == shape.tree, what


def traversal(L, info):
    """Per kind: whether a launch on this scene traverses its tree (tray_debug_query_traversal)."""
    return {kind: L.query_traversal(kind, info.stack_depth) for kind in KINDS}


def facts(info):
    return {k: getattr(info, k) for k in ("n_spheres", "has_bvh", "leaf_max", "n_nodes", "n_leaves", "stack_depth",
                                          "n_global", "bound")}


def out_of_tree(shape, n):
    return np.array([g % n for g in shape.globals_], dtype=np.int64)


def assert_live(shape, n, bound, origins, index, what):
    """The conditions under which a case does exercise the traversal, from the host's side: at least
    90 % of its rays start inside [-bound, bound]^3 (any other ray takes the per-ray scan), and at
    least 25 % of them hit a sphere of the tree (`index`: the oracle's)."""
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    index = np.asarray(index).reshape(-1)
    if shape.has_bvh:
        inside = (np.abs(origins) <= bound).all(axis=1).mean()
        assert inside >= 0.9, f"{shape.name} {what}: {inside:.3f} of the rays start inside the bound"
    in_tree = ((index >= 0) & ~np.isin(index, out_of_tree(shape, n))).mean()
    assert in_tree >= 0.25, f"{shape.name} {what}: {in_tree:.3f} of the rays hit a sphere of the tree"
