"""The scenes and motions of tests/test_gpu_scene_update.py: shapes of tests/query_shapes.py, each
with the motions that apply to it. A motion maps the spheres A of a shape to spheres B of the same
count and materials; an update of the uploaded A with B's centres and radii must then give what a
fresh upload of B gives.

The book motions leave the ground alone and keep every coordinate inside its 2000 = M, the chain motion keeps the chain's extent along x, which sets its tight M,
so every one of them is applied, never refused. Each was run through the oracle on the CPU at the
tests' settings: between A and B at least 40 % of the frame's pixels and of the camera rays' hit
records differ (the tests assert it, so that an update that does nothing cannot pass)."""
import numpy as np

import query_shapes as Q

SHAPES = {s.name: s for s in Q.SHAPES}
BOOKS = ("leaf2", "leaf4", "dense")
CASES = [(name, motion) for name in BOOKS for motion in ("jitter", "perm", "lift")] + \
        [("dome", "dome"), ("chain16", "chain"), ("chain15", "chain"), ("chain600", "chain")]


def small_of(s):
    return np.nonzero(s["radius"] < 0.5)[0]


def jitter(s):
    """x, z += U(-0.3, 0.3), R *= U(0.8, 1.25), y = R: every small sphere slides and swells on the ground."""
    rng, b, m = np.random.default_rng(5), s.copy(), small_of(s)
    b["center"][m, 0] += rng.uniform(-0.3, 0.3, len(m))
    b["center"][m, 2] += rng.uniform(-0.3, 0.3, len(m))
    b["radius"][m] *= rng.uniform(0.8, 1.25, len(m))
    b["center"][m, 1] = b["radius"][m]
    return b


def perm(s):
    """The centres of all spheres but the ground permuted among themselves: neighbours in the tree end
    up far apart, so the inner boxes grow to most of the scene and a stale one shows. (Among the small
    spheres alone the oracle finds 57 % of the pixels but only 31 % of the camera rays' hit records
    changed, the three large spheres included 73 % and 53 %; 78 % and 57 % on the 1,939-sphere scene.)"""
    rng, b, m = np.random.default_rng(5), s.copy(), np.nonzero(s["radius"] < 100.0)[0]
    b["center"][m] = s["center"][rng.permutation(m)]
    return b


def lift(s):
    """y += U(0, 3)."""
    rng, b, m = np.random.default_rng(5), s.copy(), small_of(s)
    b["center"][m, 1] += rng.uniform(0.0, 3.0, len(m))
    return b


def dome(s):
    """lift, and both out-of-tree spheres change: the dome shrinks from 5000 to 4000 and the ground
    from 1000 to 999.5 about their centres."""
    b = lift(s)
    assert b["radius"][-1] == 5000.0 and b["radius"][0] == 1000.0
    b["radius"][-1], b["radius"][0] = 4000.0, 999.5
    return b


def chain(s):
    """y = 0.3 cos i, z = 0.2 sin 2i: the chain winds about its axis; x and the radii, hence M, stay."""
    b, i = s.copy(), np.arange(len(s), dtype=np.float64)
    b["center"][:, 1] = 0.3 * np.cos(i)
    b["center"][:, 2] = 0.2 * np.sin(2.0 * i)
    return b


MOTIONS = dict(jitter=jitter, perm=perm, lift=lift, dome=dome, chain=chain)


def geometry(spheres):
    """(n, 4) float64 {cx, cy, cz, radius}: what tray_scene_update takes."""
    return np.ascontiguousarray(np.concatenate([spheres["center"], spheres["radius"][:, None]], axis=1),
                                dtype=np.float64)


def fraction_differing(a, b):
    """Of two (n, k) float64 arrays: the fraction of rows whose bits differ."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(len(a), -1).view(np.uint64)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(len(b), -1).view(np.uint64)
    return float((a != b).any(axis=1).mean())


def hits_differing(a, b):
    """Of two HIT_DTYPE arrays: the fraction of records that differ in any byte."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return float((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1).mean())
