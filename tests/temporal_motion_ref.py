"""include/tray_temporal_motion.h restated in numpy from the header's text (not from the kernel).
Everything the header takes over unchanged is tests/temporal_ref.py's and
tests/temporal_variance_ref.py's own code: their steps are run with the one function that holds
sections 2b and 2c (temporal_ref.project, which both reach through the module) replaced by the one
below, whose 2b is the new header's and whose 2c is the old one's again. The motion plane is added on
top. numpy's element-wise + - * / on float64 are the correctly rounded IEEE operations and never
contract into an FMA, so the expectation against the device is equality of bit patterns.

A geometry is (n, 4) float64 {cx, cy, cz, radius} in list order: tests/scene_update_cases.geometry.
"""
import contextlib

import numpy as np

import temporal_ref as T
import temporal_variance_ref as V

f8 = np.float64
MAX_HISTORY, DEPTH_TOLERANCE, SNAP = T.MAX_HISTORY, T.DEPTH_TOLERANCE, T.SNAP


def target(camera, width, height, index, t, geometry, prev_geometry):
    """Section 3b: (Q' (height, width, 3), valid for hits; moved: the hits whose sphere is not UNMOVED)."""
    cur = np.asarray(geometry, dtype=f8).reshape(-1, 4)
    prev = np.asarray(prev_geometry, dtype=f8).reshape(-1, 4)
    o, d = T.centre_rays(camera, width, height)
    hit = index >= 0
    with np.errstate(all="ignore"):
        Q = o + d * np.where(hit, t, 0.0)[..., None]
        if not len(cur):
            return Q, np.zeros_like(hit)
        i = np.where(hit, index, 0)
        c, R, cp, Rp = cur[i, 0:3], cur[i, 3], prev[i, 0:3], prev[i, 3]
        unmoved = (cp[..., 0] == c[..., 0]) & (cp[..., 1] == c[..., 1]) & (cp[..., 2] == c[..., 2]) & (Rp == R)
        m = (Q - c) / R[..., None]
        Qp = cp + m * Rp[..., None]
    moved = hit & ~unmoved
    return np.where(moved[..., None], Qp, Q), moved


def project(camera, prev_camera, width, height, index, t, geometry, prev_geometry):
    """Section 3b, then tray_temporal.h's 2c on its e: (z, u, v, in_range)."""
    o, d = T.centre_rays(camera, width, height)
    P, p00, pxv, pyv = T._cam(prev_camera)
    Qp, _ = target(camera, width, height, index, t, geometry, prev_geometry)
    with np.errstate(all="ignore"):
        hit = index >= 0
        e = np.where(hit[..., None], Qp - P, d)
        n = T.cross(pxv, pyv)
        c0 = p00 - P
        z = T.dot(n, e) / T.dot(n, c0)
        g = e / z[..., None] - c0
        u = T.dot(g, pxv) / T.dot(pxv, pxv)
        v = T.dot(g, pyv) / T.dot(pyv, pyv)
        in_range = (z > 0) & (u > -1) & (u < f8(width)) & (v > -1) & (v < f8(height))
    return z, u, v, in_range


@contextlib.contextmanager
def _following(geometry, prev_geometry):
    """temporal_ref.step and temporal_variance_ref.step with their projection following the spheres."""
    static = T.project

    def moving(camera, prev_camera, width, height, index, t):
        return project(camera, prev_camera, width, height, index, t, geometry, prev_geometry)

    T.project = moving
    try:
        yield
    finally:
        T.project = static


def motion_plane(camera, prev_camera, width, height, index, t, geometry, prev_geometry):
    """Section 4: (height, width, 2), (u - x, v - y) where in range, NaN elsewhere."""
    _, u, v, in_range = project(camera, prev_camera, width, height, index, t, geometry, prev_geometry)
    x = np.arange(width, dtype=f8)[None, :]
    y = np.arange(height, dtype=f8)[:, None]
    with np.errstate(all="ignore"):
        mv = np.stack([u - x, v - y], axis=-1)
    return np.where(in_range[..., None], mv, np.nan)


def step(camera, prev_camera, frame, hits, history, geometry, prev_geometry, m2, max_history=MAX_HISTORY,
         depth_tolerance=DEPTH_TOLERANCE, snap=SNAP):
    """One step. hits: (index, t) of `camera`'s centre rays in the scene of `geometry`; history: None or
    a state dict made when the scene held prev_geometry; m2: carry M2 (section 1). Returns (state dict,
    variance or None without m2, (fresh, age_sum), the motion plane or None where none is written)."""
    frame = np.asarray(frame, dtype=f8)
    height, width = frame.shape[:2]
    with _following(geometry, prev_geometry):
        if m2:
            state, variance, record = V.step(camera, prev_camera, frame, hits, history, max_history, depth_tolerance,
                                             snap)
        else:
            state, record = T.step(camera, prev_camera, frame, hits, history, max_history, depth_tolerance, snap)
            variance = None
    motion = None
    if history is not None and prev_camera is not None and max_history > 1 and frame.size:
        index = np.asarray(hits[0], dtype=np.int32)
        t = np.where(index >= 0, np.asarray(hits[1], dtype=f8), np.inf)
        motion = motion_plane(camera, prev_camera, width, height, index, t, geometry, prev_geometry)
    return state, variance, record, motion
