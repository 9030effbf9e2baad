"""include/tray_scene_update.h restated in numpy, from the header's text: the check of section 2 and
the boxes of section 3. Slow and plain on purpose; the device must agree with it byte for byte.

Nodes are tray_amd._lib.NODE_DTYPE records (tray_debug_scene_nodes): box[axis][0 low, 1 high][slot],
ref[slot] an inner node's index, 0x8000 | a leaf's index, or 0xFFFF for an unused slot. leaves[l] is
(first slot << 3) | count; bidx[slot] is the list index of the sphere in that slot."""
import numpy as np

LEAF_BIT, NONE = 0x8000, 0xFFFF
F32_INF = np.float32(np.inf)


def down(v):
    """The nearest float not above the double v."""
    v = np.float64(v)
    f = np.float32(v)
    return np.nextafter(f, -F32_INF) if np.float64(f) > v else f


def up(v):
    """The nearest float not below the double v."""
    v = np.float64(v)
    f = np.float32(v)
    return np.nextafter(f, F32_INF) if np.float64(f) < v else f


def sphere_box(sphere, pad):
    """(low[3], high[3]) of one padded sphere: two roundings in FP64, then outward to float."""
    c, r = np.asarray(sphere[:3], dtype=np.float64), np.abs(np.float64(sphere[3]))
    pad = np.float64(pad)
    lo = [down((c[a] - r) - pad) for a in range(3)]
    hi = [up((c[a] + r) + pad) for a in range(3)]
    return np.array(lo, dtype=np.float32), np.array(hi, dtype=np.float32)


def refit(nodes, leaves, bidx, geometry, bound):
    """The node array after an update with `geometry` ((n, 4): cx, cy, cz, radius) on a scene of bound
    M = `bound`: every used slot's box recomputed, leaves from their spheres, inner children as the
    union of that child's slots; unused slots, refs and pad as they were."""
    out = np.array(nodes, copy=True)
    geometry = np.asarray(geometry, dtype=np.float64)
    pad = np.float64(4e-6) * np.float64(bound)
    for node in range(len(out) - 1, -1, -1):  # a child's index exceeds its parent's: children first
        for slot in range(4):
            ref = int(out[node]["ref"][slot])
            if ref == NONE:
                continue
            if ref & LEAF_BIT:
                leaf = int(leaves[ref & (LEAF_BIT - 1)])
                first, count = leaf >> 3, leaf & 7
                lo, hi = np.full(3, F32_INF), np.full(3, -F32_INF)
                for s in range(first, first + count):
                    l, h = sphere_box(geometry[int(bidx[s])], pad)
                    lo, hi = np.minimum(lo, l), np.maximum(hi, h)
            else:
                assert ref > node
                lo = out[ref]["box"][:, 0, :].min(axis=1)
                hi = out[ref]["box"][:, 1, :].max(axis=1)
            out[node]["box"][:, 0, slot] = lo
            out[node]["box"][:, 1, slot] = hi
    return out


def check(geometry, bound):
    """(n_refused, first_refused, extent) of section 2 against M = `bound`. A scene without a tree
    refuses nothing: the caller takes (0, -1, extent) there."""
    g = np.asarray(geometry, dtype=np.float64).reshape(-1, 4)
    r = np.abs(g[:, 3:4])
    with np.errstate(invalid="ignore"):
        coords = np.abs(np.concatenate([g[:, :3] - r, g[:, :3] + r], axis=1))
        ok = (coords <= np.float64(bound)).all(axis=1)  # a NaN compares false
    bad = np.nonzero(~ok)[0]
    finite = coords[np.isfinite(coords)]
    extent = float(finite.max()) if finite.size else 0.0
    return int(bad.size), int(bad[0]) if bad.size else -1, extent
