"""TEST INFRASTRUCTURE ONLY: vectorised numpy restatement of the reference's
training-target generators (hcat/train/train_utils.py), the parity oracle of
hcunet_amd.train_utils.  Pinned bitwise against the reference's own outputs by
tests/golden/targets.npz (tests/golden/make_targets_golden.py).

  makePWL                :9-93     ring scan per background voxel
  colormask_to_mask      :175-187
  CalculateCenterOfMass  :190-237
  VectorToCenter         :240-274
"""
import numpy as np

RADII = 9


def offsets_full():
    """The 9 x 63 probe offsets (dx, dy) in the reference's order (:70-74), and
    the first row of each radius."""
    angles = np.linspace(0, 2 * np.pi, 63)
    off = [(int(np.rint(l * np.cos(theta))), int(np.rint(l * np.sin(theta))))
           for l in np.arange(1, 10) for theta in angles]
    return np.array(off, dtype=np.int64), np.arange(0, 10) * 63


def value(l0, l1):
    """:91 for integer radii arrays; 0 where l1 == 0 (fewer than two cells met)."""
    l0, l1 = np.asarray(l0, dtype=np.int64), np.asarray(l1, dtype=np.int64)
    v = 11 * np.exp(-1 * ((l0 + l1) ** 2) / (2 * (5 ** 2)))
    return np.where(l1 > 0, v, 0.0)


def keys_of(labels):
    """One integer per voxel, ordered as np.unique(axis=0) orders the colours."""
    a = np.asarray(labels).astype(np.int64)
    if a.ndim == 3:
        return a
    return (a[..., 0] << 32) | (a[..., 1] << 16) | a[..., 2]


def ring_scan(padded, Y, X, offsets, ring_begin):
    """(l0, l1) int64 [N,Y,X] of every voxel of the inner [Y,X] window of
    `padded` [N, Y + 18, X + 18] integer keys (0 = background), scanned as
    find_closest (:70-93) does: radii in order, offsets in order, the first
    non-zero key is `closest`, the first later key that is neither 0 nor
    `closest` ends the scan."""
    N = padded.shape[0]
    closest = np.zeros((N, Y, X), dtype=np.int64)
    l0 = np.zeros((N, Y, X), dtype=np.int64)
    l1 = np.zeros((N, Y, X), dtype=np.int64)
    for l in range(1, RADII + 1):
        for k in range(int(ring_begin[l - 1]), int(ring_begin[l])):
            dx, dy = int(offsets[k][0]), int(offsets[k][1])
            p = padded[:, RADII + dy:RADII + dy + Y, RADII + dx:RADII + dx + X]
            hit = (p != 0) & (l1 == 0)
            first = hit & (closest == 0)
            second = hit & (closest != 0) & (p != closest)
            closest = np.where(first, p, closest)
            l0 = np.where(first, l, l0)
            l1 = np.where(second, l, l1)
    return l0, l1


def make_pwl(labels, offsets=None, ring_begin=None):
    """makePWL()(labels): float64 [Z,Y,X]."""
    if offsets is None:
        offsets, ring_begin = offsets_full()
    k = keys_of(labels)
    Z, Y, X = k.shape
    padded = np.zeros((Z, Y + 2 * RADII, X + 2 * RADII), dtype=np.int64)   # the reference pads by 50: zeros either way
    padded[:, RADII:RADII + Y, RADII:RADII + X] = k
    l0, l1 = ring_scan(padded, Y, X, offsets, ring_begin)
    return np.where(k != 0, 0.0, value(l0, l1))


def colormask_to_mask(colormask):
    """In place; returns uint8 [Z,Y,X]."""
    colormask[(colormask != 0).any(axis=-1)] = 1
    return (colormask[:, :, :, 0] * 255).astype(np.uint8)


def center_of_mass(labels):
    """CalculateCenterOfMass()(labels): (center_of_mass float64, new_image uint32)."""
    a = np.asarray(labels)
    if a.ndim == 3:
        a = np.stack((a, a, a), axis=3)
    a = a.copy()
    a[(a == a[0, 0, 0].copy()).all(axis=-1)] = 0
    _, inverse = np.unique(a.reshape(-1, 3), axis=0, return_inverse=True)
    ids = inverse.reshape(a.shape[:3]).astype(np.uint32)
    com = np.zeros(ids.shape, dtype=np.float64)
    for i in range(int(ids.max()) + 1):
        zyx = np.nonzero(ids == i)
        z, y, x = (int(np.round(np.sum(c.astype(np.float64)) / len(c))) for c in zyx)
        com[z, y, x] = i
    return com, ids


def vector_to_center(center, colormask):
    """VectorToCenter()(center, colormask, None): float64 [Z,Y,X,3]; ValueError
    where an id has no or several centre voxels."""
    vec = np.zeros(colormask.shape + (3,), dtype=np.float64)
    for i in np.unique(colormask):
        if i == 0:
            continue
        com = np.argwhere(center == i)
        if len(com) != 1:
            raise ValueError(f'id {i} has {len(com)} centre voxels')
        where = np.nonzero(colormask == i)
        for d in range(3):
            vec[where + (d,)] = where[d] - com[0, d]
    for d in range(3):
        vec[..., d] /= vec.shape[d]
    return vec
