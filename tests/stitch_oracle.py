"""numpy restatement of the tiled stitch (hcunet_amd/instances.py:
windows, stitch_vec_to_cell; hcunet_amd/segment.py: predict_instance_mask),
built on tests/vec_to_cell_oracle.py.  Test infrastructure: the reference has
no such function, so the rule is pinned here.

For each window, x slowest and z fastest: stages 1-4 of pixel_vec_to_cell on
the window's crop in window-local coordinates; a peak is owned iff lo + peak
lies in the window's core; owned peaks take consecutive stack-wide ids from 1,
the others 0; a voxel is written at lo + (x, y, z) with its winner's id iff a
peak won, the mask does not read below 0.2, the id is not 0 and floor(c) keeps
one voxel off every face of the window that is not a face of the volume."""
import numpy as np

from tests import vec_to_cell_oracle as vo


def windows(shape, tile, halo):
    if any(t is not None and t <= 0 for t in tile) or any(h < 0 for h in halo):
        raise ValueError('tile sizes are positive and halos are not negative')
    per_axis = []
    for n, t, h in zip(shape, tile, halo):
        t = n if t is None else t
        cores = [(k * t, min((k + 1) * t, n)) for k in range(-(-n // t))]
        per_axis.append([(a, b, max(a - h, 0), min(b + h, n)) for a, b in cores])
    out = []
    for x in per_axis[0]:
        for y in per_axis[1]:
            for z in per_axis[2]:
                out.append(dict(core_lo=(x[0], y[0], z[0]), core_hi=(x[1], y[1], z[1]),
                                lo=(x[2], y[2], z[2]), hi=(x[3], y[3], z[3])))
    return out


def vote_bounds(window, shape):
    """float32 [3,2]: floor(c) of a written voxel lies in [lo, hi) per axis."""
    b = np.empty((3, 2), dtype=np.float32)
    for a in range(3):
        w = window['hi'][a] - window['lo'][a]
        b[a, 0] = 1 if window['lo'][a] != 0 else -np.inf
        b[a, 1] = w - 1 if window['hi'][a] != shape[a] else np.inf
    return b


def winners(c, peaks):
    """int64 [X,Y,Z]: the index of the peak stage 5 gives each vote, -1 where none wins."""
    shape = c.shape[1:]
    idx = np.full(shape, -1, dtype=np.int64)
    nearest = np.full(shape, vo.FARTHEST, dtype=np.float32)
    for i, p in enumerate(np.asarray(peaks).reshape(-1, 3)):
        with np.errstate(invalid='ignore', over='ignore'):
            d0, d1, d2 = (c[a] - np.float32(p[a]) for a in range(3))
            d = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
            won = nearest > d
        idx[won] = i
        nearest[won] = d[won]
    return idx


def paste(dst, vector, mask, peaks, ids, lo, bounds):
    """Write one window into dst (int32 [X,Y,Z], in place).  vector: the
    window's float32 [3,x,y,z]; mask: the window's, or None; peaks int [n,3]
    window-local; ids int [n]; lo: the window's origin; bounds as
    vote_bounds().  Returns the number of voxels that only rule (d) refused."""
    c = vo.centres(np.ascontiguousarray(vector, dtype=np.float32))
    idx = winners(c, peaks)
    ids = np.asarray(ids, dtype=np.int32).reshape(-1)
    wid = np.where(idx >= 0, ids[np.maximum(idx, 0)] if len(ids) else 0, 0).astype(np.int32)
    keep = (idx >= 0) & (wid != 0)
    if mask is not None:
        keep &= ~(np.asarray(mask).astype(np.float32) < np.float32(0.2))
    inside = np.ones(keep.shape, dtype=bool)
    with np.errstate(invalid='ignore'):
        f = np.floor(c)
        for a in range(3):
            inside &= (f[a] >= bounds[a, 0]) & (f[a] < bounds[a, 1])
    view = dst[tuple(slice(o, o + s) for o, s in zip(lo, keep.shape))]
    assert view.shape == keep.shape
    view[keep & inside] = wid[keep & inside]
    return int((keep & ~inside).sum())


def stitch(shape, tile, halo, crop, sigma=5, num_peaks=100):
    """crop(window) -> (vector float32 [3,x,y,z], mask [x,y,z]) of that
    window.  Returns dict(label int32 [X,Y,Z], centres int64 [n,3], owned: the
    number of ids each window gave out, refused: voxels only rule (d)
    refused, windows)."""
    label = np.zeros(shape, dtype=np.int32)
    centres, owned, refused = [], [], 0
    wins = windows(shape, tile, halo)
    for w in wins:
        vector, mask = crop(w)
        vector = np.ascontiguousarray(vector, dtype=np.float32)
        assert vector.shape[1:] == tuple(b - a for a, b in zip(w['lo'], w['hi']))
        peaks = vo.pixel_vec_to_cell(vector, None, num_peaks=num_peaks, sigma=sigma)['peaks'].reshape(-1, 3)
        pos = peaks + np.asarray(w['lo'])
        own = np.all((pos >= np.asarray(w['core_lo'])) & (pos < np.asarray(w['core_hi'])), axis=1)
        ids = np.zeros(len(peaks), dtype=np.int32)
        first = sum(owned) + 1
        ids[own] = np.arange(first, first + int(own.sum()))
        refused += paste(label, vector, mask, peaks, ids, w['lo'], vote_bounds(w, shape))
        centres.append(pos[own].astype(np.int64).reshape(-1, 3))
        owned.append(int(own.sum()))
    return dict(label=label, centres=np.concatenate(centres).reshape(-1, 3), owned=owned, refused=refused,
                windows=wins)


def box(w):
    return tuple(slice(a, b) for a, b in zip(w['lo'], w['hi']))


def stitch_field(vector, mask, tile, halo, sigma=5, num_peaks=100):
    """stitch() of whole-volume arrays: vector [1,3,X,Y,Z] or [3,X,Y,Z] float32, mask [X,Y,Z] or [1,1,X,Y,Z]."""
    v = np.asarray(vector)
    v = v[0] if v.ndim == 5 else v
    m = np.asarray(mask)
    m = m[0, 0] if m.ndim == 5 else m
    return stitch(v.shape[1:], tile, halo, lambda w: (v[(slice(None),) + box(w)], m[box(w)]), sigma, num_peaks)


def field(shape, centres, seed, noise=0.6):
    """fp16 [1,3,X,Y,Z]: every voxel points at its nearest centre, plus
    N(0, noise); noise=0: exactly at the integer centre."""
    grid = np.indices(shape).astype(np.float64)
    cen = np.asarray(centres, dtype=np.float64)
    d = ((grid[None] - cen[:, :, None, None, None]) ** 2).sum(1)
    v = (np.moveaxis(cen[np.argmin(d, axis=0)], -1, 0) - grid)[::-1]
    if noise:
        v = v + np.random.default_rng(seed).normal(0, noise, size=(3,) + tuple(shape))
    return v.astype(np.float32).astype(np.float16)[None]


def same_partition(a, b):
    """True iff the label volumes a and b are equal under a bijection of
    their non-zero ids (background on background)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = np.unique(np.stack([a, b]), axis=1)
    return (len(np.unique(pairs[0])) == pairs.shape[1] and len(np.unique(pairs[1])) == pairs.shape[1]
            and all((p == 0) == (q == 0) for p, q in pairs.T))
