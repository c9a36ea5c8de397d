"""numpy restatement of the reference's pixel_vec_to_cell and hist3d
(hcat/segment.py:563-658), stage by stage, as hcunet_amd/instances.py states
them.  Test infrastructure: the device kernels are held to this text, and this
text to the reference's recorded outputs (tests/golden/vec_to_cell.npz) and,
where scipy imports, to scipy.ndimage.gaussian_filter.

Volumes are [X,Y,Z]; `vector` is [3,X,Y,Z] float32 (16-bit fields are widened
by the caller, exactly)."""
import numpy as np

FARTHEST = np.float32(100000)


def centres(vector):
    """float32 [3,X,Y,Z]: c = (x + v2, y + v1, z + v0) (:590-593)."""
    v = np.asarray(vector)
    assert v.dtype == np.float32 and v.ndim == 4 and v.shape[0] == 3
    grid = np.indices(v.shape[1:]).astype(np.float32)
    return np.stack([grid[0] + v[2], grid[1] + v[1], grid[2] + v[0]])


def vote_counts(c):
    """int64 [X,Y,Z]: votes per voxel (:640-656); a vote whose floor lies
    outside the volume, or is not finite, is dropped."""
    shape = c.shape[1:]
    with np.errstate(invalid='ignore'):
        f = np.floor(c)
        ok = np.ones(shape, dtype=bool)
        for a in range(3):
            ok &= (f[a] >= 0) & (f[a] < shape[a])       # False for NaN, +-Inf
    idx = [f[a][ok].astype(np.int64) for a in range(3)]
    lin = (idx[0] * shape[1] + idx[1]) * shape[2] + idx[2]
    return np.bincount(lin, minlength=int(np.prod(shape))).reshape(shape)


def normalise(counts):
    """float64: (1 + count) / (1 + max count) (:640, :658)."""
    counts = np.asarray(counts)
    return (1.0 + counts.astype(np.float64)) / (1.0 + np.float64(counts.max()))


def hist3d(c):
    return normalise(vote_counts(c))


def max_filter2(a):
    """scipy.ndimage.maximum_filter(a, size=2, mode='constant'): the maximum
    over the offsets {-1,0}^3, 0 outside."""
    p = np.pad(a, ((1, 0), (1, 0), (1, 0)), mode='constant')
    X, Y, Z = a.shape
    out = np.zeros_like(a)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                out = np.maximum(out, p[dx:dx + X, dy:dy + Y, dz:dz + Z])
    return out


def gaussian_weights(sigma, truncate=4.0):
    """(float64 [2r+1], r): scipy's _gaussian_kernel1d, order 0."""
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return phi / phi.sum(), radius


def correlate_axis(a, w, axis):
    """One pass of a symmetric filter w [2r+1] along `axis`, mode='nearest',
    summed as scipy's correlate1d does for symmetric weights: the centre
    term, then the pairs from the outermost inwards."""
    r = len(w) // 2
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    n = a.shape[0]
    p = np.concatenate([np.repeat(a[:1], r, axis=0), a, np.repeat(a[-1:], r, axis=0)]) if r else a
    t = a * w[r]
    for i in range(r, 0, -1):
        t = t + (p[r - i:r - i + n] + p[r + i:r + i + n]) * w[r - i]
    return np.ascontiguousarray(np.moveaxis(t, 0, axis))


def gaussian(a, sigma=5):
    """skimage.filters.gaussian(a, sigma): gaussian_filter, mode='nearest',
    truncate 4, float64, axes 0, 1, 2 in order."""
    w, _ = gaussian_weights(sigma)
    for axis in range(3):
        a = correlate_axis(a, w, axis)
    return a


def peak_candidates(h):
    """(linear indices ascending, values): voxels that equal the maximum of
    their edge-clamped 3x3x3 neighbourhood, are > min(h) and lie off the
    outermost layer of every axis."""
    X, Y, Z = h.shape
    p = np.pad(h, 1, mode='edge')
    m = np.full_like(h, -np.inf)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                m = np.maximum(m, p[dx:dx + X, dy:dy + Y, dz:dz + Z])
    ok = (h == m) & (h > h.min())
    inner = np.zeros_like(ok)
    inner[1:-1, 1:-1, 1:-1] = True
    lin = np.flatnonzero(ok & inner)
    return lin, h.reshape(-1)[lin]


def select_peaks(lin, values, shape, num_peaks=100):
    """int64 [n,3]: candidates by descending value (ties in C order); one
    within Chebyshev distance 1 of an earlier kept one is dropped; the first
    num_peaks kept."""
    lin, values = np.asarray(lin, dtype=np.int64), np.asarray(values, dtype=np.float64)
    first = np.sort(lin, kind='stable')
    vals = values[np.argsort(lin, kind='stable')]
    order = np.argsort(-vals, kind='stable')
    coords = np.stack(np.unravel_index(first[order], shape), axis=1).reshape(-1, 3)
    kept = []
    for c in coords:
        if len(kept) == num_peaks:
            break
        if all(np.abs(c - k).max() > 1 for k in kept):
            kept.append(c)
    return np.array(kept, dtype=np.int64).reshape(-1, 3)


def peak_local_max(h, min_distance=1, num_peaks=100):
    assert min_distance == 1
    lin, values = peak_candidates(h)
    return select_peaks(lin, values, h.shape, num_peaks)


def labels(c, peaks, mask=None, label_offset=0):
    """float64 [X,Y,Z] (:609-626): the index of the nearest peak of each
    voxel's vote, fp32 distances, strict comparison from 100000."""
    shape = c.shape[1:]
    label = np.zeros(shape)
    nearest = np.full(shape, FARTHEST, dtype=np.float32)
    for i, p in enumerate(np.asarray(peaks).reshape(-1, 3)):
        with np.errstate(invalid='ignore', over='ignore'):
            d0, d1, d2 = (c[a] - np.float32(p[a]) for a in range(3))
            d = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
            won = nearest > d
        label[won] = i + label_offset
        nearest[won] = d[won]
    if mask is not None:
        m = np.asarray(mask)
        if m.ndim == 5:
            m = m[0, 0]
        label[m.astype(np.float32) < np.float32(0.2)] = 0
    return label


def smoothed(counts, sigma=5):
    return gaussian(max_filter2(normalise(counts)), sigma)


def pixel_vec_to_cell(vector, mask, peaks=None, num_peaks=100, sigma=5, label_offset=0):
    """vector [1,3,X,Y,Z] or [3,X,Y,Z] float32; returns dict(counts, hist,
    smooth, peaks, label)."""
    v = np.asarray(vector)
    if v.ndim == 5:
        v = v[0]
    c = centres(v)
    counts = vote_counts(c)
    smooth = smoothed(counts, sigma)
    if peaks is None:
        peaks = peak_local_max(smooth, 1, num_peaks)
    return dict(counts=counts, hist=normalise(counts), smooth=smooth, peaks=np.asarray(peaks),
                label=labels(c, peaks, mask, label_offset))
