"""numpy restatement of the cell tables (hcunet_amd/cells.py: cell_table) and
of what generate_cell_objects derives from them, written from the list in the
module docstring of hcunet_amd/cells.py and hcunet_amd/haircell.py; pinned to
the reference's own HairCell / generate_cell_objects by tests/test_cells.py
through tests/golden/cells.npz.

The per-id loop below is the host baseline the device path replaces: a
full-volume mask per id.  mean and std are float64 by math.fsum (the exactly
rounded sum), so they carry no summation-order error of their own."""
import math

import numpy as np


def cell_table(image, labels):
    """image [1,C,X,Y,Z] (read as float32), labels [X,Y,Z] or [1,1,X,Y,Z] ->
    dict of ids, boxes int64 [n,6], count int64 [n], plane_count int64 [n,Z],
    box_min float32 [n], mean / std float64 [n,C], median float32 [n,C,2]."""
    img = np.asarray(image).astype(np.float32)[0]
    labels = np.asarray(labels)
    if labels.ndim != 3:
        labels = labels[0, 0]
    C, Z = img.shape[0], labels.shape[2]
    ids = np.unique(labels)
    ids = ids[ids != 0]
    n = len(ids)
    out = dict(ids=ids, boxes=np.zeros((n, 6), np.int64), count=np.zeros(n, np.int64),
               plane_count=np.zeros((n, Z), np.int64), box_min=np.zeros(n, np.float32),
               mean=np.full((n, C), np.nan), std=np.full((n, C), np.nan),
               median=np.full((n, C, 2), np.nan, np.float32))
    for i, id in enumerate(ids):
        whole = labels == id
        x, y, z = np.nonzero(whole)
        x0, y0, z0, x1, y1, z1 = x.min(), y.min(), z.min(), x.max(), y.max(), z.max()
        out['boxes'][i] = x0, y0, z0, x1, y1, z1
        box = img[:, x0:x1, y0:y1, z0:z1]          # the maximum faces dropped
        mask = whole[x0:x1, y0:y1, z0:z1]
        cnt = int(mask.sum())
        out['count'][i] = cnt
        out['plane_count'][i, z0:z1] = mask.sum(axis=(0, 1))
        with np.errstate(invalid='ignore'):
            bmin = box.min() if box.size else np.float32(np.inf)   # NaN propagates
        out['box_min'][i] = bmin
        if cnt <= 1:
            continue
        for c in range(C):
            g = box[c][mask]
            if bmin < 0:
                g = g * np.float32(0.5) + np.float32(0.5)
            assert g.dtype == np.float32
            if np.isnan(g).any():
                continue
            g64 = g.astype(np.float64)
            mean = math.fsum(g64) / cnt
            out['mean'][i, c] = mean
            out['std'][i, c] = math.sqrt(math.fsum((g64 - mean) ** 2) / cnt)
            s = np.sort(g)
            out['median'][i, c] = s[(cnt - 1) // 2], s[cnt // 2]
    return out


def centres(boxes, x_ind_chunk, y_ind_chunk):
    """float64 [n,3]: the centre generate_cell_objects reports (no z0 in the z term)."""
    b = np.asarray(boxes, np.int64)
    return np.stack([b[:, 0] + (b[:, 3] - b[:, 0]) / 2 + x_ind_chunk,
                     b[:, 1] + (b[:, 4] - b[:, 1]) / 2 + y_ind_chunk,
                     (b[:, 5] - b[:, 2]) / 2], axis=1)


def volumes(boxes, plane_count):
    """float64 [n]: 1000e-9 * n_z * (289e-9)**2 added plane by plane over z0:z1 from int 0."""
    out = []
    for b, planes in zip(boxes, plane_count):
        v = 0
        for z in range(int(b[2]), int(b[5])):
            v += 1000e-9 * np.int64(planes[z]) * ((289e-9) ** 2)
        out.append(float(v))
    return np.asarray(out, np.float64)


def medians(median):
    """float32 [n,C]: np.median's value, the float32 mean of the two middle order statistics."""
    m = np.asarray(median, np.float32)
    return ((m[..., 0] + m[..., 1]).astype(np.float32) / np.float32(2)).astype(np.float32)


def key(f):
    """uint32 whose unsigned order is the float32 order (the device's radix key)."""
    b = np.asarray(f, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def mean_bound(n, mean_abs):
    """|numpy float32 mean - exact mean| <= (D + 1) u mean(|g|), u = 2^-24, D =
    32 + ceil(log2 n): numpy sums 128-element blocks with 8 accumulators and
    halves above, so no path to the total is deeper than D additions, and the
    division by n rounds once more."""
    D = 32 + math.ceil(math.log2(n))
    return (D + 1) * 2.0 ** -24 * mean_abs


def std_bound(n, std, mean):
    """|numpy float32 std - exact std| <= (D + 8) u std + u |mean|."""
    D = 32 + math.ceil(math.log2(n))
    return (D + 8) * 2.0 ** -24 * std + 2.0 ** -24 * abs(mean)
