#!/usr/bin/env python3
"""Generate tests/golden/cells.npz from the REFERENCE's own HairCell and
generate_cell_objects (development container only; needs the reference
checkout make_golden.py names).

As make_vec_to_cell_golden.py: hcat/segment.py imports numba and skimage at
module level (absent here), so the class (hcat/haircell.py:5-85) and the
function (hcat/segment.py:508-560) are taken from the reference files with
`ast` at generation time and executed in a namespace holding torch and numpy.
`np` is bound to a stand-in that forwards to numpy and adds the alias `NaN`
numpy 2 removed, which the bad-cell branch spells.  Nothing from the reference
is stored: the fixture holds the inputs and, per cell, what the reference's
objects reported.

Per case NAME: NAME.image fp16 [1,4,X,Y,Z] (fp32 values exact in fp16),
NAME.labels int64 [X,Y,Z], NAME.chunk (x_ind_chunk, y_ind_chunk), and per cell
NAME.unique_id, .image_coords [n,6], .center [n,3], .volume float64 [n],
.volume_is_int (the int 0 the volume starts as was never added to), .is_bad,
.stats float32 [n,5,3] (dapi, gfp, myo7a, actin of signal_stats, then
gfp_stats; mean, std, median) and .num_samples int64 [n,5] (-1: no such key).

Cases (the list is the issue's; the generator asserts each property):
  a [40,36,7]  values k/1024 in [-1,1], every good cell maps; sparse ids, one
     above 65535; an ellipsoid, two L shapes with overlapping boxes, a cell on
     the minimum faces and one on the maximum faces, a one-voxel cell, a cell
     one z plane thick (bad, volume the int 0), a 2x2x2 cell (clips to one
     voxel: bad, volume not 0), a cell that clips to 2 voxels, one with odd n
  b [48,44,7]  264 cubes of 3x3x3 on a pitch of 4 in two z layers (more ids than
     the device's LDS table), 8 samples each, values k/64 with planted ties:
     the two middle ranks are equal in some cells, part ways in the first
     radix pass (top 8 key bits) in others and in a later pass in others
  c [23,45,5]  values k/1024 in [0,1]; cell 1 has one negative voxel of channel
     3 inside its clipped box but outside its mask (it alone maps); the same
     voxel lies on cell 2's maximum face (no mapping); cell 3 has a NaN of
     channel 2 inside its mask

Usage:  python tests/golden/make_cells_golden.py
"""
import ast
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import REF  # noqa: E402
from tests import cells_oracle as co  # noqa: E402

NAMES = ['dapi', 'gfp', 'myo7a', 'actin']


class NumpyWithNaN:
    """numpy, plus the alias numpy 2 removed."""
    NaN = np.nan

    def __getattr__(self, name):
        return getattr(np, name)


def reference_functions():
    ns = {'np': NumpyWithNaN(), 'torch': torch}
    for path, kind, name in (('haircell.py', ast.ClassDef, 'HairCell'),
                             ('segment.py', ast.FunctionDef, 'generate_cell_objects')):
        tree = ast.parse(open(os.path.join(REF, 'hcat', path)).read())
        body = [n for n in tree.body if isinstance(n, kind) and n.name == name]
        assert len(body) == 1
        exec(compile(ast.Module(body=body, type_ignores=[]), 'reference:hcat/' + path, 'exec'), ns)
    return ns


def grid_values(rng, shape, lo, hi, denom):
    return (rng.integers(lo, hi + 1, size=shape) / denom).astype(np.float32)


def case_a():
    X, Y, Z = 40, 36, 7
    rng = np.random.default_rng(0)
    image = grid_values(rng, (1, 4, X, Y, Z), -1024, 1024, 1024)
    lab = np.zeros((X, Y, Z), np.int64)
    g = np.indices((X, Y, Z)).astype(np.float64)
    lab[((g[0] - 13) / 12.5) ** 2 + ((g[1] - 13) / 12.5) ** 2 + ((g[2] - 3) / 3.9) ** 2 <= 1] = 3
    lab[0:3, 0:3, 0:2] = 7                       # on the minimum faces
    lab[27:35, 2:4, 1:5] = 12                    # L
    lab[27:29, 2:11, 1:5] = 12
    lab[33:36, 5:12, 1:5] = 15                   # L, its box overlaps the other's
    lab[30:36, 10:12, 1:5] = 15
    lab[30, 20, 3] = 20                          # one voxel
    lab[27:31, 24:28, 5:6] = 21                  # one plane thick
    lab[33:35, 16:18, 2:4] = 22                  # 2x2x2: clips to one voxel
    lab[33:36, 20:22, 2:4] = 300                 # clips to 2x1x1
    lab[27:31, 30:34, 1:5] = 301                 # clips to 3x3x3: odd n
    lab[37:40, 33:36, 4:7] = 70000               # on the maximum faces
    return image, lab, (100, 200)


def case_b():
    X, Y, Z = 48, 44, 7
    rng = np.random.default_rng(1)
    image = grid_values(rng, (1, 4, X, Y, Z), -64, 64, 64)
    lab = np.zeros((X, Y, Z), np.int64)
    k = 0
    for z0 in (0, 4):
        for i in range(X // 4):
            for j in range(Y // 4):
                k += 1
                lab[4 * i:4 * i + 3, 4 * j:4 * j + 3, z0:z0 + 3] = k
    assert k == 264
    # planted: every sample equal (cells 5, 140); the middle ranks either side of 0, which after the
    # mapping is either side of 0.5, an exponent step (cells 6, 141); a tie of the middle two only (7)
    for cell, vals in ((5, [0.5] * 8), (140, [-0.25] * 8), (6, [-1, -.5, -.25, -1 / 64, 1 / 64, .25, .5, 1]),
                       (141, [1, -1 / 64, .5, -.5, 1 / 64, -1, .25, -.25]), (7, [-1, -.75, -.5, .125, .125, .5, .75, 1])):
        x, y, z = (int(v.min()) for v in np.nonzero(lab == cell))
        for c in range(4):
            image[0, c, x:x + 2, y:y + 2, z:z + 2] = np.asarray(vals, np.float32).reshape(2, 2, 2)
    return image, lab, (0, 0)


def case_c():
    X, Y, Z = 23, 45, 5
    rng = np.random.default_rng(2)
    image = grid_values(rng, (1, 4, X, Y, Z), 0, 1024, 1024)
    lab = np.zeros((X, Y, Z), np.int64)
    lab[2:8, 3:10, 0:4] = 1
    lab[4, 5, 2] = 0                             # a hole in cell 1 ...
    image[0, 3, 4, 5, 2] = -0.5                  # ... that holds the only negative value
    lab[0:2, 1:6, 0:3] = 2                       # cell 2: box x 0..5, y 0..5, z 0..2, the hole on its y and z maximum
    lab[3:6, 0:2, 0:3] = 2
    lab[12:18, 20:30, 1:5] = 3
    image[0, 2, 14, 24, 2] = np.nan
    return image, lab, (7, 11)


def run_reference(ns, image, lab, chunk):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter('ignore')          # np.median of a NaN
        cells = ns['generate_cell_objects'](torch.from_numpy(image), lab, None, chunk[0], chunk[1])
    n = len(cells)
    stats = np.full((n, 5, 3), np.nan, np.float32)
    num = np.full((n, 5), -1, np.int64)
    for i, cell in enumerate(cells):
        assert list(cell.signal_stats) == NAMES
        for j, d in enumerate([cell.signal_stats[k] for k in NAMES] + [cell.gfp_stats]):
            assert list(d)[:3] == ['mean', 'std', 'median'] and (len(d) == 3) == cell.is_bad
            stats[i, j] = [d['mean'], d['std'], d['median']]
            if not cell.is_bad:
                assert np.asarray(d['mean']).dtype == np.float32 and np.asarray(d['median']).dtype == np.float32
                (num[i, j],) = d['num_samples']
    return dict(unique_id=np.asarray([c.unique_id for c in cells]),
                image_coords=np.asarray([c.image_coords for c in cells], np.int64).reshape(n, 6),
                center=np.asarray([c.center for c in cells], np.float64).reshape(n, 3),
                volume=np.asarray([float(c.volume) for c in cells], np.float64),
                volume_is_int=np.asarray([isinstance(c.volume, int) for c in cells]),
                is_bad=np.asarray([c.is_bad for c in cells]), stats=stats, num_samples=num)


def check(name, image, lab, ref):
    """The properties the case was built for, on the reference's own results."""
    t = co.cell_table(image, lab)
    assert np.array_equal(t['ids'], ref['unique_id'])
    bad, n0 = ref['is_bad'], ref['num_samples'][:, 0]
    one_voxel = 1000e-9 * 1 * ((289e-9) ** 2)
    if name == 'a':
        ids = list(t['ids'])
        assert ids == [3, 7, 12, 15, 20, 21, 22, 300, 301, 70000]
        assert (t['box_min'][~bad] < 0).all()                                   # every good cell maps
        assert 2000 < n0[ids.index(3)] < 4000
        b12, b15 = t['boxes'][ids.index(12)], t['boxes'][ids.index(15)]
        assert (np.maximum(b12[:3], b15[:3]) < np.minimum(b12[3:], b15[3:])).all()   # the clipped boxes overlap
        assert (t['boxes'][ids.index(7)][:3] == 0).all() and (t['boxes'][ids.index(70000)][3:] == (39, 35, 6)).all()
        for id, vol_int, vol in ((20, True, 0.0), (21, True, 0.0), (22, False, one_voxel)):
            i = ids.index(id)
            assert bad[i] and ref['volume_is_int'][i] == vol_int and ref['volume'][i] == vol, id
        assert bad.sum() == 3
        assert n0[ids.index(300)] == 2 and n0[ids.index(301)] == 27 and n0[ids.index(70000)] == 8
    if name == 'b':
        assert len(t['ids']) == 264 > 256 and (n0 == 8).all() and not bad.any()
        lo, hi = co.key(t['median'][..., 0]), co.key(t['median'][..., 1])
        tie, first, later = lo == hi, (lo >> 24) != (hi >> 24), ((lo >> 24) == (hi >> 24)) & (lo != hi)
        print('b: (cell, channel) pairs whose middle ranks tie', int(tie.sum()), 'part in the first pass',
              int(first.sum()), 'part in a later pass', int(later.sum()))
        assert tie.sum() >= 16 and first.sum() >= 8 and later.sum() >= 8
        assert (t['box_min'] < 0).sum() > 200 and (t['box_min'] >= 0).sum() >= 1   # cell 5 does not map
    if name == 'c':
        assert list(t['ids']) == [1, 2, 3] and not bad.any()
        assert t['box_min'][0] == -0.5 and t['box_min'][1] >= 0 and np.isnan(t['box_min'][2])
        assert np.isnan(ref['stats'][2, 2]).all() and np.isnan(ref['stats'][2, 4]).sum() == 0
        assert np.isfinite(ref['stats'][:2]).all() and np.isfinite(ref['stats'][2, [0, 1, 3, 4]]).all()
        # cell 1 mapped (its mean is that of g/2 + 1/2), cell 2 did not
        for i, mapped in ((0, True), (1, False)):
            raw = co.cell_table(np.abs(image), lab)['mean'][i]                  # no negative: no mapping
            want = raw * 0.5 + 0.5 if mapped else raw
            assert np.allclose(ref['stats'][i, :4, 0], want, rtol=1e-5, atol=0), (i, ref['stats'][i, :4, 0], want)


def main():
    ns = reference_functions()
    out = dict(numpy_version=np.asarray(np.__version__))
    for name, make in (('a', case_a), ('b', case_b), ('c', case_c)):
        image, lab, chunk = make()
        image16 = image.astype(np.float16)
        assert np.array_equal(image16.astype(np.float32), image, equal_nan=True)
        ref = run_reference(ns, image, lab, chunk)
        check(name, image, lab, ref)
        out.update({name + '.image': image16, name + '.labels': lab, name + '.chunk': np.asarray(chunk, np.int64)})
        out.update({name + '.' + k: v for k, v in ref.items()})
        print(name, 'cells', len(ref['unique_id']), 'bad', int(ref['is_bad'].sum()), 'samples',
              ref['num_samples'][:, 0].tolist()[:12])
    path = os.path.join(HERE, 'cells.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
