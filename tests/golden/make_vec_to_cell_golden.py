#!/usr/bin/env python3
"""Generate tests/golden/vec_to_cell.npz from the REFERENCE's own
pixel_vec_to_cell and hist3d (development container only; needs the reference
checkout make_golden.py names).

As make_segment_golden.py: hcat/segment.py imports numba and skimage at module
level (absent here), so the two functions (:563-658) are taken from the
reference file with `ast` at generation time and executed in a namespace
holding numpy, torch, scipy.ndimage as `ndi`, `njit` as the identity and a
stand-in `skimage` with two stubs, whose names the fixture records:
  skimage.filters.gaussian(a, sigma)      -> scipy.ndimage.gaussian_filter(a, sigma, mode='nearest', truncate=4.0)
  skimage.feature.peak_local_max(h, ...)  -> tests/vec_to_cell_oracle.peak_local_max
Nothing from the reference is stored: the fixture holds the inputs, the arrays
the reference returned for them and the restatement's intermediate volumes.

Inputs.  'a' [64,44,6]: every voxel points at the nearest of four centres,
plus N(0, 0.6) noise (default_rng(0)), fp32 rounded through fp16 (stored as
fp16); mask all ones.  'b' [23,45,5]: three centres, default_rng(1) noise, a
random uint8 mask with about a quarter of the voxels off.

Usage:  python tests/golden/make_vec_to_cell_golden.py
"""
import ast
import contextlib
import io
import os
import sys
import types

import numpy as np
import scipy.ndimage
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import REF  # noqa: E402
from tests import vec_to_cell_oracle as vo  # noqa: E402

GAUSSIAN_STUB = "scipy.ndimage.gaussian_filter(a, sigma, mode='nearest', truncate=4.0)"
PEAK_STUB = 'tests.vec_to_cell_oracle.peak_local_max'

CASES = {
    'a': dict(shape=(64, 44, 6), centres=[(12, 10, 2), (48, 12, 3), (14, 34, 2), (50, 31, 4)], seed=0, mask=None),
    'b': dict(shape=(23, 45, 5), centres=[(6, 9, 2), (16, 24, 2), (8, 37, 3)], seed=1, mask=0.75),
}


def field(shape, centres, seed):
    """fp16 [1,3,X,Y,Z]: v[2], v[1], v[0] = centre - (x, y, z) of the nearest centre, plus noise."""
    grid = np.indices(shape).astype(np.float64)
    cen = np.asarray(centres, dtype=np.float64)
    d = ((grid[None] - cen[:, :, None, None, None]) ** 2).sum(1)
    near = cen[np.argmin(d, axis=0)]                       # [X,Y,Z,3]
    to_centre = np.moveaxis(near, -1, 0) - grid            # [3,X,Y,Z]: (c0 - x, c1 - y, c2 - z)
    v = to_centre[::-1] + np.random.default_rng(seed).normal(0, 0.6, size=(3,) + tuple(shape))
    return v.astype(np.float32).astype(np.float16)[None]


def reference_functions():
    tree = ast.parse(open(os.path.join(REF, 'hcat', 'segment.py')).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ('pixel_vec_to_cell', 'hist3d')]
    assert len(body) == 2
    seen = {}

    def gaussian(a, sigma):
        return scipy.ndimage.gaussian_filter(a, sigma, mode='nearest', truncate=4.0)

    def peak_local_max(h, min_distance, num_peaks):
        seen['peaks'] = vo.peak_local_max(h, min_distance, num_peaks)
        return seen['peaks']

    def hist3d_spy(fn):
        def run(mat):
            seen['hist'] = fn(mat)
            return seen['hist']
        return run

    ns = {'np': np, 'torch': torch, 'ndi': scipy.ndimage, 'njit': lambda f: f,
          'skimage': types.SimpleNamespace(filters=types.SimpleNamespace(gaussian=gaussian),
                                           feature=types.SimpleNamespace(peak_local_max=peak_local_max))}
    exec(compile(ast.Module(body=body, type_ignores=[]), 'reference:hcat/segment.py', 'exec'), ns)
    ns['hist3d'] = hist3d_spy(ns['hist3d'])
    return ns, seen


def main():
    ns, seen = reference_functions()
    out = dict(gaussian_stub=np.asarray(GAUSSIAN_STUB), peak_stub=np.asarray(PEAK_STUB),
               scipy_version=np.asarray(scipy.__version__))
    for name, case in CASES.items():
        shape = case['shape']
        vector = field(shape, case['centres'], case['seed'])
        if case['mask'] is None:
            mask = np.ones((1, 1) + shape, dtype=np.float32)
        else:
            mask = (np.random.default_rng(case['seed'] + 100).random((1, 1) + shape) < case['mask']).astype(np.uint8)
        with contextlib.redirect_stdout(io.StringIO()):
            label = ns['pixel_vec_to_cell'](torch.from_numpy(vector), torch.from_numpy(mask))
        mine = vo.pixel_vec_to_cell(vector.astype(np.float32), mask)
        assert label.dtype == np.float64 and seen['hist'].dtype == np.float64
        out.update({name + '.vector': vector, name + '.mask': mask, name + '.hist': seen['hist'],
                    name + '.label': label, name + '.counts': mine['counts'].astype(np.int32),
                    name + '.smooth': mine['smooth'], name + '.peaks': mine['peaks'].astype(np.int64)})
        top = np.sort(mine['smooth'][tuple(mine['peaks'].T)])[::-1]
        print(name, 'votes dropped', int(np.prod(shape) - mine['counts'].sum()), 'max count', int(mine['counts'].max()),
              'peaks', mine['peaks'].tolist(), 'label counts', np.unique(label, return_counts=True)[1].tolist(),
              'smallest gap of peak values', float(np.min(-np.diff(top))) if len(top) > 1 else None,
              'restatement == reference:', np.array_equal(mine['hist'], seen['hist']),
              np.array_equal(mine['label'], label), np.array_equal(mine['peaks'], seen['peaks']))
    path = os.path.join(HERE, 'vec_to_cell.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
