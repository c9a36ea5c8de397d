#!/usr/bin/env python3
"""Generate tests/golden/targets.npz from the REFERENCE's own training-target
generators (development container only; needs /root/reference).

As make_augment_golden.py: hcat/train/train_utils.py imports skimage and numba
at module level (absent here), so makePWL (:9-93), colormask_to_mask
(:175-187), CalculateCenterOfMass (:190-237) and VectorToCenter (:240-274) are
taken from the reference file with `ast` at generation time and executed in a
namespace holding scipy.ndimage, `njit` as the identity, an `io.imread` that
returns the fixture array of that name, and numpy behind a stand-in that also
answers `np.bool` (:213; removed from numpy 1.24).  Nothing from the reference
is stored: the fixture holds the two label stacks and the arrays the
reference returned for them.

The stack, [3, 24, 28, 3] uint16 (its uint8 variant is the high byte of every
channel): cell A touches the x = 0 border; B lies 3 voxels from A and its
colour differs from A's only in channel 2 and only above bit 8; C lies 12
voxels from B (no voxel sees both within radius 9); D is alone in slice 1 and
close to B in slice 2.  Voxel [0, 0, 0] is background.

The pure-Python makePWL loop over the two padded stacks takes a few minutes.

Usage:  python tests/golden/make_targets_golden.py
"""
import ast
import contextlib
import io as _io
import os
import sys

import numpy as np
import scipy
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

KEEP = {'makePWL', 'colormask_to_mask', 'CalculateCenterOfMass', 'VectorToCenter'}


class _Numpy:
    """numpy, plus the alias the reference still uses."""
    bool = bool

    def __getattr__(self, name):
        return getattr(np, name)


class _Files:
    def __init__(self, arrays):
        self.arrays = arrays

    def imread(self, name):
        return self.arrays[name].copy()


def reference_targets(arrays):
    tree = ast.parse(open(os.path.join(REF, 'hcat', 'train', 'train_utils.py')).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in KEEP]
    ns = {'np': _Numpy(), 'scipy': scipy, 'njit': lambda f: f, 'io': _Files(arrays)}
    exec(compile(ast.Module(body=body, type_ignores=[]), 'reference:hcat/train/train_utils.py', 'exec'), ns)
    return ns


def label_stack():
    a = np.zeros((3, 24, 28, 3), dtype=np.uint16)
    A, B = (0x1234, 0x0200, 0x0100), (0x1234, 0x0200, 0x0300)
    C, D = (0x0500, 0xFF00, 0x0100), (0xFFFF, 0x0100, 0x8000)
    for z in (0, 2):
        a[z, 2:8, 0:6] = A
        a[z, 2:8, 9:14] = B
        a[z, 20:23, 9:14] = C
    a[2, 3:7, 4:6] = 0          # A is not the same in every slice (its centre is no lattice point)
    a[1, 11:14, 22:25] = D
    a[2, 9:12, 15:19] = D
    return a


def main():
    u16 = label_stack()
    arrays = {'u16': u16, 'u8': (u16 >> 8).astype(np.uint8)}
    T = reference_targets(arrays)
    out = {}
    for name, a in arrays.items():
        out[name + '.labels'] = a
        with contextlib.redirect_stdout(_io.StringIO()):
            pwl = T['makePWL']()(name)
            com, ids = T['CalculateCenterOfMass']()(name)
            vec = T['VectorToCenter']()(com, ids, None)
            binary = a.copy()
            mask = T['colormask_to_mask'](binary)
        assert pwl.dtype == np.float64 and com.dtype == np.float64 and ids.dtype == np.uint32
        assert vec.dtype == np.float64 and mask.dtype == np.uint8 and binary.dtype == a.dtype
        out[name + '.pwl'] = pwl
        out[name + '.com'] = com
        out[name + '.ids'] = ids
        out[name + '.vec'] = vec
        out[name + '.mask'] = mask
        out[name + '.binary'] = binary
        print(name, 'pwl max', pwl.max(), 'distinct', len(np.unique(pwl)), 'ids', int(ids.max()),
              'centres', np.argwhere(com > 0).tolist())
    np.savez_compressed(os.path.join(HERE, 'targets.npz'), **out)


if __name__ == '__main__':
    main()
