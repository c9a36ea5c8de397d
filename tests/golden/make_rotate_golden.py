#!/usr/bin/env python3
"""Generate tests/golden/rotate.npz from the REFERENCE's own random_rotate
(development container only; needs the reference tree, make_golden.REF, and
scipy).

As make_augment_golden.py: the classes the chains of tests/rotate_chains.py use
-- joint_transform (:15-91), to_float, to_tensor, reshape, normalize,
random_affine (:200-227), random_rotate (:230-254), drop_channel,
random_intensity, random_crop, nul_crop, clean_image -- are taken from the
reference file with `ast` at generation time and executed in a namespace
holding numpy, torch, copy and `ndimage = scipy.ndimage`.  The reference calls
image.astype(np.float), an alias numpy 1.24 removed: the namespace's `np`
forwards to numpy and answers `float` with the builtin, there only.

Nothing from the reference is stored, and the raw inputs are those of
tests/golden/augment.npz (not copied): the fixture holds each chain's numpy
seed, the reference's fp16 outputs (as uint16 bits), the np.random.random()
drawn right after the chain (which pins the number and order of the draws) and
exception type names.

Usage:  python tests/golden/make_rotate_golden.py
"""
import ast
import copy
import os
import sys
import warnings

import numpy
import scipy.ndimage
import scipy.special
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from make_input_golden import bits  # noqa: E402
import rotate_chains as rc  # noqa: E402

KEEP = {'joint_transform', 'to_float', 'to_tensor', 'reshape', 'normalize', 'random_crop', 'nul_crop',
        'random_intensity', 'drop_channel', 'clean_image', 'random_rotate', 'random_affine'}


class _Numpy:
    """numpy with the removed alias `float` (the builtin, as it was)."""

    def __getattr__(self, name):
        return float if name == 'float' else getattr(numpy, name)


def reference_transforms():
    tree = ast.parse(open(os.path.join(REF, 'hcat', 'transforms.py')).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in KEEP]
    ns = {'np': _Numpy(), 'torch': torch, 'copy': copy, 'ndimage': scipy.ndimage}
    exec(compile(ast.Module(body=body, type_ignores=[]), 'reference:hcat/transforms.py', 'exec'), ns)
    return ns


def run(T, name, G):
    """(fp16 bits of each output | exception type name, the next draw)."""
    numpy.random.seed(rc.SEEDS[name])
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')   # int(1-element array); the overflow to fp16 Inf of host_before_to_float
            chain = rc.chain(T, name)
            vols = rc.apply(chain, *rc.raws(G, chain['raw']))
            vols = T['to_tensor']()(vols if len(vols) > 1 else vols[0])
    except Exception as e:  # noqa: BLE001
        return type(e).__name__, None
    vols = vols if isinstance(vols, list) else [vols]
    return [bits(v) for v in vols], numpy.random.random()


def exact_ties(nx, ny, angle):
    """Output voxels of an (nx, ny) plane whose source coordinate along x or y
    is exactly k + 0.5 and inside, by scipy's own arithmetic."""
    c, s = scipy.special.cosdg(angle), scipy.special.sindg(angle)
    m = numpy.array([[c, s], [-s, c]])
    off = (numpy.array([nx, ny]) - 1) / 2 - m @ ((numpy.array([nx, ny]) - 1) / 2)
    u = numpy.arange(nx, dtype=float)[:, None]
    v = numpy.arange(ny, dtype=float)[None, :]
    cx = (u * c + v * s) + off[0]
    cy = (u * -s + v * c) + off[1]
    inside = (cx >= 0) & (cx <= nx - 1) & (cy >= 0) & (cy <= ny - 1)
    return int((inside & ((cx - numpy.floor(cx) == 0.5) | (cy - numpy.floor(cy) == 0.5))).sum())


def main():
    T = reference_transforms()
    G = numpy.load(os.path.join(HERE, 'augment.npz'))
    out = {}
    # `ties`: a 40x40 window rotated by 45 degrees; the seed only moves the window, the ties are in every one
    n_ties = exact_ties(40, 40, 45)
    assert n_ties >= 1, 'the ties chain has no source coordinate at an exact .5'
    print('ties: %d output columns with a source coordinate at exactly k + 0.5' % n_ties)
    for name in rc.SEEDS:
        res, nxt = run(T, name, G)
        out[name + '.seed'] = numpy.array(rc.SEEDS[name])
        if isinstance(res, str):
            out[name + '.error'] = numpy.array(res)
            print(name, 'raises', res)
            continue
        out[name + '.next'] = numpy.array(nxt)
        for key, b in zip(('image', 'mask', 'pwl'), res):
            out[name + '.' + key] = b
        img = res[0].view(numpy.float16).astype(numpy.float32)
        print(name, [b.shape for b in res], 'min', float(img.min()), 'max', float(img.max()))
    assert out['ties.image'].shape == (1, 4, 40, 40, 12)
    # fill_order: outside voxels were 0 when random_intensity saw them, so none is (0 - mean) / std = -0.8
    assert (out['fill_order.image'].view(numpy.float16)[0, 0, 0, 0] >= 0).all()
    # val: the cut corners of the 37x33 window are (0 - .5) / .5
    assert (out['val.image'].view(numpy.float16)[0, :, 0, 0] == -1).all()
    numpy.savez_compressed(os.path.join(HERE, 'rotate.npz'), **out)


if __name__ == '__main__':
    main()
