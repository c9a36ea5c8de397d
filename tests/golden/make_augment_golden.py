#!/usr/bin/env python3
"""Generate tests/golden/augment.npz from the REFERENCE's own crop and
augmentation transforms (development container only; needs /root/reference).

As make_input_golden.py: hcat/transforms.py imports skimage, cv2 and
elasticdeform at module level (absent here), so the classes the chains use --
joint_transform (:15-91), to_float, to_tensor, reshape, normalize,
drop_channel (:285-298), random_intensity (:301-334), random_crop (:337-396),
nul_crop (:460-489), remove_channel (:590-613), clean_image (:616-631) -- are
taken from the reference file with `ast` at generation time and executed in a
namespace holding numpy, torch and copy.  The chains are those of
tests/augment_chains.py.  Nothing from the reference is stored: the fixture
holds the raw inputs, each chain's numpy seed, the reference's fp16 outputs
(as uint16 bits), the np.random.random() drawn right after the chain (which
pins the number and order of the draws) and exception type names.

Usage:  python tests/golden/make_augment_golden.py
"""
import ast
import copy
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from make_input_golden import bits  # noqa: E402
import augment_chains as ac  # noqa: E402

KEEP = {'joint_transform', 'to_float', 'to_tensor', 'reshape', 'normalize', 'drop_channel', 'random_intensity',
        'random_crop', 'nul_crop', 'remove_channel', 'clean_image'}
SEEDS = {'crop': 11, 'order': 5, 'order_f64': 6, 'remove': 7, 'nul_rate0': 8, 'quirk_x_whole': 9,
         'quirk_short_z': 10, 'quirk_too_small': 12}


def reference_transforms():
    tree = ast.parse(open(os.path.join(REF, 'hcat', 'transforms.py')).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in KEEP]
    ns = {'np': np, 'torch': torch, 'copy': copy}
    exec(compile(ast.Module(body=body, type_ignores=[]), 'reference:hcat/transforms.py', 'exec'), ns)
    return ns


def raw_inputs():
    rng = np.random.default_rng(21)
    out = {}
    Z, Y, X = 12, 45, 70
    out['base.image'] = rng.integers(0, 65536, size=(Z, Y, X, 4)).astype(np.uint16)
    # two separated boxes (47 x rows, 29 y rows) and one isolated voxel, whose
    # row sums to 255 / 256: not > 1, so nul_crop drops it
    mask = np.zeros((Z, Y, X), dtype=np.uint8)
    mask[2:9, 3:15, 5:25] = 255
    mask[4:11, 20:37, 35:62] = 255
    mask[5, 41, 66] = 255
    out['base.mask'] = mask
    out['base.pwl'] = rng.integers(0, 65536, size=(Z, Y, X)).astype(np.uint16)
    f = rng.random((5, 9, 11, 4)) * 1.2 - 0.1
    f[0, 0, 0, 0], f[1, 2, 3, 1], f[2, 3, 4, 2], f[4, 8, 10, 3] = np.nan, np.inf, -np.inf, np.nan
    out['f64.image'] = f
    return out


def run(T, name, G, seed):
    """(fp16 bits of each output | exception type name, the next draw)."""
    chain = ac.chains(T)[name]
    np.random.seed(seed)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', DeprecationWarning)   # int(1-element array), numpy >= 1.25
            vols = ac.apply(chain, *ac.raws(G, chain['raw']))
            vols = T['to_tensor']()(vols if len(vols) > 1 else vols[0])
    except Exception as e:  # noqa: BLE001
        return type(e).__name__, None
    vols = vols if isinstance(vols, list) else [vols]
    return [bits(v) for v in vols], np.random.random()


def main():
    T = reference_transforms()
    out = raw_inputs()
    # the recipe's seed: the first one under which drop_channel drops a channel
    # and random_intensity lifts values above 1 (a wrong upper clamp would show)
    for seed in range(100, 400):
        res, _ = run(T, 'recipe', out, seed)
        img = res[0].view(np.float16)
        if any((img[0, c] == -1).all() for c in range(4)) and img.max() > 1.02:   # (0 - .5) / .5
            SEEDS['recipe'] = seed
            break
    for name, seed in SEEDS.items():
        res, nxt = run(T, name, out, seed)
        out[name + '.seed'] = np.array(seed)
        if isinstance(res, str):
            out[name + '.error'] = np.array(res)
            print(name, 'raises', res)
            continue
        out[name + '.next'] = np.array(nxt)
        for key, b in zip(('image', 'mask', 'pwl'), res):
            out[name + '.' + key] = b
        print(name, seed, [b.shape for b in res], 'max', float(res[0].view(np.float16).astype(np.float32).max()))
    np.savez_compressed(os.path.join(HERE, 'augment.npz'), **out)


if __name__ == '__main__':
    main()
