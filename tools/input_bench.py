#!/usr/bin/env python3
"""Input-path benchmark: batches of randomly cropped, augmented training
volumes from two 1024x1024x32 stacks (4-channel uint16 image, uint8 mask,
uint16 pixel-weight map, generated from a seed).

The chain is the reference's training recipe (tests/transforms_test.py:22-39)
plus random_gamma and spekle, cropped to 256x256x16:
  joint  to_float, reshape, nul_crop(1), random_crop([256, 256, 16])
  image  random_gamma, random_intensity, drop_channel, spekle, clean_image, normalize

  --mode device    hcat.transforms' lazy classes and Stack.batches: resident raw
                   stacks, one hcu_ingest_jobs launch per batch on a side stream.
  --mode fallback  the same recipe with crop / augmentation classes defined
                   HERE (plain numpy, as a caller's own classes): Stack hands
                   them PendingVolume.to_ndarray(), the whole stack converted
                   to float64 on the host, and a batch is built item by item.
                   This is the only way to run the recipe on a tree whose
                   hcat.transforms lacks the classes, so it also runs there.

  --rotate         appends random_rotate() to the joint chain, after random_crop
                   (the reference's geometric step, hcat/transforms.py:230-254):
                   ht.random_rotate() in device mode, one more job field of the
                   same launch; in fallback mode a caller's own class that
                   calls scipy.ndimage.rotate as the reference does.

Batches are timed with device events around the whole loop after a warm-up
(the consumer only waits for each batch, so this is the input path alone).
Prints one JSON line.  `--merge RESULT.json --stats-csv KERNEL_STATS.csv` runs
nothing: it adds the kernel's own time, taken from a separate
`rocprofv3 --kernel-trace --stats` run of this tool, to an earlier result and
reports the kernel's bytes (raw window read + fp16 written) over that time
against 8 TB/s.
"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hcat.dataloader as hdl  # noqa: E402
import hcat.transforms as ht  # noqa: E402

CROP = [256, 256, 16]
PEAK_BYTES_PER_S = 8e12


# ---- a caller's own numpy transforms (fallback mode) -------------------------
class np_nul_crop:
    def __call__(self, vols):
        np.random.random()
        m = vols[1]
        lr = m.sum(axis=(1, 2, 3)) > 1
        vols = [v[lr] for v in vols]
        ud = vols[1].sum(axis=(0, 2, 3)) > 1
        return [v[:, ud] for v in vols]


class np_random_crop:
    def __init__(self, dim):
        self.dim = dim

    def __call__(self, vols):
        np.random.seed(np.random.randint(0, 1e8, 1))
        s, d = vols[0].shape, self.dim
        o = [int(np.random.randint(0, s[i] - d[i] + 1, 1)[0]) for i in range(3)]
        return [v[o[0]:o[0] + d[0], o[1]:o[1] + d[1], o[2]:o[2] + d[2]] for v in vols]


class np_random_rotate:
    """The reference's random_rotate on a list, with scipy as it calls it."""

    def __call__(self, vols):
        from scipy import ndimage
        np.random.seed(np.random.randint(0, 1e8, 1))
        theta = np.random.randint(0, 360, 1)[0]
        return [ndimage.rotate(v.astype(float), axes=(0, 1), angle=theta, reshape=False, order=0, mode='constant',
                               prefilter=False) for v in vols]


class np_augment:
    """random_gamma, random_intensity, drop_channel, spekle, clean_image on a float image."""

    def __call__(self, a):
        a = a ** np.random.uniform(.8, 1.2, 1)
        val = np.random.randint(-15, 15, a.shape[-1]) / 100
        for c in range(a.shape[-1]):
            if np.random.random() > 0:
                a[..., c] -= val[c]
        a[a < 0] = 0
        if np.random.random() > .8:
            a[..., np.random.randint(0, a.shape[-1])] = 0
        a = a + np.float32(np.random.normal(0, .05, a.shape))
        a[a < 0] = 0
        a[a > 1] = 1
        a[np.isnan(a)] = 0
        a[np.isinf(a)] = 1
        return a


def make_stacks(seed, n, X, Y, Z):
    """{file name: array} of n seeded stacks; the mask is one box per stack that
    leaves a nul_crop'd volume larger than the crop."""
    rng = np.random.default_rng(seed)
    files = {}
    for i in range(n):
        files['s%d.tif' % i] = rng.integers(0, 65536, size=(Z, Y, X, 4), dtype=np.uint16)
        mask = np.zeros((Z, Y, X), dtype=np.uint8)
        mask[:, Y // 8 + 3 * i:Y - Y // 8, X // 10:X - X // 10 - 5 * i] = 255
        files['s%d.mask.tif' % i] = mask
        files['s%d.pwl.tif' % i] = rng.integers(0, 65536, size=(Z, Y, X), dtype=np.uint16)
    return files


def build(mode, files, tmp, rotate=False):
    for n in files:
        open(os.path.join(tmp, n), 'wb').close()
    if mode == 'device':
        joint = [ht.to_float(), ht.reshape(), ht.nul_crop(1), ht.random_crop(CROP)]
        image = [ht.random_gamma((.8, 1.2)), ht.random_intensity((-15, 15)), ht.drop_channel(.8), ht.spekle(.05),
                 ht.clean_image(), ht.normalize([.5] * 4, [.5] * 4)]
    else:
        joint = [ht.to_float(), ht.reshape(), np_nul_crop(), np_random_crop(CROP)]
        image = [np_augment(), ht.normalize([.5] * 4, [.5] * 4)]
    if rotate:
        joint.append(ht.random_rotate() if mode == 'device' else np_random_rotate())
    return hdl.Stack(tmp, image_transforms=image, joint_transforms=joint,
                     reader=lambda p: files[os.path.basename(p)])


def batches(mode, data, B, n):
    order = [i % len(data) for i in range(B * n)]
    if mode == 'device':
        yield from data.batches(B, order=order)
    else:
        for k in range(n):
            items = [data[i] for i in order[k * B:(k + 1) * B]]
            yield tuple(torch.cat([it[j] for it in items]) for j in range(3))


def kernel_ms(path, name='ingest_jobs_kernel'):
    """(calls, average ms) of the kernel in a rocprofv3 kernel-stats CSV."""
    with open(path) as f:
        for row in csv.DictReader(f):
            if name in row.get('Name', ''):
                return int(row['Calls']), float(row['AverageNs']) * 1e-6
    raise SystemExit('no %s in %s' % (name, path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['device', 'fallback'], default='device')
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--batches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--size', type=int, nargs=3, default=[1024, 1024, 32], metavar=('X', 'Y', 'Z'))
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--rotate', action='store_true')
    ap.add_argument('--stats-csv', default=None)
    ap.add_argument('--merge', default=None)
    args = ap.parse_args()
    if args.merge:
        res = json.loads(open(args.merge).read().strip().splitlines()[-1])
        calls, ms = kernel_ms(args.stats_csv)
        rate = res['kernel_bytes_per_batch'] / (ms * 1e-3)
        res.update(kernel_calls=calls, kernel_ms=ms, kernel_bytes_per_s=rate,
                   kernel_share_of_8TBps=rate / PEAK_BYTES_PER_S)
        print(json.dumps(res))
        return
    if not torch.cuda.is_available():
        raise SystemExit('input_bench: no ROCm device (a time measured without one means nothing)')
    files = make_stacks(args.seed, 2, *args.size)
    with tempfile.TemporaryDirectory() as tmp:
        data = build(args.mode, files, tmp, args.rotate)
        np.random.seed(args.seed)
        for out in batches(args.mode, data, args.batch, args.warmup):
            pass
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for out in batches(args.mode, data, args.batch, args.batches):
            pass
        e1.record()
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3 / args.batches
    B = args.batch
    vox = CROP[0] * CROP[1] * CROP[2]
    # per item: image 4 x uint16 read + 4 x fp16 written, mask uint8 + fp16, pwl uint16 + fp16
    # (with --rotate a voxel whose source lies outside reads nothing: an upper bound then)
    nbytes = B * vox * ((8 + 8) + (1 + 2) + (2 + 2))
    res = dict(tool='input_bench', mode=args.mode, rotate=args.rotate, batch=B, batches=args.batches,
               warmup=args.warmup,
               stack=args.size, crop=CROP, out_shape=list(out[0].shape),
               ms_per_batch=e0.elapsed_time(e1) / args.batches, host_ms_per_batch=host_ms,
               kernel_bytes_per_batch=nbytes)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
