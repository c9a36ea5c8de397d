"""random_rotate inside the device input pass (csrc/augment.hip,
`hcu_ingest_jobs`, through hcat.transforms / hcat.dataloader.Stack): the
fixture chains bit-equal to the reference's own outputs
(tests/golden/rotate.npz), as jobs of the one launch where the chain is a
device chain; batches equal to items; poisoned buffers; and the smallest tile
with inside and outside voxels against the numpy restatement."""
import os

import numpy as np
import pytest
import torch

import hcat.dataloader as hdl
import hcat.transforms as ht
from hcunet_amd import _lib
from hcunet_amd import transforms as tr
from tests import rotate_chains as rc

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'rotate.npz'))
BASE = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'augment.npz'))


def bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def write_stack(path, name, image, mask, pwl):
    # Stack reads <name>.tif, <name>.mask.tif, <name>.pwl.tif; np.save'd arrays, read back with np.load
    for suffix, a in [('.tif', image), ('.mask.tif', mask), ('.pwl.tif', pwl)]:
        with open(os.path.join(path, name + suffix), 'wb') as f:
            np.save(f, a)


@pytest.fixture
def launches(monkeypatch):
    """Every materialise_many call: whether each of its volumes was a job of the hcu_ingest_jobs launch."""
    seen = []
    inner = tr.materialise_many

    def spy(vols, *args, **kw):
        seen.append([tr._is_job(v) and v.rot is not None for v in vols])
        return inner(vols, *args, **kw)

    monkeypatch.setattr(tr, 'materialise_many', spy)
    return seen


@pytest.mark.parametrize('name', rc.DEVICE + rc.HOST)
def test_chain_matches_reference(name, tmp_path, launches):
    np.random.seed(int(GOLD[name + '.seed']))
    chain = rc.chain(ht, name)
    if chain['stack']:
        write_stack(tmp_path, 'vol', *rc.raws(BASE, chain['raw']))
        data = hdl.Stack(str(tmp_path), image_transforms=chain['image'], joint_transforms=chain['joint'],
                         reader=np.load)
        got = data[0]
    else:
        got = [ht.to_tensor()(rc.apply(chain, *rc.raws(BASE, chain['raw']))[0])]
    nxt = np.random.random()
    for key, v in zip(('image', 'mask', 'pwl'), got):
        assert v.is_cuda and v.dtype == torch.float16
        np.testing.assert_array_equal(bits(v), GOLD[name + '.' + key], err_msg=key)
    assert nxt == float(GOLD[name + '.next'])
    # a device chain: every volume a rotated job of ONE launch; a host chain: rotated before it got there
    assert launches == [[name in rc.DEVICE] * len(got)]


def recipe(crop):
    """The `recipe` chain of tests/rotate_chains.py with the crop as a
    parameter: its [37, 33, 9] ends with 47 x rows on one of the two stacks
    below and 42 on the other (random_crop widens x to the whole axis when y is
    short), which no batch can hold; [37, 29, 9] is a real window on both, as
    in tests/test_gpu_augment.py."""
    return dict(joint_transforms=[ht.to_float(), ht.reshape(), ht.nul_crop(1), ht.random_crop(crop),
                                  ht.random_rotate()],
                image_transforms=[ht.random_intensity((-15, 15)), ht.drop_channel(.8), ht.clean_image(),
                                  ht.normalize([.5] * 4, [.5] * 4)])


@pytest.fixture
def two_stacks(tmp_path):
    """Two stacks of different raw sizes: the fixture volume (47 x rows kept by
    nul_crop) and its [12,40,57] corner (42 kept: the second box is cut)."""
    image, mask, pwl = rc.raws(BASE, 'base')
    write_stack(tmp_path, 'a', image, mask, pwl)
    write_stack(tmp_path, 'b', np.ascontiguousarray(image[:, :40, :57]), np.ascontiguousarray(mask[:, :40, :57]),
                np.ascontiguousarray(pwl[:, :40, :57]))
    return str(tmp_path)


def test_batches_equal_items(two_stacks, launches):
    data = hdl.Stack(two_stacks, reader=np.load, **recipe([37, 29, 9]))
    np.random.seed(31)
    items = [data[0], data[1]]
    np.random.seed(31)
    batches = list(data.batches(2))
    assert len(batches) == 1
    assert launches == [[True] * 3, [True] * 3, [True] * 6]   # the batch: six rotated jobs, one launch
    for k in range(3):
        assert batches[0][k].shape == (2, 4 if k == 0 else 1, 37, 29, 9)
        for b in range(2):
            np.testing.assert_array_equal(bits(batches[0][k][b:b + 1]), bits(items[b][k]))
    # each item rotated its image, mask and pwl alike: where a whole z column of the (random, non-zero) pwl is 0
    # the rotation cut the corner, so the mask is 0 there and every image channel holds one constant
    image, mask, pwl = (x.cpu().numpy() for x in batches[0])
    for b in range(2):
        cut = (pwl[b, 0] == 0).all(axis=-1)
        assert cut.any() and not cut.all() and (mask[b, 0][cut] == 0).all()
        corner = image[b][:, cut]
        assert (corner == corner[:, :1, :1]).all()


def test_poisoned_buffers_do_not_show(two_stacks, monkeypatch):
    """tests/test_gpu_poison.py's convention: bitwise the same whatever _lib.empty's buffers held."""
    runs = []
    for fill in (None, 0xFF, 0x3F):
        monkeypatch.setattr(_lib, 'POISON', fill)
        data = hdl.Stack(two_stacks, reader=np.load, **recipe([37, 29, 9]))
        np.random.seed(5)
        out = list(next(iter(data.batches(2)))) + list(data[1])
        torch.cuda.synchronize()
        runs.append([bits(x) for x in out])
    monkeypatch.setattr(_lib, 'POISON', None)
    assert all(np.isfinite(x.view(np.float16)).all() for x in runs[0])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('angle', [45, 90])
def test_smallest_tile_equals_the_restatement(angle):
    """An 8x8x2 one-channel uint8 stack: one tile, far narrower than its 32 x
    lanes, with inside and outside voxels (45 degrees cuts the corners)."""
    raw = np.random.default_rng(angle).integers(1, 256, size=(2, 8, 8, 1)).astype(np.uint8)
    v = ht.random_rotate(angle)(ht.reshape()(ht.to_float()(raw.copy())))
    assert tr._is_job(v) and v.rot is not None
    want = tr.rotate_nearest((raw.astype(np.float64) / 2 ** 8).swapaxes(2, 0), *tr.cos_sin(angle))
    assert ((want == 0).any() and (want != 0).any()) if angle == 45 else (want != 0).all()
    want = np.moveaxis(want.astype(np.float32).astype(np.float16), -1, 0)[None].view(np.uint16)
    np.testing.assert_array_equal(bits(ht.to_tensor()(v)), want)
