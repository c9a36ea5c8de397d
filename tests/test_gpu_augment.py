"""Crops and augmentation inside the device input pass (csrc/augment.hip,
`hcu_ingest_jobs`, through hcat.transforms / hcat.dataloader.Stack): the
fixture chains bit-equal to the reference's own outputs
(tests/golden/augment.npz), batches equal to items, residency, poisoned
buffers, and the two steps that are not bit-pinned: random_gamma (adjacent fp16
values, rarely) and spekle (its statistics)."""
import os

import numpy as np
import pytest
import torch

import hcat.dataloader as hdl
import hcat.loss as hl
import hcat.transforms as ht
from hcat.unet import Unet_Constructor
from hcunet_amd import _lib
from tests import augment_chains as ac
from tests.helpers import REF_KW

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'augment.npz'))
CHAINS = ['crop', 'recipe', 'order', 'order_f64', 'remove', 'nul_rate0', 'quirk_x_whole', 'quirk_short_z']


def bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def write_stack(path, name, image, mask, pwl):
    # Stack reads <name>.tif, <name>.mask.tif, <name>.pwl.tif; np.save'd arrays, read back with np.load
    for suffix, a in [('.tif', image), ('.mask.tif', mask), ('.pwl.tif', pwl)]:
        with open(os.path.join(path, name + suffix), 'wb') as f:
            np.save(f, a)


@pytest.mark.parametrize('name', CHAINS)
def test_chain_matches_reference(name, tmp_path):
    chain = ac.chains(ht)[name]
    np.random.seed(int(GOLD[name + '.seed']))
    if chain['stack']:
        write_stack(tmp_path, 'vol', *ac.raws(GOLD, chain['raw']))
        data = hdl.Stack(str(tmp_path), image_transforms=chain['image'], joint_transforms=chain['joint'],
                         reader=np.load)
        got = data[0]
    else:
        got = [ht.to_tensor()(ac.apply(chain, *ac.raws(GOLD, chain['raw']))[0])]
    nxt = np.random.random()
    for key, v in zip(('image', 'mask', 'pwl'), got):
        assert v.is_cuda and v.dtype == torch.float16
        np.testing.assert_array_equal(bits(v), GOLD[name + '.' + key], err_msg=key)
    assert nxt == float(GOLD[name + '.next'])


def recipe(crop):
    return dict(joint_transforms=[ht.to_float(), ht.reshape(), ht.nul_crop(1), ht.random_crop(crop)],
                image_transforms=[ht.random_intensity((-15, 15)), ht.drop_channel(.8), ht.clean_image(),
                                  ht.normalize([.5] * 4, [.5] * 4)])


@pytest.fixture
def two_stacks(tmp_path):
    """Two stacks of different raw sizes: the fixture volume (47 x rows kept by
    nul_crop) and its [12,40,57] corner (42 kept: the second box is cut)."""
    image, mask, pwl = ac.raws(GOLD, 'base')
    write_stack(tmp_path, 'a', image, mask, pwl)
    write_stack(tmp_path, 'b', np.ascontiguousarray(image[:, :40, :57]), np.ascontiguousarray(mask[:, :40, :57]),
                np.ascontiguousarray(pwl[:, :40, :57]))
    return str(tmp_path)


def test_batches_equal_items_and_residency(two_stacks):
    kw = recipe([37, 29, 9])
    res = {}
    probe = hdl.Stack(two_stacks, reader=np.load, **kw)
    item0 = sum(r.tensor.numel() * r.tensor.element_size() for r in (probe.image[0], probe.mask[0], probe.pwl[0]))
    for tag, extra in (('resident', {}), ('copied', dict(resident_bytes=0)),
                       ('one_resident', dict(resident_bytes=item0))):   # item 0's stacks fit, item 1's do not
        data = hdl.Stack(two_stacks, reader=np.load, **kw, **extra)
        assert sorted(tuple(r.tensor.shape) for r in data.image) == [(12, 40, 57, 4), (12, 45, 70, 4)]
        np.random.seed(31)
        items = [data[0], data[1]]
        np.random.seed(31)
        batches = list(data.batches(2))
        assert len(batches) == 1
        for k in range(3):
            assert batches[0][k].shape == (2, 4 if k == 0 else 1, 37, 29, 9)
            for b in range(2):
                np.testing.assert_array_equal(bits(batches[0][k][b:b + 1]), bits(items[b][k]))
        np.random.seed(31)
        three = list(data.batches(2, order=[0, 1, 0]))     # a short last batch as it is; prefetch on the side stream
        assert [tuple(b[0].shape) for b in three] == [(2, 4, 37, 29, 9), (1, 4, 37, 29, 9)]
        np.testing.assert_array_equal(bits(three[0][0]), bits(batches[0][0]))
        res[tag] = [bits(x) for x in batches[0]] + [bits(x) for x in three[1]]
        n_res = sum(len(r.device_copy) for r in data.image + data.mask + data.pwl)
        assert n_res == {'resident': 6, 'copied': 0, 'one_resident': 3}[tag]
    for tag in ('copied', 'one_resident'):
        for a, b in zip(res['resident'], res[tag]):
            np.testing.assert_array_equal(a, b)


def test_batches_name_differing_extents(two_stacks):
    # 45 x rows fit stack a's 47 kept rows, stack b's 42 shrink the request: (45,29,9) against (42,29,9)
    data = hdl.Stack(two_stacks, reader=np.load, **recipe([45, 29, 9]))
    np.random.seed(1)
    with pytest.raises(ValueError, match='different extents.*item 0.*item 1'):
        list(data.batches(2))


def test_poisoned_buffers_do_not_show(two_stacks, monkeypatch):
    """tests/test_gpu_poison.py's convention: bitwise the same whatever _lib.empty's buffers held."""
    kw = recipe([37, 29, 9])
    kw['image_transforms'] = kw['image_transforms'][:3] + [ht.spekle(.05)] + kw['image_transforms'][3:]
    runs = []
    for fill in (None, 0xFF, 0x3F):
        monkeypatch.setattr(_lib, 'POISON', fill)
        data = hdl.Stack(two_stacks, reader=np.load, **kw)
        np.random.seed(5)
        out = list(next(iter(data.batches(2)))) + list(data[1])
        torch.cuda.synchronize()
        runs.append([bits(x) for x in out])
    monkeypatch.setattr(_lib, 'POISON', None)
    assert all(np.isfinite(x.view(np.float16)).all() for x in runs[0])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            np.testing.assert_array_equal(a, b)


def test_random_gamma_within_one_fp16_step_of_numpy():
    """numpy's float64 a ** g pushed through the reference rounding: every voxel
    equal or the adjacent fp16 value, and at most 1 voxel in 10^4 unequal (15
    of 151,200).  The cap: a float64 pow within 16 ulp of numpy's flips the
    float32 rounding with probability about 2^-24 per voxel (and the fp16
    rounding of that float32 more rarely still), while a wrong formula flips
    nearly all."""
    raw = GOLD['base.image']
    v = ht.reshape()(ht.to_float()(raw.copy()))
    np.random.seed(17)
    v = ht.random_gamma((.7, 1.3))(v)
    np.random.seed(17)
    g = np.random.uniform(.7, 1.3, 1)
    got = bits(ht.to_tensor()(v)).astype(np.int32)
    a = (raw.astype(np.float64) / 2 ** 16).swapaxes(2, 0) ** g
    want = np.moveaxis(a.astype(np.float32).astype(np.float16), -1, 0)[None].view(np.uint16).astype(np.int32)
    assert got.size == 151200
    diff = np.abs(got - want)          # non-negative finite halves: adjacent values are adjacent bit patterns
    print('random_gamma: unequal', int((diff != 0).sum()), 'of', got.size, 'max step', int(diff.max()))
    assert diff.max() <= 1
    assert (diff != 0).sum() <= 15


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_spekle_statistics(tmp_path):
    """spekle(0.05) on a constant 0.5 image, N = 64*64*16*4 per item, two items
    in one batch.  fp16 spacing in [0.25, 0.5) is 2^-12 and in [0.5, 1) 2^-11 = q."""
    gamma, q = 0.05, 2.0 ** -11
    shape = (16, 64, 64, 4)
    N = int(np.prod(shape))
    for n in 'ab':
        write_stack(tmp_path, n, np.full(shape, 32768, np.uint16), np.full(shape[:3], 255, np.uint8),
                    np.zeros(shape[:3], np.uint16))

    def batch(seed, g=gamma):
        data = hdl.Stack(str(tmp_path), reader=np.load, joint_transforms=[ht.to_float(), ht.reshape()],
                         image_transforms=[ht.spekle(g)])
        np.random.seed(seed)
        return next(iter(data.batches(2)))[0]

    out = batch(3)
    assert out.shape == (2, 4, 64, 64, 16)
    x = out.cpu().numpy().astype(np.float64)
    assert x.min() >= 0 and x.max() <= 1
    for b in range(2):
        d = x[b] - 0.5
        mean, std = d.mean(), d.std()
        z1 = _corr(d[..., :-1].ravel(), d[..., 1:].ravel())
        ch = max(abs(_corr(d[i].ravel(), d[j].ravel())) for i in range(4) for j in range(i))
        print('spekle item', b, 'mean', mean, 'std/gamma - 1', std / gamma - 1, 'lag-1 z', z1, 'channels', ch)
        assert abs(mean) <= 6 * gamma / np.sqrt(N) + 2.0 ** -12
        assert abs(std / gamma - 1) <= 6 / np.sqrt(2 * N) + q * q / (24 * gamma * gamma)
        assert abs(z1) <= 6 / np.sqrt(N)
        assert ch <= 6 / np.sqrt(N)
    items = _corr(x[0].ravel() - 0.5, x[1].ravel() - 0.5)
    print('spekle items', items)
    assert abs(items) <= 6 / np.sqrt(N)
    # deterministic given the numpy seed; another seed, other bits
    np.testing.assert_array_equal(bits(batch(3)), bits(out))
    assert (bits(batch(4)) != bits(out)).mean() > 0.9
    # gamma = 0: the clipped image, bit for bit
    zero = batch(3, 0)
    assert (bits(zero) == np.float16(0.5).view(np.uint16)).all()


def test_recipe_batch_trains_a_small_unet(two_stacks):
    """batches(2) of the recipe -> Unet_Constructor -> cross_entropy(pixel) ->
    backward: finite, and the same loss as from the batch built item by item."""
    data = hdl.Stack(two_stacks, reader=np.load, **recipe([18, 18, 3]))
    np.random.seed(23)
    image, mask, pwl = next(iter(data.batches(2)))
    assert image.shape == (2, 4, 18, 18, 3) and mask.shape == pwl.shape == (2, 1, 18, 18, 3)
    np.random.seed(23)
    items = [data[0], data[1]]
    by_item = [torch.cat([it[k] for it in items]) for k in range(3)]
    losses = []
    for im, m, p in ((image, mask, pwl), by_item):
        torch.manual_seed(0)
        net = Unet_Constructor(**dict(REF_KW, feature_sizes=[2, 4])).cuda().train()
        out = net(im.float())   # an fp32 model takes fp32 input, as the reference's (fp16 goes in under autocast)
        loss = hl.cross_entropy(out, m, p, method='pixel')
        loss.backward()
        assert all(torch.isfinite(q.grad).all() for q in net.parameters())
        losses.append(float(loss.detach()))
    assert np.isfinite(losses[0]) and losses[0] == losses[1]
