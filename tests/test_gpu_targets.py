"""Training targets on the GPU (csrc/targets.hip through
hcunet_amd.train_utils / hcat.train) and hcat.dataloader.RecursiveStack.

Every result is held to the reference's recorded output
(tests/golden/targets.npz) or to the numpy restatement
(tests/targets_oracle.py, itself pinned to that fixture) with np.array_equal on
the bits: tolerance zero.  That is the claim, not a measurement -- the kernels
do integer work, look float64 values up in a table the host computed with the
reference's expressions, or divide two exact integers once in IEEE float64.
Every output buffer is poisoned before its kernel runs (_lib.POISON), so an
unwritten voxel shows."""
import os
import pickle

import numpy as np
import pytest
import torch

import hcat.dataloader as hdl
import hcat.transforms as ht
from hcat.train import train_utils as htu
from hcunet_amd import _lib
from hcunet_amd import train_utils as tu
from oracle import input_oracle as io
from tests import targets_oracle as to

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'targets.npz'))
DTYPES = ['u16', 'u8']


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setattr(_lib, 'POISON', 0xFF)   # NaN in float64, -1 in the integer tables


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    return a.tobytes() == b.tobytes()   # np.array_equal on the bits (-0.0 != 0.0, NaN == NaN)


@pytest.mark.parametrize('name', DTYPES)
def test_pwl_matches_reference(name):
    got = htu.makePWL()(GOLD[name + '.labels'])
    assert np.array_equal(got, GOLD[name + '.pwl']) and same(got, GOLD[name + '.pwl'])


@pytest.mark.parametrize('name', DTYPES)
def test_center_of_mass_matches_reference(name):
    com, ids = htu.CalculateCenterOfMass()(GOLD[name + '.labels'])
    assert np.array_equal(ids, GOLD[name + '.ids']) and same(ids, GOLD[name + '.ids'])
    assert np.array_equal(com, GOLD[name + '.com']) and same(com, GOLD[name + '.com'])


@pytest.mark.parametrize('name', DTYPES)
def test_vector_to_center_matches_reference(name):
    got = htu.VectorToCenter()(GOLD[name + '.com'], GOLD[name + '.ids'], None)
    assert np.array_equal(got, GOLD[name + '.vec']) and same(got, GOLD[name + '.vec'])


@pytest.mark.parametrize('name', DTYPES)
@pytest.mark.parametrize('fill', [0xFF, 0x3F])   # 0xFF is a value of this uint8 mask: also a byte that is not
def test_colormask_to_mask_matches_reference(name, fill, monkeypatch):
    monkeypatch.setattr(_lib, 'POISON', fill)
    binary = GOLD[name + '.labels'].copy()
    mask = htu.colormask_to_mask(binary)
    assert np.array_equal(mask, GOLD[name + '.mask']) and same(mask, GOLD[name + '.mask'])
    assert same(binary, GOLD[name + '.binary'])   # in place, as the reference


def test_as_tensor_equals_numpy():
    labels = GOLD['u16.labels']
    dev = torch.from_numpy(labels.view(np.int16)).cuda()   # the same bits on the device
    pwl = htu.makePWL(as_tensor=True)(dev)
    assert pwl.is_cuda and pwl.dtype == torch.float64 and same(pwl.cpu().numpy(), GOLD['u16.pwl'])
    com, ids = htu.CalculateCenterOfMass(as_tensor=True)(dev)
    assert com.is_cuda and ids.is_cuda and ids.dtype == torch.int32
    assert same(com.cpu().numpy(), GOLD['u16.com']) and same(ids.cpu().numpy().view(np.uint32), GOLD['u16.ids'])
    vec = htu.VectorToCenter(as_tensor=True)(com, ids, None)
    assert vec.is_cuda and same(vec.cpu().numpy(), GOLD['u16.vec'])
    binary = dev.clone()
    mask = htu.colormask_to_mask(binary, as_tensor=True)
    assert mask.is_cuda and same(mask.cpu().numpy(), GOLD['u16.mask'])
    assert same(binary.cpu().numpy().view(np.uint16), GOLD['u16.binary'])


# ---------------------------------------------------------------------------
# One seeded stack that crosses what the fixture cannot: Z=2, Y=70, X=45 is
# 3 x 2 tiles of 32 x 32 per slice with ragged edges.
def random_ids():
    rng = np.random.default_rng(11)
    Z, Y, X = 2, 70, 45
    a = np.zeros((Z, Y, X), dtype=np.uint16)
    nxt = [1]

    def cell(z, ys, xs):
        a[z, ys, xs] = nxt[0]
        nxt[0] += 1
        return nxt[0] - 1

    # slice 0, by hand.  A voxel of tile (0, 0) whose nearest cells lie in tiles (1, 0) and (0, 1):
    cell(0, slice(34, 37), slice(27, 30))
    cell(0, slice(28, 31), slice(35, 38))
    # two cells near every corner (each corner voxel itself is background)
    for y, x in ((2, 1), (1, 5), (66, 2), (68, 6), (3, 41), (1, 37), (67, 42), (64, 38)):
        cell(0, slice(y, y + 2), slice(x, x + 2))
    # cells 7, 9 and 16 voxels from a lone voxel: l0 and l1 up to the last radius
    cell(0, 50, 20)
    cell(0, 50, 27)
    cell(0, 41, 20)
    cell(0, 50, 4)
    # a mean ending in exactly .5 along x, to an even and to an odd neighbour (half to even: 20 and 24)
    half_a = cell(0, 15, slice(20, 22))
    half_b = cell(0, 19, slice(23, 25))
    # two ids with the same rounded centre: the later id must be the one left there
    low = cell(0, 58, [30, 32])
    high = cell(0, 58, 31)
    # slice 1: one- to four-voxel cells on a 3 x 3 lattice, more ids than the LDS window of the moments
    sites = [(y, x) for y in range(1, Y - 2, 3) for x in range(1, X - 2, 3)]
    for k in rng.permutation(len(sites))[:300]:
        y, x = sites[k]
        cell(1, slice(y, y + rng.integers(1, 3)), slice(x, x + rng.integers(1, 3)))
    assert nxt[0] - 1 > _lib.MOMENT_LDS_IDS + 40
    for z in range(Z):
        for y, x in ((0, 0), (0, X - 1), (Y - 1, 0), (Y - 1, X - 1)):
            assert a[z, y, x] == 0
    return a, dict(half_a=half_a, half_b=half_b, low=low, high=high)


@pytest.fixture(scope='module')
def rand():
    ids, marks = random_ids()
    com, new = to.center_of_mass(ids)
    return dict(ids=ids, marks=marks, pwl=to.make_pwl(ids), com=com, new=new)


def test_random_stack_pwl(rand):
    want = rand['pwl']
    # the case holds what it was built for: both radii up to 9, and a voxel of
    # tile (0, 0) that found its two cells in two other tiles
    assert want[0, 30, 30] == to.value(4, 5) and want[0, 50, 12] == to.value(8, 8) and want[0, 45, 20] > 0
    assert {want[0, 0, 0], want[0, 69, 44]} <= set(to.value(np.arange(1, 10)[:, None], np.arange(1, 10)).ravel())
    got = htu.makePWL()(rand['ids'])
    assert np.array_equal(got, want) and same(got, want)


def test_random_stack_moments_and_center_of_mass(rand):
    ids, new, m = rand['ids'], rand['new'], rand['marks']
    n = int(new.max()) + 1
    got = tu._moments(torch.from_numpy(new.view(np.int32)).cuda(), n).cpu().numpy()
    z, y, x = np.indices(new.shape)
    want = np.stack([np.bincount(new.ravel(), weights=w.ravel(), minlength=n).astype(np.int64)
                     for w in (np.ones(new.shape), z, y, x)], axis=1)
    assert np.array_equal(got, want)
    # half to even, and the overwrite order (ids of this stack are already 0..n-1 in order)
    assert np.array_equal(new, ids)
    assert rand['com'][0, 15, 20] == m['half_a'] and rand['com'][0, 19, 24] == m['half_b']
    assert rand['com'][0, 58, 31] == m['high'] and not (rand['com'] == m['low']).any()
    com, got_ids = htu.CalculateCenterOfMass()(ids)
    assert same(got_ids, new) and same(com, rand['com'])


def test_random_stack_vector_to_center(rand):
    new, m = rand['new'], rand['marks']
    # the reference's own centre volume has lost the overwritten id: one error type
    with pytest.raises(ValueError, match=f"id {m['low']} has 0"):
        htu.VectorToCenter()(rand['com'], new, None)
    twice = rand['com'].copy()
    twice[1, 0, 0] = m['high']
    twice[0, 58, 30] = m['low']
    with pytest.raises(ValueError, match=f"id {m['high']} has 2"):
        htu.VectorToCenter()(twice, new, None)
    # a general centre volume: the first voxel of every cell
    center = np.zeros(new.shape)
    flat = new.ravel()
    first = np.unique(flat, return_index=True)[1]
    center.ravel()[first[1:]] = flat[first[1:]]
    want = to.vector_to_center(center, new)
    got = htu.VectorToCenter()(center, new, None)
    assert np.array_equal(got, want) and same(got, want)
    got16 = htu.VectorToCenter()(center.astype(np.uint16), new.astype(np.uint16), None)   # other dtypes, same result
    assert same(got16, want)


def test_random_stack_colour_form(rand):
    # the same cells as colours whose order is not the id order, uint16 with
    # high bits set in every channel: keys, ids and the scan agree with the restatement
    ids = rand['ids'].astype(np.int64)
    colour = np.stack([(ids * 40503) % 65536, (ids * 7) % 65536, (ids * 65521) % 65536], axis=-1).astype(np.uint16)
    colour[ids == 0] = 0
    want_com, want_ids = to.center_of_mass(colour)
    com, got_ids = htu.CalculateCenterOfMass()(colour)
    assert same(got_ids, want_ids) and same(com, want_com)
    assert same(htu.makePWL()(colour), rand['pwl'])
    # a stack whose first voxel is a cell: that colour is the background
    shifted = colour.copy()
    shifted[shifted.any(-1) == 0] = (9, 9, 9)
    shifted[0, 0, 0] = colour[0, 34, 27]
    want_com, want_ids = to.center_of_mass(shifted)
    com, got_ids = htu.CalculateCenterOfMass()(shifted)
    assert same(got_ids, want_ids) and same(com, want_com)


def bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def test_recursive_stack_matches_oracle(tmp_path):
    rng = np.random.default_rng(4)
    Z, Y, X = 5, 33, 20
    raw = {
        '.tif': rng.integers(0, 65536, size=(Z, Y, X, 4)).astype(np.uint16),
        '.mask.tif': (rng.random((Z, Y, X)) < 0.3).astype(np.uint8) * 255,
        '.pwl.tif': rng.integers(0, 65536, size=(Z, Y, X)).astype(np.uint16),
        '.labels.com.tif': (rng.integers(0, 40, size=(Z, Y, X)) * (rng.random((Z, Y, X)) < 0.05)).astype(np.uint8),
    }
    vec = (rng.integers(-X, X, size=(Z, Y, X, 3)) / np.array([Z, Y, X])).astype(np.float64)
    for suffix, a in raw.items():
        with open(os.path.join(tmp_path, 'vol' + suffix), 'wb') as f:
            np.save(f, a)
    with open(os.path.join(tmp_path, 'vol.labels.vector.pkl'), 'wb') as f:
        pickle.dump(vec, f)
    mean, std = [0.5, 0.4, 0.3, 0.6], [0.5, 0.25, 0.1, 0.7]
    data = hdl.RecursiveStack(str(tmp_path), image_transforms=[ht.normalize(mean, std)],
                              joint_transforms=[ht.to_float(), ht.reshape()], reader=np.load)
    assert len(data) == 1
    want = [io.network_input(raw['.tif'], mean, std), io.network_input(raw['.mask.tif']),
            io.network_input(raw['.pwl.tif']), io.network_input(raw['.labels.com.tif']), io.network_input(vec)]
    assert want[4].shape == (1, 3, X, Y, Z)
    for items in (data[0], next(iter(data.prefetch([0]))), next(iter(data.batches(1)))):
        assert len(items) == 5
        for got, w in zip(items, want):
            assert got.is_cuda and got.dtype == torch.float16 and tuple(got.shape) == w.shape
            np.testing.assert_array_equal(bits(got), w.view(np.uint16))
