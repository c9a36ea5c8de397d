"""Instance labels from the vector field on the GPU (csrc/instances.hip
through hcunet_amd.instances / hcat.segment).

Every result is held to the numpy restatement (tests/vec_to_cell_oracle.py,
itself pinned to the reference's recorded outputs and to scipy) or to the
fixture (tests/golden/vec_to_cell.npz) on the bits: tolerance zero.  The votes
are integer atomics; the normalisation is one IEEE division of exact integers;
the Gaussian multiplies and adds in float64 in scipy's order without
contraction; the distances multiply, add and take a correctly rounded square
root in fp32 as numpy does.  Every output buffer is poisoned before its kernel
runs, once with 0xFF (NaN) and once with 0x3F (about 0.75 / a large positive
integer), so an unwritten or stale word shows.

Shapes: 64x44x6 has two axes longer than the 41 taps and one shorter than the
radius; 48x20x6 an axis between the radius and the kernel length and a single
peak; 23x45x5 odd sizes; each spans several tiles of at least one pass."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import hcat.segment as hs
from hcunet_amd import _lib, instances
from tests import vec_to_cell_oracle as vo

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'vec_to_cell.npz'))
CASES = ['a', 'b', 'c']


@pytest.fixture(autouse=True, params=[0xFF, 0x3F], ids=['poisonFF', 'poison3F'])
def poisoned(request, monkeypatch):
    monkeypatch.setattr(_lib, 'POISON', request.param)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return a.tobytes() == b.tobytes()


def field(shape, centres, seed):
    """fp16 [1,3,X,Y,Z]: every voxel points at its nearest centre, plus noise."""
    grid = np.indices(shape).astype(np.float64)
    cen = np.asarray(centres, dtype=np.float64)
    d = ((grid[None] - cen[:, :, None, None, None]) ** 2).sum(1)
    to_centre = np.moveaxis(cen[np.argmin(d, axis=0)], -1, 0) - grid
    v = to_centre[::-1] + np.random.default_rng(seed).normal(0, 0.6, size=(3,) + tuple(shape))
    return v.astype(np.float32).astype(np.float16)[None]


@functools.lru_cache(maxsize=None)
def case(name):
    """(vector fp16 [1,3,X,Y,Z], mask, the restatement's results); shared, not to be written."""
    if name == 'c':
        vector = field((48, 20, 6), [(25, 9, 3)], 2)
        mask = np.ones((1, 1, 48, 20, 6), dtype=np.float32)
    else:
        vector, mask = GOLD[name + '.vector'], GOLD[name + '.mask']
    want = vo.pixel_vec_to_cell(vector.astype(np.float32), mask)
    if name == 'c':
        assert len(want['peaks']) == 1
    return vector, mask, want


def as_dtype(vector16, dtype):
    """The field as a host tensor of `dtype` and the fp32 array it reads as."""
    t = torch.from_numpy(vector16.astype(np.float32)).to(dtype)
    return t, t.float().numpy()


@pytest.mark.parametrize('strided', ['dense', 'slice', 'gap', 'copy'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('name', CASES)
def test_counts_and_hist(name, dtype, strided):
    vector, _, _ = case(name)
    t, v32 = as_dtype(vector, dtype)
    c = vo.centres(v32[0])
    want = vo.vote_counts(c)
    dev = t.cuda()
    if strided == 'slice':   # the channel slice of a five-channel network output, read in place
        out = torch.full((1, 5) + tuple(t.shape[2:]), 7.0, dtype=dtype, device='cuda')
        out[:, 2:] = dev
        dev = out[:, 2:]
        assert dev.storage_offset() > 0
    elif strided == 'gap':   # channel planes with other data between them: read in place too
        X = t.shape[2]
        out = torch.full((1, 5, X + 2) + tuple(t.shape[3:]), 7.0, dtype=dtype, device='cuda')
        out[:, 2:, 1:X + 1] = dev
        dev = out[:, 2:, 1:X + 1]
        assert not dev.is_contiguous()
    elif strided == 'copy':  # an axis reversed: no plane layout, copied
        dev = dev.flip(4).flip(4).transpose(3, 4).contiguous().transpose(3, 4)
        assert not dev.is_contiguous()
    got = instances.vote_counts(dev[0])
    assert got.dtype == torch.int32 and same(got.cpu().numpy(), want.astype(np.int32))
    if dtype == torch.float32 and name != 'c':
        assert same(got.cpu().numpy(), GOLD[name + '.counts'])
    # hist3d takes the points themselves: a numpy array gives a numpy array, a tensor a device tensor
    hist = hs.hist3d(c)
    assert isinstance(hist, np.ndarray) and same(hist, vo.hist3d(c))
    if dtype == torch.float32 and name != 'c':
        assert same(hist, GOLD[name + '.hist'])
    hist_t = hs.hist3d(torch.from_numpy(c).cuda())
    assert hist_t.is_cuda and hist_t.dtype == torch.float64 and same(hist_t.cpu().numpy(), hist)


def test_votes_skip_nonfinite_and_outside():
    X, Y, Z = 23, 45, 5
    rng = np.random.default_rng(5)
    v = rng.normal(0, 1.5, size=(3, X, Y, Z)).astype(np.float32)
    v[0, 3, 4, 2], v[1, 5, 6, 1], v[2, 7, 8, 3] = np.nan, np.inf, -np.inf
    v[:, 9, 9, 2] = np.nan
    # past every face, by a lot and by a hair (channel 2 moves x, 1 moves y, 0 moves z)
    v[2, 0, 0, 0], v[2, X - 1, 1, 0], v[2, 2, 2, 0], v[2, 3, 3, 0] = -0.25, 1.0, -1e6, 1e6
    v[1, 1, 0, 1], v[1, 1, Y - 1, 1], v[1, 4, 4, 0], v[1, 5, 5, 0] = -1e-3, 1.0, -3e9, 3e9
    v[0, 2, 1, 0], v[0, 2, 1, Z - 1], v[0, 6, 6, 0], v[0, 7, 7, 0] = -1.0, 1.0, -1e30, 1e30
    v[2, X - 1, 2, 1], v[1, 2, Y - 1, 1], v[0, 2, 3, Z - 1] = 0.96875, 0.96875, 0.96875   # the last voxel, inside
    c = vo.centres(v)
    want = vo.vote_counts(c)
    assert want.sum() < X * Y * Z - 12
    got = instances.vote_counts(torch.from_numpy(v).cuda())
    assert same(got.cpu().numpy(), want.astype(np.int32))
    assert same(hs.hist3d(c), vo.hist3d(c))
    # the label pass recomputes c: a NaN distance never wins, +-Inf is farther than 100000
    peaks = np.array([[4, 4, 2], [15, 30, 3]])
    mask = np.ones((X, Y, Z), dtype=np.uint8)
    lab = hs.pixel_vec_to_cell(torch.from_numpy(v[None]).cuda(), mask, peaks=peaks, label_offset=1)
    assert same(lab, vo.labels(c, peaks, mask, label_offset=1))
    assert lab[9, 9, 2] == 0 and lab[3, 4, 2] == 0 and lab[5, 6, 1] == 0 and lab[7, 8, 3] == 0


@pytest.mark.parametrize('name', CASES)
def test_smoothed_votes_bitwise(name):
    vector, _, want = case(name)
    got = instances.smoothed_votes(torch.from_numpy(vector[0]).cuda())
    diff = np.abs(got.cpu().numpy() - want['smooth']).max()
    print('smoothed votes', name, 'max abs difference', diff)
    assert same(got.cpu().numpy(), want['smooth'])
    if name != 'c':
        assert same(got.cpu().numpy(), GOLD[name + '.smooth'])


@pytest.mark.parametrize('shape', [(64, 44, 6), (48, 20, 6), (23, 45, 5), (3, 70, 1), (130, 2, 45)])
def test_gaussian_alone_bitwise(shape):
    a = np.random.default_rng(11).random(shape)
    for sigma in (5, 1.3):
        got = instances.smooth_f64(torch.from_numpy(a).cuda(), sigma).cpu().numpy()
        want = vo.gaussian(a, sigma)
        print('gaussian', shape, sigma, 'max abs difference', np.abs(got - want).max())
        assert same(got, want)


@pytest.mark.parametrize('name', CASES)
def test_peak_candidates(name):
    _, _, want = case(name)
    h = torch.from_numpy(want['smooth']).cuda()
    idx, val = instances.peak_candidates(h)
    lin, values = vo.peak_candidates(want['smooth'])
    order = np.argsort(idx)
    assert same(idx[order], lin.astype(np.int64)) and same(val[order], values)
    assert same(instances.select_peaks(idx, val, h.shape), want['peaks'])


def test_peak_candidates_list_too_small():
    a = np.random.default_rng(13).random((23, 45, 5))
    a[5:8, 5:8, 1:4] = 2.0                 # a plateau: every voxel of it equals its neighbourhood's maximum
    a[0, :, :] = 3.0                       # the outermost layer never counts
    lin, values = vo.peak_candidates(a)
    assert len(lin) > 40
    h = torch.from_numpy(a).cuda()
    idx, val = instances.peak_candidates(h)
    order = np.argsort(idx)
    assert same(idx[order], lin.astype(np.int64)) and same(val[order], values)
    # room for 8: the error code and the number found, never a silent truncation
    index = _lib.empty((8,), torch.int32, h.device)
    value = _lib.empty((8,), torch.float64, h.device)
    state = _lib.empty((2,), torch.int64, h.device)
    found = ctypes.c_int(0)
    rc = _lib.lib().hcu_peak_candidates(_lib.ptr(h), 23, 45, 5, _lib.ptr(index), _lib.ptr(value), 8, _lib.ptr(state),
                                        ctypes.byref(found), _lib.stream_handle(h.device))
    assert rc == _lib.HCU_ERR_WORKSPACE and found.value == len(lin)
    assert set(index.cpu().numpy().tolist()) <= set(lin.tolist())        # the eight slots hold candidates
    with pytest.raises(RuntimeError, match='candidates'):
        instances.peak_candidates(h, capacity=8, grow=False)
    idx, _ = instances.peak_candidates(h, capacity=8)                    # grown to what was found
    assert same(np.sort(idx), lin.astype(np.int64))


@pytest.mark.parametrize('n', [0, 1, 3, 100])
def test_labels_for_given_peaks(n):
    vector, mask, _ = case('b')
    shape = vector.shape[2:]
    rng = np.random.default_rng(17 + n)
    peaks = np.stack([rng.integers(0, s, size=n) for s in shape], axis=1).astype(np.int64).reshape(n, 3)
    if n == 100:
        peaks[99] = (6, 9, 2)   # the last peak on the field's first centre: it has to win there
        assert not (peaks[:99] == peaks[99]).all(1).any()
    c = vo.centres(vector[0].astype(np.float32))
    for offset in (0, 1):
        got = hs.pixel_vec_to_cell(torch.from_numpy(vector).cuda(), torch.from_numpy(mask).cuda(), peaks=peaks,
                                   label_offset=offset)
        assert got.dtype == np.float64 and same(got, vo.labels(c, peaks, mask, offset))
    if n == 0:
        assert not got.any()
    if n == 100:
        assert (got == 100).sum() > 100


def test_label_ties_and_far_peaks():
    shape = (9, 6, 5)
    zero = torch.zeros((1, 3) + shape, device='cuda')
    ones = torch.ones(shape, dtype=torch.bool, device='cuda')
    peaks = np.array([[6, 3, 2], [2, 3, 2]])
    got = hs.pixel_vec_to_cell(zero, ones, peaks=peaks, label_offset=1)
    c = vo.centres(np.zeros((3,) + shape, dtype=np.float32))
    assert same(got, vo.labels(c, peaks, None, 1))
    assert (got[4] == 1).all() and (got[:4] == 2).all() and (got[5:] == 1).all()   # the plane x = 4: the earlier peak
    # the reference's numbering: the first peak's voxels read 0, as the background does
    got0 = hs.pixel_vec_to_cell(zero, ones, peaks=peaks)
    assert (got0[4:] == 0).all() and (got0[:4] == 1).all()
    # farther than 100000: nothing wins, the label stays 0
    far = np.array([[200000, 3, 2], [2, -150000, 2]])
    gotf = hs.pixel_vec_to_cell(zero, ones, peaks=far, label_offset=1)
    assert same(gotf, vo.labels(c, far, None, 1)) and not gotf.any()
    near = np.array([[99990, 0, 0], [2, 3, 2]])     # the first is within 100000 of x >= 0 only just
    gotn = hs.pixel_vec_to_cell(zero, ones, peaks=near, label_offset=1)
    assert same(gotn, vo.labels(c, near, None, 1)) and (gotn == 2).all()


@pytest.mark.parametrize('kind', ['bool', 'uint8', 'f32', 'f16', 'bf16', 'f64', '5d'])
def test_mask_dtypes(kind):
    vector, _, want = case('b')
    shape = vector.shape[2:]
    rng = np.random.default_rng(19)
    levels = np.array([0.0, 0.1, 0.19999999, 0.2, 0.2000001, 0.25, 1.0])
    m = levels[rng.integers(0, len(levels), size=shape)]
    mask = {'bool': lambda: torch.from_numpy(m > 0.5), 'uint8': lambda: torch.from_numpy((m * 4).astype(np.uint8)),
            'f32': lambda: torch.from_numpy(m.astype(np.float32)), 'f16': lambda: torch.from_numpy(m).half(),
            'bf16': lambda: torch.from_numpy(m).bfloat16(), 'f64': lambda: torch.from_numpy(m),
            '5d': lambda: torch.from_numpy(m.astype(np.float32))[None, None]}[kind]()
    host = mask.float().numpy()                      # float(mask), as the reference compares it
    c = vo.centres(vector[0].astype(np.float32))
    expect = vo.labels(c, want['peaks'], host, 1)
    assert 0 < (expect == 0).mean() < 1
    for where in ('cpu', 'cuda'):
        got = hs.pixel_vec_to_cell(torch.from_numpy(vector).cuda(), mask.to(where), peaks=want['peaks'], label_offset=1)
        assert same(got, expect)


@pytest.mark.parametrize('name', CASES)
def test_end_to_end(name, capsys):
    vector, mask, want = case(name)
    gold = want['label'] if name == 'c' else GOLD[name + '.label']
    assert same(want['label'], gold)
    # host arrays in, a numpy array out, as the reference
    got = hs.pixel_vec_to_cell(torch.from_numpy(vector), torch.from_numpy(mask))
    assert isinstance(got, np.ndarray) and same(got, gold)
    assert capsys.readouterr().out == 'Predicted %d cell from runet output\n' % len(want['peaks'])
    # device tensors in; as_tensor: a device float64 tensor with the same bits
    dv, dm = torch.from_numpy(vector).cuda(), torch.from_numpy(mask).cuda()
    assert same(hs.pixel_vec_to_cell(dv, dm), gold)
    t = hs.pixel_vec_to_cell(dv, dm, as_tensor=True)
    assert t.is_cuda and t.dtype == torch.float64 and same(t.cpu().numpy(), gold)
    # the recorded peaks handed in
    assert same(hs.pixel_vec_to_cell(dv, dm, peaks=want['peaks']), gold)
    assert same(hs.pixel_vec_to_cell(dv.float(), dm, label_offset=1), vo.labels(
        vo.centres(vector[0].astype(np.float32)), want['peaks'], mask, 1))


def test_rdcnet_output():
    from hcunet_amd.r_unet import RDCNet
    from oracle import inputs
    torch.manual_seed(3)
    net = RDCNet(4, 5)
    with torch.no_grad():   # vectors of a few voxels, so that votes gather
        net.transposed_conv.weight.mul_(25.0)
    net = net.cuda().eval()
    x = torch.from_numpy(inputs.make_x((1, 4, 64, 64, 24))).cuda()
    with torch.no_grad():
        out = net(x)
    assert tuple(out.shape) == (1, 5, 64, 64, 24) and out.dtype == torch.float32
    got = hs.pixel_vec_to_cell(out[:, 2:], out[0, 0] > 0.5)
    host = out.cpu().numpy()
    want = vo.pixel_vec_to_cell(host[:, 2:], host[0, 0] > 0.5)
    print('rdcnet: max count', int(want['counts'].max()), 'peaks', len(want['peaks']),
          'masked', float((host[0, 0] <= 0.5).mean()))
    assert want['counts'].max() > 1
    assert same(got, want['label'])
    sm = instances.smoothed_votes(out[0, 2:])
    assert same(sm.cpu().numpy(), want['smooth'])
