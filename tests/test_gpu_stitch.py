"""The tiled stitch on the GPU (hcu_vec_label_paste in csrc/instances.hip
through hcunet_amd.instances.stitch_vec_to_cell and
hcunet_amd.segment.predict_instance_mask).

Every result is held to the numpy restatement (tests/stitch_oracle.py) on the
bits, tolerance zero: stages 1-4 are pixel_vec_to_cell's, whose bit match
tests/test_gpu_vec_to_cell.py argues, and the new pass adds integer work only
(an id table, four comparisons of floats that both sides form the same way,
an address).  Every buffer handed out by _lib.empty is poisoned first, once
with 0xFF and once with 0x3F.

Shapes: 40x36x6 cut 3x3x1 and 24x20x12 cut 2x2x2, windows of a few thousand
voxels with clipped halos on every kind of face; the network case is four
48x48x24 windows of a 64x64x24 stack."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import hcat.segment as hs
from hcunet_amd import _lib, cells, instances
from tests import stitch_oracle as so
from tests import vec_to_cell_oracle as vo
from tests.test_stitch import GEOMETRIES, INV_HALO, INV_TILE, invariance_case

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'vec_to_cell.npz'))
MANY_CENTRES = [[(5, 6, 2), (7, 27, 3), (15, 15, 2), (18, 31, 3), (24, 7, 3), (29, 22, 2), (35, 12, 3), (36, 30, 2)],
                [(4, 5, 3), (5, 15, 8), (11, 9, 9), (13, 4, 2), (17, 14, 4), (20, 6, 8), (19, 16, 10), (9, 16, 2)]]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


@pytest.fixture(autouse=True, params=[0xFF, 0x3F], ids=['poisonFF', 'poison3F'])
def poisoned(request, monkeypatch):
    monkeypatch.setattr(_lib, 'POISON', request.param)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def many(geometry, dtype):
    """(field as a host tensor of dtype, mask uint8, the restatement's result); shared, not to be written."""
    shape, tile, halo = GEOMETRIES[geometry]
    t = torch.from_numpy(so.field(shape, MANY_CENTRES[geometry], 23 + geometry).astype(np.float32)).to(dtype)
    mask = (np.random.default_rng(29 + geometry).random(shape) > 0.1).astype(np.uint8)
    want = so.stitch_field(t.float().numpy(), mask, tile, halo, sigma=1.3)
    # not vacuous: several windows give out ids, and rule (d) alone refuses some voxels
    assert sum(1 for k in want['owned'] if k) >= 2 and want['refused'] > 0
    assert 0 < (want['label'] == 0).mean() < 1
    return t, mask, want


@pytest.mark.parametrize('name', ['a', 'b'])
def test_one_window_is_pixel_vec_to_cell(name, capsys):
    vector, mask = torch.from_numpy(GOLD[name + '.vector']).cuda(), torch.from_numpy(GOLD[name + '.mask']).cuda()
    want = hs.pixel_vec_to_cell(vector, mask, label_offset=1)
    capsys.readouterr()
    for tile in [(None, None, None), tuple(vector.shape[2:]), (1000, 1000, 1000)]:
        got, centres = hs.stitch_vec_to_cell(vector, mask, tile=tile, halo=(8, 8, 8))
        assert isinstance(got, np.ndarray) and same(got, want.astype(np.int32))
        assert same(centres, GOLD[name + '.peaks'])
        assert capsys.readouterr().out == 'Predicted %d cell from runet output\n' % len(centres)
    assert same(want, vo.labels(vo.centres(GOLD[name + '.vector'][0].astype(np.float32)), GOLD[name + '.peaks'],
                                GOLD[name + '.mask'], 1))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('geometry', [0, 1])
def test_many_windows(geometry, dtype, capsys):
    t, mask, want = many(geometry, dtype)
    _, tile, halo = GEOMETRIES[geometry]
    got, centres = hs.stitch_vec_to_cell(t, mask, tile=tile, halo=halo, sigma=1.3)       # host arrays in, numpy out
    assert capsys.readouterr().out == 'Predicted %d cell from runet output\n' % len(want['centres'])
    assert same(got, want['label']) and same(centres, want['centres'])
    dev, centres = hs.stitch_vec_to_cell(t.cuda(), torch.from_numpy(mask).cuda()[None, None], tile=tile, halo=halo,
                                         sigma=1.3, as_tensor=True)
    assert dev.is_cuda and dev.dtype == torch.int32 and same(dev.cpu().numpy(), want['label'])
    assert same(centres, want['centres'])


def test_num_peaks_is_per_window():
    t, mask, want = many(0, torch.float16)
    _, tile, halo = GEOMETRIES[0]
    one = so.stitch_field(t.float().numpy(), mask, tile, halo, sigma=1.3, num_peaks=1)
    assert len(want['centres']) > len(one['centres']) >= 2
    got, centres = hs.stitch_vec_to_cell(t, mask, tile=tile, halo=halo, sigma=1.3, num_peaks=1)
    assert same(got, one['label']) and same(centres, one['centres'])


def paste(vec, mask, peaks, ids, bounds, dst, lo, n=None, dims=None, dst_dims=None):
    """hcu_vec_label_paste on device tensors; returns the code."""
    table = torch.from_numpy(np.ascontiguousarray(peaks, dtype=np.int32)).cuda()
    idt = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
    b = np.ascontiguousarray(bounds, dtype=np.float32).reshape(-1)
    X, Y, Z = dims or tuple(vec.shape[1:])
    DX, DY, DZ = dst_dims or tuple(dst.shape)
    rc = _lib.lib().hcu_vec_label_paste(
        _lib.ptr(vec), instances._VEC_CODES[vec.dtype], X * Y * Z, X, Y, Z, _lib.ptr(table), _lib.ptr(idt),
        len(ids) if n is None else n, _lib.ptr(mask), _lib.HCU_U8, b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
        _lib.ptr(dst), DX, DY, DZ, *lo, _lib.stream_handle(dst.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f16', 'bf16'])
def test_paste_abi(dtype):
    shape = (21, 18, 7)
    rng = np.random.default_rng(31)
    inf = np.inf
    # two overlapping windows: [2,15) x [0,12) x [0,7) and then [9,21) x [5,18) x [1,7)
    calls = []
    for lo, dims, bounds, peaks, ids in [
            ((2, 0, 0), (13, 12, 7), [[1, 12], [-inf, 11], [-inf, inf]],
             [[3, 3, 3], [9, 8, 2], [6, 2, 5], [11, 10, 3]], [4, 0, 9, 2]),
            ((9, 5, 1), (12, 13, 6), [[1, inf], [1, inf], [2, 5]],
             [[4, 4, 2], [8, 9, 3], [2, 10, 4]], [0, 11, 3])]:
        v = torch.from_numpy(rng.normal(0, 2.5, size=(3,) + dims).astype(np.float32)).to(dtype)
        v[2, 1, 1, 1], v[1, 2, 2, 2], v[0, 3, 3, 3], v[0, 4, 4, 4] = np.nan, np.inf, -np.inf, 1e30
        m = (rng.random(dims) > 0.15).astype(np.uint8)
        calls.append((lo, bounds, np.array(peaks), np.array(ids), v, m))
    want = np.full(shape, 7, dtype=np.int32)
    refused = 0
    for lo, bounds, peaks, ids, v, m in calls:
        refused += so.paste(want, v.float().numpy(), m, peaks, ids, lo, np.array(bounds, dtype=np.float32))
    assert refused > 0
    assert set(np.unique(want).tolist()) == {2, 3, 4, 7, 9, 11}       # every non-zero id of both calls, never an id 0
    assert (want[:2] == 7).all() and (want[15:, :5] == 7).all()        # outside both windows
    first = np.full(shape, 7, dtype=np.int32)
    so.paste(first, calls[0][4].float().numpy(), calls[0][5], calls[0][2], calls[0][3], calls[0][0],
             np.array(calls[0][1], dtype=np.float32))
    assert ((first != 7) & (want != first)).any()                      # the later call wins somewhere
    dst = torch.full(shape, 7, dtype=torch.int32, device='cuda')
    for lo, bounds, peaks, ids, v, m in calls:
        assert paste(v.cuda(), torch.from_numpy(m).cuda(), peaks, ids, bounds, dst, lo) == _lib.HCU_OK
    assert same(dst.cpu().numpy(), want)
    # more peaks than the workgroup's LDS table holds: the winner is the last one, read from global memory
    lo, bounds, peaks, ids, v, m = calls[0]
    far = np.tile(np.array([[500, 500, 500]]), (1030, 1))
    long_peaks, long_ids = np.concatenate([far, peaks]), np.concatenate([np.full(1030, 5), ids])
    want2, dst2 = np.full(shape, 7, dtype=np.int32), torch.full(shape, 7, dtype=torch.int32, device='cuda')
    so.paste(want2, v.float().numpy(), m, long_peaks, long_ids, lo, np.array(bounds, dtype=np.float32))
    assert paste(v.cuda(), torch.from_numpy(m).cuda(), long_peaks, long_ids, bounds, dst2, lo) == _lib.HCU_OK
    assert same(dst2.cpu().numpy(), want2) and same(want2, first)


def test_paste_bad_arguments_never_write():
    shape = (21, 18, 7)
    dims = (13, 12, 7)
    v = torch.zeros((3,) + dims, device='cuda')
    m = torch.ones(dims, dtype=torch.uint8, device='cuda')
    open_ = [[-np.inf, np.inf]] * 3
    dst = torch.full(shape, 7, dtype=torch.int32, device='cuda')
    peaks, ids = [[3, 3, 3]], [5]
    SHP, INV = _lib.HCU_ERR_SHAPE, _lib.HCU_ERR_INVALID
    assert paste(v, m, peaks, ids, open_, dst, (9, 0, 0)) == SHP          # past the destination's x face
    assert paste(v, m, peaks, ids, open_, dst, (0, 7, 0)) == SHP
    assert paste(v, m, peaks, ids, open_, dst, (0, 0, 1)) == SHP
    assert paste(v, m, peaks, ids, open_, dst, (-1, 0, 0)) == SHP
    assert paste(v, m, peaks, ids, open_, dst, (0, 0, 0), n=-1) == INV
    assert paste(v, m, peaks, ids, [[np.nan, 1]] * 3, dst, (0, 0, 0)) == INV
    assert paste(v, m, peaks, ids, open_, dst, (0, 0, 0), dst_dims=(21, 18, 0)) == SHP
    assert paste(v, m, peaks, ids, open_, dst, (0, 0, 0), n=0) == _lib.HCU_OK   # no peak: nothing written
    assert (dst == 7).all()
    assert paste(v, m, peaks, ids, open_, dst, (8, 6, 0)) == _lib.HCU_OK        # flush with the far corner
    got = dst.cpu().numpy()
    assert (got[8:, 6:] == 5).all() and (got[:8] == 7).all() and (got[:, :6] == 7).all()


def test_invariance_on_the_device():
    vector, mask = invariance_case()
    want = so.stitch_field(vector.astype(np.float32), mask, INV_TILE, INV_HALO, sigma=1.3)
    got, centres = hs.stitch_vec_to_cell(vector, mask, tile=INV_TILE, halo=INV_HALO, sigma=1.3)
    assert same(got, want['label']) and same(centres, want['centres'])
    whole = hs.pixel_vec_to_cell(vector, mask, sigma=1.3, label_offset=1)
    assert so.same_partition(got, whole.astype(np.int32)) and len(centres) == len(np.unique(whole)) - 1


@functools.lru_cache(maxsize=None)
def network():
    """The seeded RDCNet of test_gpu_vec_to_cell.test_rdcnet_output and its input."""
    from hcunet_amd.r_unet import RDCNet
    from oracle import inputs
    torch.manual_seed(3)
    net = RDCNet(4, 5)
    with torch.no_grad():   # vectors of a few voxels, so that votes gather
        net.transposed_conv.weight.mul_(25.0)
    return net.cuda().eval(), torch.from_numpy(inputs.make_x((1, 4, 64, 64, 24))).cuda()


@pytest.mark.parametrize('batched', [False, True], ids=['one_by_one', 'batched'])
def test_network(batched):
    net, x = network()
    shape, tile, halo = (64, 64, 24), (32, 32, None), (16, 16, 0)
    wins = so.windows(shape, tile, halo)
    assert [tuple(b - a for a, b in zip(w['lo'], w['hi'])) for w in wins] == [(48, 48, 24)] * 4
    crops = [x[(slice(None), slice(None)) + so.box(w)].contiguous() for w in wins]
    with torch.no_grad():
        outs = net(torch.cat(crops)).cpu().numpy() if batched else np.concatenate([net(c).cpu().numpy() for c in crops])
    assert outs.shape == (4, 5, 48, 48, 24)
    index = {w['lo']: k for k, w in enumerate(wins)}
    want = so.stitch(shape, tile, halo, lambda w: (outs[index[w['lo']], 2:], outs[index[w['lo']], 0] > 0.5))
    print('network: ids', len(want['centres']), 'per window', want['owned'], 'refused by (d)', want['refused'],
          'labelled', float((want['label'] != 0).mean()))
    assert len(want['centres']) >= 2
    labels, centres = hs.predict_instance_mask(net, x.cpu(), tile=tile, halo=halo,
                                               tiles_per_batch=None if batched else 1)
    assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == (1, 1) + shape
    assert same(labels[0, 0].cpu().numpy(), want['label']) and same(centres, want['centres'])


def test_network_refuses_odd_sizes_and_short_outputs():
    net, x = network()
    with pytest.raises(ValueError, match='crop the image'):
        hs.predict_instance_mask(net, torch.zeros(1, 4, 65, 64, 24, device='cuda'), tile=(32, 32, None),
                                 halo=(16, 16, 0))
    with pytest.raises(RuntimeError, match='at least 5 channels'):
        hs.predict_instance_mask(torch.nn.Identity(), x, tile=(32, 32, None), halo=(16, 16, 0))
    with pytest.raises(RuntimeError, match='at least 5 channels'):
        hs.predict_instance_mask(lambda_module(lambda t: torch.zeros(t.shape[0], 5, 8, 8, 8, device='cuda')), x,
                                 tile=(32, 32, None), halo=(16, 16, 0))


def lambda_module(fn):
    class M(torch.nn.Module):
        def forward(self, t):
            return fn(t)
    return M().eval()


def test_cell_table_of_stitched_labels():
    t, mask, want = many(0, torch.float16)
    _, tile, halo = GEOMETRIES[0]
    labels, centres = hs.stitch_vec_to_cell(t.cuda(), torch.from_numpy(mask).cuda(), tile=tile, halo=halo, sigma=1.3,
                                            as_tensor=True)
    image = torch.from_numpy(np.random.default_rng(37).random((1, 4) + tuple(labels.shape)).astype(np.float32)).cuda()
    table = cells.cell_table(image, labels)
    present = np.unique(want['label'])
    present = present[present != 0]
    assert len(present) >= 2 and present.max() <= len(centres)
    assert table.ids.dtype == torch.int32 and table.ids.cpu().numpy().tolist() == present.tolist()
    assert all(getattr(table, k).shape[0] == len(present) for k in table._fields)
