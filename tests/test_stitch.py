"""CPU: the tiled stitch without a device.  The window geometry of
hcunet_amd.instances.windows, the numpy restatement of the stitching rule
(tests/stitch_oracle.py) against the single-volume restatement it is built on,
the rule's invariance on a field whose cells fit their windows, the host
helpers of the paste pass, and the entry point's refusal of bad arguments
before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hcat.segment
from hcunet_amd import _lib, instances, segment
from tests import stitch_oracle as so
from tests import vec_to_cell_oracle as vo

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'vec_to_cell.npz'))
GEOMETRIES = [((40, 36, 6), (16, 16, None), (8, 8, 0)), ((24, 20, 12), (12, 10, 6), (4, 4, 2))]

# The invariance layout, (40, 36, 6) cut by tile (16, 16, None), halo (8, 8, 0): cores end at x, y = 16, 32 and
# interior window faces lie at 8 and 24.  Every centre is 4 voxels from the nearest of those and from the
# volume's faces in x and y, the centres are at least 11.3 apart, and a cell is the ball of radius 4 around
# its centre (the mask), below the halo of 8.
INV_SHAPE, INV_TILE, INV_HALO = GEOMETRIES[0]
INV_CENTRES = [(4, 4, 2), (4, 20, 3), (12, 12, 2), (12, 28, 3), (20, 4, 3), (20, 20, 2), (28, 12, 3), (28, 28, 2),
               (36, 4, 2), (36, 20, 3)]
INV_RADIUS = 4


def invariance_case():
    """(vector fp16 [1,3,X,Y,Z] noise-free, mask uint8 [X,Y,Z])."""
    vector = so.field(INV_SHAPE, INV_CENTRES, 0, noise=0)
    grid = np.indices(INV_SHAPE)
    mask = np.zeros(INV_SHAPE, dtype=np.uint8)
    for c in INV_CENTRES:
        mask |= (sum((grid[a] - c[a]) ** 2 for a in range(3)) <= INV_RADIUS ** 2).astype(np.uint8)
    return vector, mask


@pytest.mark.parametrize('shape,tile,halo', GEOMETRIES)
def test_windows(shape, tile, halo):
    wins = instances.windows(shape, tile, halo)
    assert wins == so.windows(shape, tile, halo)
    covered = np.zeros(shape, dtype=np.int32)
    for w in wins:
        covered[tuple(slice(a, b) for a, b in zip(w['core_lo'], w['core_hi']))] += 1
        for a in range(3):
            assert 0 <= w['lo'][a] <= w['core_lo'][a] < w['core_hi'][a] <= w['hi'][a] <= shape[a]
            h = halo[a]
            assert w['lo'][a] == max(w['core_lo'][a] - h, 0) and w['hi'][a] == min(w['core_hi'][a] + h, shape[a])
            assert all(v % 2 == 0 for v in (w['lo'][a], w['hi'][a], w['core_lo'][a], w['core_hi'][a]))   # even in, even out
    assert (covered == 1).all()                                   # the cores partition the volume
    keys = [w['core_lo'] for w in wins]
    assert keys == sorted(keys)                                   # x slowest, z fastest
    n = [-(-s // (s if t is None else t)) for s, t in zip(shape, tile)]
    assert len(wins) == n[0] * n[1] * n[2]
    assert wins[n[2] * n[1]]['core_lo'] == (tile[0], 0, 0)        # the next x core comes after all of y and z


def test_windows_whole_axis_and_errors():
    one = instances.windows((9, 7, 5), (None, None, None), (3, 3, 3))
    assert one == [dict(core_lo=(0, 0, 0), core_hi=(9, 7, 5), lo=(0, 0, 0), hi=(9, 7, 5))]
    assert instances.windows((9, 7, 5), (100, 100, 100), (0, 0, 0)) == one
    odd = instances.windows((9, 7, 5), (4, None, None), (1, 0, 0))
    assert [(w['core_lo'][0], w['core_hi'][0], w['lo'][0], w['hi'][0]) for w in odd] == [(0, 4, 0, 5), (4, 8, 3, 9),
                                                                                        (8, 9, 7, 9)]
    for tile, halo in [((0, 4, 4), (0, 0, 0)), ((4, -2, 4), (0, 0, 0)), ((4, 4, 4), (0, -1, 0))]:
        with pytest.raises(ValueError):
            instances.windows((9, 7, 5), tile, halo)
    with pytest.raises(ValueError):
        instances.windows((9, 7), (4, 4), (0, 0))


def test_bounds_and_ownership():
    shape = (40, 36, 6)
    wins = instances.windows(shape, (16, 16, None), (8, 8, 0))
    for w in wins:
        assert np.array_equal(instances.vote_bounds(w, shape).reshape(3, 2), so.vote_bounds(w, shape))
    mid = wins[4]     # core [16,32) x [16,32), window [8,40) x [8,36): x's upper face and y's are the volume's
    assert mid['lo'] == (8, 8, 0) and mid['hi'] == (40, 36, 6)
    assert instances.vote_bounds(mid, shape).tolist() == [1.0, np.inf, 1.0, np.inf, -np.inf, np.inf]
    assert instances.vote_bounds(wins[0], shape).tolist() == [-np.inf, 23.0, -np.inf, 23.0, -np.inf, np.inf]
    # window-local peaks of `mid`: lo + peak inside the core [16,32) x [16,32) x [0,6)
    peaks = np.array([[8, 8, 2], [7, 8, 2], [23, 23, 5], [24, 23, 0], [10, 24, 3]])
    ids, centres = instances.owned_ids(peaks, mid, 5)
    assert ids.dtype == np.int32 and ids.tolist() == [5, 0, 6, 0, 0]
    assert centres.dtype == np.int64 and centres.tolist() == [[16, 16, 2], [31, 31, 5]]


@pytest.mark.parametrize('name', ['a', 'b'])
def test_one_window_is_pixel_vec_to_cell(name):
    vector, mask = GOLD[name + '.vector'].astype(np.float32), GOLD[name + '.mask']
    want = vo.pixel_vec_to_cell(vector, mask, label_offset=1)
    shape = vector.shape[2:]
    for tile in [(None, None, None), (1000, 1000, 1000), shape]:
        got = so.stitch_field(vector, mask, tile, (8, 8, 8))
        assert got['label'].dtype == np.int32 and np.array_equal(got['label'], want['label'].astype(np.int32))
        assert np.array_equal(got['centres'], want['peaks']) and got['owned'] == [len(want['peaks'])]
        assert got['refused'] == 0


def test_invariance_of_the_rule():
    vector, mask = invariance_case()
    v32 = vector.astype(np.float32)
    whole = vo.pixel_vec_to_cell(v32, mask, sigma=1.3, label_offset=1)['label'].astype(np.int32)
    tiled = so.stitch_field(v32, mask, INV_TILE, INV_HALO, sigma=1.3)
    n = len(INV_CENTRES)
    assert len(np.unique(whole)) == n + 1                        # every cell, and the background
    assert sorted(np.unique(tiled['label']).tolist()) == list(range(n + 1)) and len(tiled['centres']) == n
    assert so.same_partition(tiled['label'], whole)              # 100 %: every cell matched, voxel for voxel
    assert (tiled['label'] != 0).sum() == (mask != 0).sum()
    assert sum(1 for k in tiled['owned'] if k) >= 4
    # a centre is where its id's cell is: within the peak's one voxel of max_filter(size=2)
    for g, c in enumerate(tiled['centres'], 1):
        near = np.abs(np.asarray(INV_CENTRES) - c).max(axis=1) <= 1
        assert near.sum() == 1 and tiled['label'][tuple(np.asarray(INV_CENTRES)[near][0])] == g


def test_same_partition_tells_apart():
    a = np.array([0, 1, 1, 2, 2, 0])
    assert so.same_partition(a, np.array([0, 5, 5, 3, 3, 0]))
    assert not so.same_partition(a, np.array([0, 5, 5, 5, 5, 0]))       # merged
    assert not so.same_partition(a, np.array([0, 5, 4, 3, 3, 0]))       # split
    assert not so.same_partition(a, np.array([0, 5, 5, 3, 3, 3]))       # background painted
    assert not so.same_partition(a, np.array([0, 5, 5, 0, 0, 0]))       # a cell lost


_VP = ctypes.c_void_p


def test_paste_rejects_bad_arguments():
    L = _lib.lib()
    p = _VP(4096)   # never dereferenced: every call below fails its host checks
    F32, U8 = _lib.HCU_F32, _lib.HCU_U8
    INV, SHP, UNS = _lib.HCU_ERR_INVALID, _lib.HCU_ERR_SHAPE, _lib.HCU_ERR_UNSUPPORTED
    inf = float('inf')
    ok = (ctypes.c_float * 6)(-inf, inf, -inf, inf, -inf, inf)
    nan = (ctypes.c_float * 6)(-inf, inf, float('nan'), inf, -inf, inf)
    big = (1 << 11, 1 << 10, 1 << 10)   # 2^31 voxels

    def call(vec=p, dtype=F32, cs=512, win=(8, 8, 8), peaks=p, ids=p, n=1, mask=p, mdt=U8, bounds=ok, dst=p,
             dims=(16, 16, 16), org=(0, 0, 0)):
        return L.hcu_vec_label_paste(vec, dtype, cs, *win, peaks, ids, n, mask, mdt, bounds, dst, *dims, *org, None)

    assert call(vec=None) == INV and call(dst=None) == INV and call(bounds=None) == INV
    assert call(peaks=None) == INV and call(ids=None) == INV and call(n=-1) == INV
    assert call(dtype=_lib.HCU_F64) == INV and call(dtype=_lib.HCU_U16) == INV
    assert call(mdt=_lib.HCU_I32) == INV and call(cs=511) == INV and call(bounds=nan) == INV
    assert 'vec_label_paste' in _lib.last_error()
    assert call(win=(8, 0, 8)) == SHP and call(dims=(16, 16, 0)) == SHP
    assert call(org=(9, 0, 0)) == SHP and call(org=(0, -1, 0)) == SHP and call(org=(0, 0, 1 << 30)) == SHP
    assert call(dims=(8, 8, 7)) == SHP
    assert call(cs=1 << 31, win=big, dims=big) == UNS and call(dims=big) == UNS
    assert call(n=0, peaks=None, ids=None) == _lib.HCU_OK       # no peak: nothing to launch


def test_namespace_and_host_side_errors():
    assert hcat.segment.stitch_vec_to_cell is instances.stitch_vec_to_cell
    assert hcat.segment.predict_instance_mask is segment.predict_instance_mask
    mask = torch.ones(4, 6, 6)
    kw = dict(tile=(2, 2, 2), halo=(0, 0, 0))
    with pytest.raises(ValueError, match='batch of 2'):
        instances.stitch_vec_to_cell(torch.zeros(2, 3, 4, 6, 6), mask, **kw)
    with pytest.raises(ValueError):
        instances.stitch_vec_to_cell(torch.zeros(1, 3, 4, 6, 6), torch.ones(4, 6, 7), **kw)
    with pytest.raises(TypeError):
        instances.stitch_vec_to_cell(torch.zeros(1, 3, 4, 6, 6), mask.long(), **kw)
    with pytest.raises(ValueError):
        instances.stitch_vec_to_cell(torch.zeros(1, 3, 4, 6, 6), mask, tile=(0, 2, 2), halo=(0, 0, 0))
    with pytest.raises(TypeError):
        instances.stitch_vec_to_cell(torch.zeros(1, 3, 4, 6, 6), mask)                       # tile and halo are required
    # odd sizes are refused before anything touches a device
    for image, tile, halo in [(torch.zeros(1, 4, 65, 64, 24), (32, 32, None), (16, 16, 0)),
                              (torch.zeros(1, 4, 64, 64, 24), (32, 31, None), (16, 16, 0)),
                              (torch.zeros(1, 4, 64, 64, 24), (32, 32, None), (16, 16, 1))]:
        with pytest.raises(ValueError, match=r'crop the image'):
            segment.predict_instance_mask(None, image, tile=tile, halo=halo)
    with pytest.raises(ValueError):
        segment.predict_instance_mask(None, torch.zeros(2, 4, 64, 64, 24))
