"""CPU: the cell tables' numpy restatement (tests/cells_oracle.py) against what
the reference's own HairCell / generate_cell_objects reported for the fixture
(tests/golden/cells.npz, written by tests/golden/make_cells_golden.py), the
host HairCell constructor against the same cells, the argument checks and the
re-exports.  No kernel is launched.

Exact: ids, boxes, centres, is_bad, num_samples, the volume's bits and the
median's value (-0.0 == 0.0, NaN equal to NaN).  The reference's mean and std
are float32 sums in numpy's pairwise order, the restatement's are the exactly
rounded float64 ones, so they are held to the summation's own bound (u = 2^-24,
D = 32 + ceil(log2 n): no path through numpy's 8 accumulators, 128-element
blocks and their halving is deeper than D additions):
    |mean32 - mean| <= (D + 1) u mean(|g|)
    |std32  - std | <= (D + 8) u std + u |mean|
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import cells_oracle as co

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'cells.npz'))
CASES = ['a', 'b', 'c']
NAMES = ['dapi', 'gfp', 'myo7a', 'actin']
STAT_CHANNEL = [0, 1, 2, 3, 1]   # the fixture's five entries: signal_stats x4, then gfp_stats


@functools.lru_cache(maxsize=None)
def case(name):
    """(image fp32 [1,4,X,Y,Z], labels int64 [X,Y,Z], the restatement's tables); shared, not to be written."""
    image = GOLD[name + '.image'].astype(np.float32)
    labels = GOLD[name + '.labels']
    return image, labels, co.cell_table(image, labels)


def mean_abs(image, labels, table):
    """float64 [n,C]: mean(|g|) of the mapped values of every cell and channel (0 for a bad cell)."""
    out = np.zeros(table['mean'].shape)
    for i, id in enumerate(table['ids']):
        x0, y0, z0, x1, y1, z1 = table['boxes'][i]
        m = (labels == id)[x0:x1, y0:y1, z0:z1]
        if m.sum() <= 1:
            continue
        for c in range(out.shape[1]):
            g = image[0, c, x0:x1, y0:y1, z0:z1][m]
            if table['box_min'][i] < 0:
                g = g * np.float32(0.5) + np.float32(0.5)
            out[i, c] = np.abs(g.astype(np.float64)).mean()
    return out


def check_float32_stats(got_mean, got_std, table, mabs, slack_ulps=0):
    """got_mean / got_std float32 [n,5] against the restatement's float64 tables by the bounds above
    (slack_ulps: float32 ulps of the value added to each bound)."""
    checked, used_mean, used_std = 0, 0.0, 0.0
    for i in range(len(table['ids'])):
        n = int(table['count'][i])
        for j, c in enumerate(STAT_CHANNEL):
            mean, std = table['mean'][i, c], table['std'][i, c]
            if np.isnan(mean):
                assert np.isnan(got_mean[i, j]) and np.isnan(got_std[i, j])
                continue
            em = abs(float(got_mean[i, j]) - mean)
            es = abs(float(got_std[i, j]) - std)
            bm = co.mean_bound(n, mabs[i, c]) + slack_ulps * float(np.spacing(np.float32(abs(mean))))
            bs = co.std_bound(n, std, mean) + slack_ulps * float(np.spacing(np.float32(std)))
            assert em <= bm, ('mean', i, j, n, em, bm)
            assert es <= bs, ('std', i, j, n, es, bs)
            used_mean, used_std = max(used_mean, em / bm), max(used_std, es / bs if bs else 0.0)
            checked += 1
    print('float32 statistics: entries', checked, 'largest share of the bound used: mean', used_mean, 'std', used_std)
    return checked


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_reference(name):
    image, labels, t = case(name)
    chunk = GOLD[name + '.chunk']
    assert np.array_equal(t['ids'], GOLD[name + '.unique_id'])
    assert np.array_equal(t['boxes'], GOLD[name + '.image_coords'])
    assert np.array_equal(co.centres(t['boxes'], chunk[0], chunk[1]), GOLD[name + '.center'])
    assert np.array_equal(t['count'] <= 1, GOLD[name + '.is_bad'])
    vol = co.volumes(t['boxes'], t['plane_count'])
    assert vol.tobytes() == GOLD[name + '.volume'].tobytes()
    num = GOLD[name + '.num_samples']
    good = ~GOLD[name + '.is_bad']
    assert (num[~good] == -1).all() and (num[good] == t['count'][good, None]).all()
    stats = GOLD[name + '.stats']
    med = co.medians(t['median'])[:, STAT_CHANNEL]
    np.testing.assert_array_equal(med, stats[:, :, 2])     # by value: -0.0 == 0.0, NaN == NaN
    checked = check_float32_stats(stats[:, :, 0], stats[:, :, 1], t, mean_abs(image, labels, t))
    assert checked >= 5 * good.sum() - 1     # case c: one channel of one cell holds a NaN


@pytest.mark.parametrize('name', CASES)
def test_host_haircell_reproduces_reference(name):
    from hcat.haircell import HairCell
    image, labels, t = case(name)
    chunk = GOLD[name + '.chunk']
    centre = co.centres(t['boxes'], chunk[0], chunk[1])
    for i, id in enumerate(t['ids']):
        if name == 'b' and i % 16 not in (4, 5, 6):     # 264 like cubes: the planted ones and a sample
            continue
        x0, y0, z0, x1, y1, z1 = t['boxes'][i]
        cell = HairCell(image_coords=list(t['boxes'][i]), center=list(centre[i]),
                        image=torch.from_numpy(image)[:, :, x0:x1, y0:y1, z0:z1],
                        mask=(labels == id)[x0:x1, y0:y1, z0:z1], id=id)
        assert cell.unique_id == id and cell.type is None and cell.distance_from_apex == []
        assert cell.is_bad == GOLD[name + '.is_bad'][i]
        assert isinstance(cell.volume, int) == GOLD[name + '.volume_is_int'][i]
        assert np.float64(cell.volume).tobytes() == GOLD[name + '.volume'][i].tobytes()
        assert list(cell.signal_stats) == NAMES
        for j, d in enumerate([cell.signal_stats[k] for k in NAMES] + [cell.gfp_stats]):
            want = GOLD[name + '.stats'][i, j]
            if cell.is_bad:
                assert list(d) == ['mean', 'std', 'median'] and all(np.isnan(v) for v in d.values())
                assert tuple(cell.unique_mask.shape) == (10,)
                continue
            assert list(d) == ['mean', 'std', 'median', 'num_samples']
            assert d['num_samples'] == (GOLD[name + '.num_samples'][i, j],)
            got = np.asarray([d['mean'], d['std'], d['median']])
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got, want)       # the same numpy calls on the same values


def test_haircell_from_table_row():
    from hcunet_amd.haircell import HairCell
    image, labels, t = case('a')
    ids = list(t['ids'])
    for id in (3, 22, 21, 300):
        i = ids.index(id)
        cell = HairCell.from_table(list(t['boxes'][i]), [1.0, 2.0, 3.0], id, t['count'][i], t['plane_count'][i],
                                   t['mean'][i], t['std'][i], t['median'][i])
        assert cell.is_bad == GOLD['a.is_bad'][i] and cell.center == [1.0, 2.0, 3.0]
        assert isinstance(cell.volume, int) == GOLD['a.volume_is_int'][i]
        assert np.float64(cell.volume).tobytes() == GOLD['a.volume'][i].tobytes()
        if cell.is_bad:
            assert list(cell.gfp_stats) == ['mean', 'std', 'median'] and np.isnan(cell.gfp_stats['median'])
            continue
        d = cell.signal_stats['myo7a']
        assert d['num_samples'] == (int(t['count'][i]),) and type(d['mean']) is np.float32
        assert type(d['median']) is np.float32 and d['median'] == GOLD['a.stats'][i, 2, 2]
        assert d['mean'] == np.float32(t['mean'][i, 2]) and d['std'] == np.float32(t['std'][i, 2])
        assert cell.gfp_stats == cell.signal_stats['gfp']


def test_set_frequency():
    from hcat.haircell import HairCell
    cell = HairCell([0, 0, 0, 2, 2, 2], [10.0, 4.0, 1.0], np.zeros((1, 4, 2, 2, 2), np.float32),
                    np.zeros((2, 2, 2), bool), 9)
    curve = np.array([[0.0, 4.0, 50.0], [0.0, 9.0, 50.0]])     # x row against centre[1], y row against centre[0]
    cell.set_frequency(curve, np.array([0.1, 0.5, 0.9]))
    assert cell.frequency[1] == 0.5 and np.array_equal(cell.frequency[0], curve[:, 1])


def test_argument_errors():
    from hcunet_amd.cells import cell_table, generate_cell_objects
    image = torch.zeros((1, 4, 6, 5, 3))
    labels = np.zeros((6, 5, 3), np.int32)
    with pytest.raises(ValueError, match='batch'):
        cell_table(torch.zeros((2, 4, 6, 5, 3)), labels)
    with pytest.raises(ValueError, match='image'):
        cell_table(image[0], labels)
    with pytest.raises(ValueError, match='match'):
        cell_table(image, np.zeros((6, 5, 4), np.int32))
    with pytest.raises(ValueError, match='match'):
        cell_table(image, np.zeros((1, 1, 6, 6, 3), np.int64))
    with pytest.raises(TypeError, match='fp32'):
        cell_table(image.double(), labels)
    with pytest.raises(TypeError, match='integer'):
        cell_table(image, labels.astype(np.float32))
    with pytest.raises(TypeError, match='integer'):
        cell_table(image, labels.astype(bool))
    with pytest.raises(IndexError, match='channels'):
        generate_cell_objects(image[:, :3], labels, None, 0, 0)


def test_reexports():
    import hcat
    import hcat.haircell
    import hcat.segment
    from hcunet_amd import cells, haircell
    assert hcat.haircell.HairCell is haircell.HairCell and hcat.segment.HairCell is haircell.HairCell
    assert hcat.segment.generate_cell_objects is cells.generate_cell_objects
    assert hcat.generate_cell_objects is cells.generate_cell_objects


def test_entry_point_argument_checks():
    """The C entry points refuse, before any launch: a volume of 2^31 voxels or more, more z planes than
    the LDS plane table, a channel stride below the volume, null tables."""
    import ctypes
    from hcunet_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(64)     # never read: every call below returns from its checks
    assert L.hcu_cell_boxes(p, 2048, 2048, 512, 4, p, None) == _lib.HCU_ERR_UNSUPPORTED
    assert L.hcu_cell_boxes(p, 8, 8, 8, 0, p, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_cell_boxes(None, 8, 8, 8, 4, p, None) == _lib.HCU_ERR_INVALID
    stats = lambda stride, C, X, Y, Z, n, dtype=_lib.HCU_F16: L.hcu_cell_stats(p, p, p, dtype, stride, C, X, Y, Z, n,
                                                                            p, p, p, p, p, p, None)
    assert stats(1 << 31, 4, 2048, 2048, 512, 4) == _lib.HCU_ERR_UNSUPPORTED
    assert stats(8 * 8 * (_lib.CELL_MAX_PLANES + 1), 4, 8, 8, _lib.CELL_MAX_PLANES + 1, 4) == _lib.HCU_ERR_UNSUPPORTED
    assert stats(8 * 8 * 8 - 1, 4, 8, 8, 8, 4) == _lib.HCU_ERR_INVALID
    assert stats(8 * 8 * 8, 0, 8, 8, 8, 4) == _lib.HCU_ERR_INVALID
    assert 'chan_stride' in _lib.last_error() or 'positive' in _lib.last_error()
