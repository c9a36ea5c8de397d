"""Cell tables and cell objects on the GPU (csrc/cells.hip through
hcunet_amd.cells / hcat.segment) against the numpy restatement
(tests/cells_oracle.py, itself pinned to the reference's recorded cells by
tests/test_cells.py) and against the fixture (tests/golden/cells.npz).

Exact: ids, boxes, count, plane_count, box_min and both order statistics of the
median (integer atomics, a minimum, an exact radix select; compared by value
with NaN equal to NaN, so a zero's sign is free).  mean and std are float64
sums in the device's fixed order against the exactly rounded sums of the
restatement: the any-order float64 summation bounds
    |mean - fsum mean| <= (n + 2) 2^-53 mean(|g|)
    |std  - fsum std | <= (n + 8) 2^-52 std + 2^-52 |mean|
and two calls give the same bytes.  Every output buffer is poisoned before its
kernel runs, once with 0xFF (NaN / -1) and once with 0x3F (about 0.75 / a large
positive integer), so an unwritten or stale word shows.

Shapes: the fixture's, a few seconds in all: 40x36x7 (boxes of one to 2284
samples, on every face of the volume), 48x44x7 (264 ids, past the 256 of the
LDS box table; 8 samples a cell), 23x45x5 (odd sizes, a NaN, the mapping
decided by a voxel outside the mask)."""
import functools
import os

import numpy as np
import pytest
import torch

import hcat.segment as hs
from hcunet_amd import _lib, cells
from tests import cells_oracle as co
from tests.test_cells import GOLD, NAMES, STAT_CHANNEL, case, check_float32_stats, mean_abs

pytestmark = pytest.mark.gpu
CASES = ['a', 'b', 'c']
EXACT = ['boxes', 'count', 'plane_count', 'box_min', 'median']


@pytest.fixture(autouse=True, params=[0xFF, 0x3F], ids=['poisonFF', 'poison3F'])
def poisoned(request, monkeypatch):
    monkeypatch.setattr(_lib, 'POISON', request.param)


def host(table):
    return {k: getattr(table, k).cpu().numpy() for k in table._fields}


@functools.lru_cache(maxsize=None)
def mabs(name):
    image, labels, t = case(name)
    return mean_abs(image, labels, t)


def check_table(got, want, mean_abs_g):
    """got: host arrays of a CellTable; want: the restatement's tables of the same input."""
    assert got['boxes'].dtype == np.int32 and got['count'].dtype == np.int32 and got['plane_count'].dtype == np.int32
    assert got['box_min'].dtype == np.float32 and got['median'].dtype == np.float32
    assert got['mean'].dtype == np.float64 and got['std'].dtype == np.float64
    np.testing.assert_array_equal(got['ids'], want['ids'])
    for k in EXACT:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    nan = np.isnan(want['mean'])
    assert np.array_equal(np.isnan(got['mean']), nan) and np.array_equal(np.isnan(got['std']), nan)
    n = want['count'][:, None].astype(np.float64)
    em = np.abs(got['mean'] - want['mean'])
    es = np.abs(got['std'] - want['std'])
    bm = (n + 2) * 2.0 ** -53 * mean_abs_g
    bs = (n + 8) * 2.0 ** -52 * want['std'] + 2.0 ** -52 * np.abs(want['mean'])
    ok = ~nan
    print('largest mean error / bound', float((em[ok] / np.maximum(bm[ok], 1e-300)).max()) if ok.any() else None,
          'std', float((es[ok] / np.maximum(bs[ok], 1e-300)).max()) if ok.any() else None)
    assert (em[ok] <= bm[ok]).all(), (em[ok].max(), np.argwhere(ok & (em > bm))[:4])
    assert (es[ok] <= bs[ok]).all(), (es[ok].max(), np.argwhere(ok & (es > bs))[:4])


@pytest.mark.parametrize('name', CASES)
def test_cell_table(name):
    image, labels, want = case(name)
    table = cells.cell_table(torch.from_numpy(image).cuda(), torch.from_numpy(labels).cuda())
    assert all(getattr(table, k).is_cuda for k in table._fields) and table.ids.dtype == torch.int64
    got = host(table)
    check_table(got, want, mabs(name))
    # the same input again: the same bytes in every table
    again = host(cells.cell_table(torch.from_numpy(image).cuda(), torch.from_numpy(labels).cuda()))
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize('layout', ['dense', 'slice'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('name', ['a', 'c'])
def test_image_dtypes_and_layouts(name, dtype, layout):
    image, labels, want = case(name)
    t = torch.from_numpy(image).to(dtype)
    seen = t.float().numpy()                    # what the kernel reads: bf16 rounds the fixture's values
    if dtype == torch.bfloat16:
        want = co.cell_table(seen, labels)
    dev = t.cuda()
    if layout == 'slice':                       # channels 1..4 of a six-channel tensor, read in place
        wide = torch.full((1, 6) + tuple(t.shape[2:]), -7.0, dtype=dtype, device='cuda')
        wide[:, 1:5] = dev
        dev = wide[:, 1:5]
        assert dev.storage_offset() > 0 and dev.untyped_storage().nbytes() > dev.numel() * dev.element_size()
    got = host(cells.cell_table(dev, torch.from_numpy(labels).cuda()))
    check_table(got, want, mean_abs(seen, labels, want))


@pytest.mark.parametrize('where', ['numpy', 'cpu', 'cuda'])
@pytest.mark.parametrize('kind', ['int32', 'int64', 'float64', '5d'])
def test_label_dtypes(kind, where):
    image, labels, want = case('a')
    lab = {'int32': labels.astype(np.int32), 'int64': labels, 'float64': labels.astype(np.float64),
           '5d': labels.astype(np.int32)[None, None]}[kind]
    arg = lab if where == 'numpy' else torch.from_numpy(lab).to(where)
    table = cells.cell_table(torch.from_numpy(image).half().cuda(), arg)
    assert table.ids.dtype == {'int32': torch.int32, 'int64': torch.int64, 'float64': torch.float64,
                               '5d': torch.int32}[kind]
    check_table(host(table), want, mabs('a'))


def test_host_image_and_one_channel():
    image, labels, want = case('c')
    got = host(cells.cell_table(image, labels))               # numpy in: the tables are still device tensors
    check_table(got, want, mabs('c'))
    one = np.ascontiguousarray(image[:, 1:2])
    w1 = co.cell_table(one, labels)
    assert w1['box_min'][0] >= 0                               # the negative voxel is in channel 3: no mapping now
    check_table(host(cells.cell_table(torch.from_numpy(image).cuda()[:, 1:2], labels)), w1,
                mean_abs(one, labels, w1))


def test_generate_cell_objects():
    image, labels, want = case('a')
    got = hs.generate_cell_objects(torch.from_numpy(image).half().cuda(), torch.from_numpy(labels).cuda(), None,
                                   100, 200)
    assert tuple(GOLD['a.chunk']) == (100, 200) and len(got) == len(want['ids'])
    mean, std = np.zeros((len(got), 5), np.float32), np.zeros((len(got), 5), np.float32)
    for i, cell in enumerate(got):
        assert isinstance(cell, hs.HairCell)
        assert cell.unique_id == GOLD['a.unique_id'][i] and type(cell.unique_id) is np.int64
        assert list(cell.image_coords) == list(GOLD['a.image_coords'][i])
        assert list(cell.center) == list(GOLD['a.center'][i])
        assert cell.is_bad == GOLD['a.is_bad'][i]
        assert isinstance(cell.volume, int) == GOLD['a.volume_is_int'][i]
        assert np.float64(cell.volume).tobytes() == GOLD['a.volume'][i].tobytes()
        assert list(cell.signal_stats) == NAMES
        for j, d in enumerate([cell.signal_stats[k] for k in NAMES] + [cell.gfp_stats]):
            if cell.is_bad:
                assert list(d) == ['mean', 'std', 'median'] and all(np.isnan(v) for v in d.values())
                mean[i, j] = std[i, j] = np.nan
                continue
            assert list(d) == ['mean', 'std', 'median', 'num_samples']
            assert d['num_samples'] == (GOLD['a.num_samples'][i, j],)
            assert type(d['mean']) is np.float32 and type(d['std']) is np.float32 and type(d['median']) is np.float32
            assert d['median'] == GOLD['a.stats'][i, j, 2]
            mean[i, j], std[i, j] = d['mean'], d['std']
    # np.float32 of the device's float64 values against the reference's float32 sums: each within the
    # pairwise-summation bound of the exact value, plus the one rounding to float32
    ref = GOLD['a.stats']
    fixture = dict(want, mean=ref[:, :4, 0].astype(np.float64), std=ref[:, :4, 1].astype(np.float64))
    assert check_float32_stats(mean, std, fixture, mabs('a'), slack_ulps=1) == 35      # 7 good cells x 5 entries
    assert check_float32_stats(mean, std, want, mabs('a'), slack_ulps=1) == 35


def test_chained_with_pixel_vec_to_cell():
    gold = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'vec_to_cell.npz'))
    vector, mask = gold['a.vector'], gold['a.mask']
    dv = torch.from_numpy(vector).cuda()
    label = hs.pixel_vec_to_cell(dv, torch.from_numpy(mask).cuda(), as_tensor=True, label_offset=1)
    assert label.is_cuda and label.dtype == torch.float64
    image = torch.cat([dv, dv[:, :1] * 0.5], 1)                # four channels of fp16 values, negatives among them
    table = cells.cell_table(image, label)
    lab = label.cpu().numpy()
    img = image.float().cpu().numpy()
    want = co.cell_table(img, lab)
    # label_offset=1: cell i of the recorded peaks is labelled i + 1 and the all-ones mask leaves no background
    assert table.ids.dtype == torch.float64 and len(gold['a.peaks']) >= 3
    assert list(want['ids']) == [float(i + 1) for i in range(len(gold['a.peaks']))] and not (lab == 0).any()
    check_table(host(table), want, mean_abs(img, lab, want))
    assert int(want['count'].max()) > 1000


def test_background_only():
    image = torch.zeros((1, 4, 6, 5, 3), device='cuda')
    table = cells.cell_table(image, np.zeros((6, 5, 3), np.int64))
    assert [tuple(getattr(table, k).shape) for k in table._fields] == [(0,), (0, 6), (0,), (0, 3), (0,), (0, 4), (0, 4),
                                                                       (0, 4, 2)]
    assert all(getattr(table, k).is_cuda for k in table._fields)
    assert hs.generate_cell_objects(image, np.zeros((6, 5, 3), np.int64), None, 0, 0) == []
