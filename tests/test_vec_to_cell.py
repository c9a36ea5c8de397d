"""CPU: instance labels from the vector field (hcunet_amd/instances.py,
csrc/instances.hip) without a device.  The numpy restatement
(tests/vec_to_cell_oracle.py) reproduces the reference's recorded hist and
label (tests/golden/vec_to_cell.npz) bit for bit, and its Gaussian is
scipy.ndimage.gaussian_filter's bit for bit where scipy imports; the host
weight table and the host half of the peak search; the entry points refuse bad
arguments before any launch; the drop-in namespace."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hcat.segment
from hcunet_amd import _lib, instances
from tests import vec_to_cell_oracle as vo

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'vec_to_cell.npz'))
CASES = ['a', 'b']


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixture_holds_what_it_should():
    assert GOLD['a.vector'].shape == (1, 3, 64, 44, 6) and GOLD['b.vector'].shape == (1, 3, 23, 45, 5)
    assert GOLD['a.vector'].dtype == np.float16
    assert str(GOLD['gaussian_stub']).startswith('scipy.ndimage.gaussian_filter')
    assert str(GOLD['peak_stub']) == 'tests.vec_to_cell_oracle.peak_local_max'
    # at least three peaks whose smoothed values lie far more than 1e-13 apart
    top = np.sort(GOLD['a.smooth'][tuple(GOLD['a.peaks'].T)])[::-1]
    assert len(top) >= 3 and np.min(-np.diff(top)) > 1e-7
    assert GOLD['a.counts'].sum() < 64 * 44 * 6                        # some votes leave the volume
    assert 0 < GOLD['b.mask'].mean() < 1 and GOLD['b.mask'].dtype == np.uint8


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_reference(name):
    got = vo.pixel_vec_to_cell(GOLD[name + '.vector'].astype(np.float32), GOLD[name + '.mask'])
    assert same_bits(got['hist'], GOLD[name + '.hist'])
    assert same_bits(got['label'], GOLD[name + '.label'])
    assert same_bits(got['counts'].astype(np.int32), GOLD[name + '.counts'])
    assert same_bits(got['smooth'], GOLD[name + '.smooth'])
    assert same_bits(got['peaks'], GOLD[name + '.peaks'])
    # the recorded peaks handed back in give the same label
    again = vo.pixel_vec_to_cell(GOLD[name + '.vector'].astype(np.float32), GOLD[name + '.mask'],
                                 peaks=GOLD[name + '.peaks'])
    assert same_bits(again['label'], GOLD[name + '.label'])


@pytest.mark.parametrize('shape', [(64, 44, 6), (48, 20, 6), (23, 45, 5)])
def test_restatement_gaussian_is_scipys(shape):
    ndi = pytest.importorskip('scipy.ndimage')
    a = np.random.default_rng(3).random(shape)
    want = ndi.gaussian_filter(a, 5, mode='nearest', truncate=4.0)
    assert same_bits(vo.gaussian(a, 5), want)
    mf = ndi.maximum_filter(a, size=2, mode='constant')
    assert same_bits(vo.max_filter2(a), mf)


def test_host_weight_table():
    for sigma in (5, 2.5, 0.7):
        w, r = instances.gaussian_weights(sigma)
        w2, r2 = vo.gaussian_weights(sigma)
        assert r == r2 == int(4.0 * float(sigma) + 0.5) and same_bits(w, w2)
        assert len(w) == 2 * r + 1 and same_bits(w, w[::-1])
    w, r = instances.gaussian_weights(5)
    assert r == _lib.VOTE_RADIUS == 20
    x = np.arange(-20, 21)
    phi = np.exp(-0.5 / 25.0 * x ** 2)
    assert same_bits(w, phi / phi.sum())


def test_select_peaks_orders_ties_and_spacing():
    shape = (9, 10, 11)

    def lin(*c):
        return int(np.ravel_multi_index(c, shape))

    # value ties keep C order, whatever order the device appended them in
    idx = [lin(5, 5, 5), lin(2, 2, 2), lin(7, 2, 8), lin(2, 7, 3)]
    val = [0.5, 0.5, 0.9, 0.5]
    for perm in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]):
        got = instances.select_peaks([idx[p] for p in perm], [val[p] for p in perm], shape)
        assert got.tolist() == [[7, 2, 8], [2, 2, 2], [2, 7, 3], [5, 5, 5]]
        assert np.array_equal(got, vo.select_peaks([idx[p] for p in perm], [val[p] for p in perm], shape))
    # a plateau: of two neighbours of equal value the first in C order stays.  (4,4,5) is next to
    # (4,4,4) and goes; (5,5,6) is next to the dropped (4,4,5) only, two from (4,4,4), and stays;
    # (4,4,7) is diagonal to (5,5,6) and goes; (3,3,3) is diagonal to (4,4,4) and goes
    idx = [lin(4, 4, 4), lin(4, 4, 5), lin(5, 5, 6), lin(4, 4, 7), lin(3, 3, 3)]
    val = [0.7, 0.7, 0.7, 0.6, 0.2]
    got = instances.select_peaks(idx[::-1], val[::-1], shape)
    assert got.tolist() == [[4, 4, 4], [5, 5, 6]]
    assert np.array_equal(got, vo.select_peaks(idx, val, shape))
    # nothing
    assert instances.select_peaks([], [], shape).shape == (0, 3)


def test_select_peaks_caps_at_num_peaks():
    shape = (40, 40, 5)
    coords = [(2 + 3 * (k // 12), 2 + 3 * (k % 12), 2) for k in range(101)]   # 101 candidates, all 3 apart
    idx = [int(np.ravel_multi_index(c, shape)) for c in coords]
    val = np.linspace(0.2, 0.9, 101)
    got = instances.select_peaks(idx, val, shape)
    assert got.shape == (100, 3)
    assert got.tolist() == [list(c) for c in coords[::-1][:100]]              # the lowest value is the one left out
    assert np.array_equal(got, vo.select_peaks(idx, val, shape))
    assert instances.select_peaks(idx, val, shape, num_peaks=7).tolist() == [list(c) for c in coords[::-1][:7]]


_VP = ctypes.c_void_p


def test_entry_points_reject_bad_arguments():
    L = _lib.lib()
    p = _VP(4096)   # never dereferenced: every call below fails its host checks
    D = ctypes.POINTER(ctypes.c_double)
    w = np.ascontiguousarray(instances.gaussian_weights(5)[0][:21])
    wp = w.ctypes.data_as(D)
    big = (1 << 11, 1 << 10, 1 << 10)   # 2^31 voxels
    F32, INV, SHP, UNS = _lib.HCU_F32, _lib.HCU_ERR_INVALID, _lib.HCU_ERR_SHAPE, _lib.HCU_ERR_UNSUPPORTED

    assert L.hcu_vec_votes(None, F32, 512, 0, 8, 8, 8, p, p, None) == INV
    assert L.hcu_vec_votes(p, F32, 512, 0, 8, 8, 8, None, p, None) == INV
    assert L.hcu_vec_votes(p, F32, 512, 0, 8, 8, 8, p, None, None) == INV
    assert L.hcu_vec_votes(p, _lib.HCU_F64, 512, 0, 8, 8, 8, p, p, None) == INV
    assert L.hcu_vec_votes(p, _lib.HCU_U8, 512, 0, 8, 8, 8, p, p, None) == INV
    assert L.hcu_vec_votes(p, F32, 511, 0, 8, 8, 8, p, p, None) == INV            # planes overlap
    assert 'vec_votes' in _lib.last_error()
    assert L.hcu_vec_votes(p, F32, 512, 0, 8, 0, 8, p, p, None) == SHP
    assert L.hcu_vec_votes(p, F32, 1 << 31, 0, *big, p, p, None) == UNS

    assert L.hcu_vote_hist(None, p, 8, 8, 8, p, None) == INV
    assert L.hcu_vote_hist(p, p, 8, 8, 8, None, None) == INV
    assert L.hcu_vote_hist(p, p, 8, 8, -1, p, None) == SHP
    assert L.hcu_vote_hist(p, p, *big, p, None) == UNS

    q = _VP(8192)
    assert L.hcu_vote_smooth(None, p, 8, 8, 8, wp, 20, p, q, None) == INV
    assert L.hcu_vote_smooth(p, p, 8, 8, 8, None, 20, p, q, None) == INV
    assert L.hcu_vote_smooth(p, p, 8, 8, 8, wp, 20, p, p, None) == INV           # out is scratch
    assert L.hcu_vote_smooth(p, p, 8, 8, 8, wp, 21, p, q, None) == INV           # past HCU_VOTE_RADIUS
    assert L.hcu_vote_smooth(p, p, 8, 8, 8, wp, -1, p, q, None) == INV
    assert L.hcu_vote_smooth(p, p, 0, 8, 8, wp, 20, p, q, None) == SHP
    assert L.hcu_vote_smooth(p, p, *big, wp, 20, p, q, None) == UNS
    assert 'vote_smooth' in _lib.last_error()

    r = _VP(12288)
    assert L.hcu_smooth_f64(None, 8, 8, 8, wp, 20, q, r, None) == INV
    assert L.hcu_smooth_f64(p, 8, 8, 8, wp, 20, p, r, None) == INV               # in place
    assert L.hcu_smooth_f64(p, 8, 8, 8, wp, 20, q, q, None) == INV
    assert L.hcu_smooth_f64(p, 8, 8, 8, wp, 40, q, r, None) == INV
    assert L.hcu_smooth_f64(p, 8, 8, 0, wp, 20, q, r, None) == SHP

    n = ctypes.c_int(-5)
    nb = ctypes.byref(n)
    assert L.hcu_peak_candidates(None, 8, 8, 8, p, p, 16, p, nb, None) == INV
    assert L.hcu_peak_candidates(p, 8, 8, 8, p, p, 16, None, nb, None) == INV
    assert L.hcu_peak_candidates(p, 8, 8, 8, p, p, 16, p, None, None) == INV
    assert L.hcu_peak_candidates(p, 8, 8, 8, p, p, 0, p, nb, None) == INV
    assert L.hcu_peak_candidates(p, 8, 8, 8, p, p, 16, _VP(4100), nb, None) == INV   # state: 8-byte words
    assert L.hcu_peak_candidates(p, 8, 0, 8, p, p, 16, p, nb, None) == SHP
    assert L.hcu_peak_candidates(p, *big, p, p, 16, p, nb, None) == UNS
    assert n.value == -5

    assert L.hcu_vec_label(None, F32, 512, 8, 8, 8, p, 1, p, _lib.HCU_U8, 0, p, None) == INV
    assert L.hcu_vec_label(p, F32, 512, 8, 8, 8, p, 1, p, _lib.HCU_U8, 0, None, None) == INV
    assert L.hcu_vec_label(p, F32, 512, 8, 8, 8, None, 1, p, _lib.HCU_U8, 0, p, None) == INV   # a peak, no table
    assert L.hcu_vec_label(p, F32, 512, 8, 8, 8, p, -1, p, _lib.HCU_U8, 0, p, None) == INV
    assert L.hcu_vec_label(p, F32, 512, 8, 8, 8, p, 1, p, _lib.HCU_I32, 0, p, None) == INV    # mask dtype
    assert L.hcu_vec_label(p, F32, 512, 8, 8, 8, p, 1, p, _lib.HCU_U8, -1, p, None) == INV
    assert L.hcu_vec_label(p, _lib.HCU_U16, 512, 8, 8, 8, p, 1, p, _lib.HCU_U8, 0, p, None) == INV
    assert L.hcu_vec_label(p, F32, 100, 8, 8, 8, p, 1, p, _lib.HCU_U8, 0, p, None) == INV
    assert L.hcu_vec_label(p, F32, 512, 8, 8, 0, p, 1, p, _lib.HCU_U8, 0, p, None) == SHP
    assert L.hcu_vec_label(p, F32, 1 << 31, *big, p, 1, p, _lib.HCU_U8, 0, p, None) == UNS
    assert 'vec_label' in _lib.last_error()


def test_namespace_and_host_side_errors():
    assert hcat.segment.pixel_vec_to_cell is instances.pixel_vec_to_cell
    assert hcat.segment.hist3d is instances.hist3d
    assert hcat.segment.predict_segmentation_mask is not None
    mask = torch.ones(1, 1, 4, 5, 6)
    with pytest.raises(ValueError, match='batch of 2'):
        hcat.segment.pixel_vec_to_cell(torch.zeros(2, 3, 4, 5, 6), mask)
    with pytest.raises(ValueError):
        hcat.segment.pixel_vec_to_cell(torch.zeros(1, 2, 4, 5, 6), mask)            # not three channels
    with pytest.raises(ValueError):
        hcat.segment.pixel_vec_to_cell(torch.zeros(3, 4, 5, 6), mask)
    with pytest.raises(ValueError):
        hcat.segment.pixel_vec_to_cell(torch.zeros(1, 3, 4, 5, 6), torch.ones(4, 5, 7))
    with pytest.raises(TypeError):
        hcat.segment.pixel_vec_to_cell(torch.zeros(1, 3, 4, 5, 6), torch.ones(4, 5, 6, dtype=torch.int64))
    with pytest.raises(ValueError):
        hcat.segment.pixel_vec_to_cell(torch.zeros(1, 3, 4, 5, 6), mask, peaks=np.zeros((2, 3)))   # not integer
    with pytest.raises(ValueError):
        hcat.segment.pixel_vec_to_cell(torch.zeros(1, 3, 4, 5, 6), mask, peaks=np.zeros((3, 3), dtype=int), num_peaks=2)
    with pytest.raises(ValueError):
        hcat.segment.hist3d(np.zeros((2, 4, 5, 6), dtype=np.float32))
