"""CPU: the training-target generators (hcunet_amd/train_utils.py,
csrc/targets.hip) without a device.  The numpy restatement
(tests/targets_oracle.py) reproduces the reference's recorded outputs
(tests/golden/targets.npz) bit for bit; the host tables of the ring scan are
the reference's expressions, and dropping a ring's repeated offsets changes
no (l0, l1); VectorToCenter's and RecursiveStack's host-side errors; the entry
points refuse bad arguments before any launch."""
import ctypes
import os

import numpy as np
import pytest

import hcat.dataloader as hdl
import hcat.train
import hcat.train.train_utils as htu
from hcunet_amd import _lib
from hcunet_amd import train_utils as tu
from tests import targets_oracle as to

GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'targets.npz'))
DTYPES = ['u16', 'u8']


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixture_holds_what_it_should():
    a = GOLD['u16.labels']
    assert a.shape == (3, 24, 28, 3) and a.dtype == np.uint16 and GOLD['u8.labels'].dtype == np.uint8
    assert not a[0, 0, 0].any()
    for name in DTYPES:
        assert int(GOLD[name + '.ids'].max()) == 4                    # four cells
        assert len(np.unique(GOLD[name + '.pwl'])) > 4                # several (l0, l1) pairs met
        assert (GOLD[name + '.pwl'][1] == 0).all()                    # the cell alone in its slice: no second cell
    cols = np.unique(a.reshape(-1, 3), axis=0)
    close = [(p, q) for p in cols for q in cols
             if p[0] == q[0] and p[1] == q[1] and p[2] != q[2] and (int(p[2]) ^ int(q[2])) < 0x10000
             and (int(p[2]) ^ int(q[2])) & 0xFF == 0 and p.any() and q.any()]
    assert close   # two colours that differ only in channel 2 and only above bit 8


@pytest.mark.parametrize('name', DTYPES)
def test_restatement_reproduces_the_reference(name):
    labels = GOLD[name + '.labels']
    assert same_bits(to.make_pwl(labels), GOLD[name + '.pwl'])
    com, ids = to.center_of_mass(labels)
    assert same_bits(com, GOLD[name + '.com']) and same_bits(ids, GOLD[name + '.ids'])
    assert same_bits(to.vector_to_center(GOLD[name + '.com'], GOLD[name + '.ids']), GOLD[name + '.vec'])
    binary = labels.copy()
    assert same_bits(to.colormask_to_mask(binary), GOLD[name + '.mask'])
    assert same_bits(binary, GOLD[name + '.binary'])


def test_host_tables_are_the_reference_expressions():
    off, begin = tu.pwl_offsets(dedup=False)
    assert off.shape == (9 * 63, 2) and list(begin) == [63 * i for i in range(10)]
    angles = np.linspace(0, 2 * np.pi, 63)
    k = 0
    for l in np.arange(1, 10):
        for theta in angles:
            assert off[k, 0] == int(np.rint(l * np.cos(theta))) and off[k, 1] == int(np.rint(l * np.sin(theta)))
            k += 1
    assert np.abs(off).max() == 9
    values = tu.pwl_values()
    assert values.dtype == np.float64 and values.shape == (9, 9)
    lens = np.arange(1, 10)
    for i in range(9):
        for j in range(9):
            want = 11 * np.exp(-1 * ((lens[i] + lens[j]) ** 2) / (2 * (5 ** 2)))
            assert values[i, j].tobytes() == np.float64(want).tobytes()
    # the restatement's own tables are the same
    full, fbegin = to.offsets_full()
    assert np.array_equal(full, off) and np.array_equal(fbegin, begin)
    # the de-duplicated table: each ring's distinct offsets in first-occurrence order
    d, dbegin = tu.pwl_offsets()
    assert dbegin[0] == 0 and dbegin[9] == len(d) <= _lib.PWL_MAX_OFFSETS
    for l in range(1, 10):
        ring = [tuple(r) for r in off[begin[l - 1]:begin[l]]]
        assert [tuple(r) for r in d[dbegin[l - 1]:dbegin[l]]] == list(dict.fromkeys(ring))


def test_dropping_repeated_offsets_keeps_l0_l1():
    # every voxel of a 19 x 19 window decides the scan of its centre; windows
    # from empty to crowded, two to four distinct keys
    rng = np.random.default_rng(7)
    full, fbegin = to.offsets_full()
    d, dbegin = tu.pwl_offsets()
    seen = set()
    for density in (0.004, 0.01, 0.03, 0.1, 0.4):
        w = rng.integers(1, 5, size=(4000, 19, 19)) * (rng.random((4000, 19, 19)) < density)
        w[:, 9, 9] = 0
        a = to.ring_scan(w, 1, 1, full, fbegin)
        b = to.ring_scan(w, 1, 1, d, dbegin)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        seen |= set(zip(a[0].reshape(-1).tolist(), a[1].reshape(-1).tolist()))
    # the windows reached every radius for l0, pairs with l1 == l0 and l1 > l0, and scans that met one or no cell
    assert {p[0] for p in seen} == set(range(10))
    assert any(p[1] == p[0] > 0 for p in seen) and any(p[1] > p[0] > 0 for p in seen)
    assert any(p[0] > 0 and p[1] == 0 for p in seen) and (0, 0) in seen


def test_namespace():
    for name in ('makePWL', 'CalculateCenterOfMass', 'VectorToCenter', 'colormask_to_mask'):
        assert getattr(htu, name) is getattr(tu, name) is getattr(hcat.train, name)
    assert not hasattr(htu, 'makeMask')
    assert hdl.RecursiveStack.__mro__[1] is hdl.Stack


def test_vector_to_center_error_cases():
    ids = np.zeros((2, 4, 5), dtype=np.uint32)
    ids[0, 1, 1:3] = 1
    ids[1, 2, 2] = 2
    com = np.zeros(ids.shape)
    com[0, 1, 1], com[1, 2, 2] = 1, 2
    assert to.vector_to_center(com, ids).shape == (2, 4, 5, 3)
    # an id without a centre voxel, an id with two: one exception type
    none, two = com.copy(), com.copy()
    none[1, 2, 2] = 0
    two[1, 3, 3] = 2
    for bad in (none, two):
        with pytest.raises(ValueError):
            to.vector_to_center(bad, ids)
    present = np.array([True, True, True, False])
    assert list(tu.check_centres(present, np.array([0, 1, 1, 0]))) == [False, True, True, False]
    with pytest.raises(ValueError, match='id 2 has 0'):
        tu.check_centres(present, np.array([5, 1, 0, 0]))
    with pytest.raises(ValueError, match='id 1 has 2'):
        tu.check_centres(present, np.array([0, 2, 1, 7]))
    # what the host refuses before it touches the device
    v = tu.VectorToCenter()
    with pytest.raises(ValueError):
        v(com[:1], ids, None)                              # shapes differ
    with pytest.raises(ValueError):
        v(com[..., None], ids[..., None], None)            # not a [Z,Y,X] id stack
    with pytest.raises(TypeError):
        v(com, ids.astype(np.float32), None)               # ids are integers
    with pytest.raises(TypeError):
        v(com.astype(np.float32), ids, None)
    with pytest.raises(ValueError):
        tu.colormask_to_mask(np.zeros((2, 3, 4), dtype=np.uint8))


def test_recursive_stack_on_an_empty_folder(tmp_path):
    with pytest.raises(FileExistsError):
        hdl.RecursiveStack(str(tmp_path), image_transforms=[], joint_transforms=[], reader=np.load)


def test_recursive_stack_reports_an_incomplete_stack(tmp_path, capsys):
    # <name>.tif, .mask.tif and .pwl.tif are there, .labels.com.tif is not:
    # the message is printed and the lists stay as far as they were filled
    for suffix in ('.tif', '.mask.tif', '.pwl.tif'):
        with open(os.path.join(tmp_path, 'vol' + suffix), 'wb') as f:
            np.save(f, np.zeros((2, 3, 4), dtype=np.uint8))

    def reader(path):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        return np.load(path)

    data = hdl.RecursiveStack(str(tmp_path), image_transforms=[], joint_transforms=[], reader=reader)
    assert 'ISSUE WITH: ' + os.path.join(str(tmp_path), 'vol.mask') in capsys.readouterr().out
    assert len(data) == 1 and (len(data.image), len(data.pwl), len(data.com), len(data.vec)) == (1, 1, 0, 0)


_VP = ctypes.c_void_p


def test_entry_points_reject_bad_arguments():
    L = _lib.lib()
    p = _VP(4096)   # never dereferenced: every call below fails its host checks
    off, begin = tu.pwl_offsets()
    values = np.ascontiguousarray(tu.pwl_values())
    I, D = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)

    def scan(keys=p, shape=(2, 8, 8), off=off, begin=begin, out=p):
        off, begin = np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(begin, dtype=np.int32)
        return L.hcu_pwl_scan(keys, *shape, off.ctypes.data_as(I), begin.ctypes.data_as(I),
                              values.ctypes.data_as(D), out, None)

    assert scan(keys=None) == _lib.HCU_ERR_INVALID
    assert scan(out=None) == _lib.HCU_ERR_INVALID
    assert scan(shape=(0, 8, 8)) == _lib.HCU_ERR_SHAPE
    assert scan(shape=(1 << 11, 1 << 10, 1 << 10)) == _lib.HCU_ERR_UNSUPPORTED      # 2^31 voxels
    far = off.copy()
    far[3, 1] = 10                                                                   # past the LDS halo
    assert scan(off=far) == _lib.HCU_ERR_INVALID
    far[3, 1] = -10
    assert scan(off=far) == _lib.HCU_ERR_INVALID
    b = begin.copy()
    b[9] = _lib.PWL_MAX_OFFSETS + 1
    assert scan(begin=b, off=np.zeros((_lib.PWL_MAX_OFFSETS + 1, 2))) == _lib.HCU_ERR_INVALID
    b = begin.copy()
    b[4] = b[3] - 1
    assert scan(begin=b) == _lib.HCU_ERR_INVALID
    b = begin.copy()
    b[0] = 1
    assert scan(begin=b) == _lib.HCU_ERR_INVALID
    assert 'pwl_scan' in _lib.last_error()

    assert L.hcu_label_keys(None, _lib.HCU_U16, 2, 8, 8, 3, 0, p, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_label_keys(p, _lib.HCU_U16, 2, 8, 8, 2, 0, p, None) == _lib.HCU_ERR_SHAPE
    assert L.hcu_label_keys(p, _lib.HCU_F32, 2, 8, 8, 3, 0, p, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_label_keys(p, _lib.HCU_I32, 2, 8, 8, 3, 0, p, None) == _lib.HCU_ERR_INVALID   # colours are 8 / 16 bit
    assert L.hcu_label_keys(p, _lib.HCU_U8, 2, -1, 8, 1, 0, p, None) == _lib.HCU_ERR_SHAPE
    assert L.hcu_label_keys(p, _lib.HCU_U8, 1 << 11, 1 << 10, 1 << 10, 1, 0, p, None) == _lib.HCU_ERR_UNSUPPORTED

    assert L.hcu_label_moments(p, 2, 8, 8, 4, None, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_label_moments(p, 2, 8, 8, 0, p, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_label_moments(p, 2, 8, 0, 4, p, None) == _lib.HCU_ERR_SHAPE

    assert L.hcu_center_table(p, _lib.HCU_F64, 2, 8, 8, 4, p, None, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_center_table(p, _lib.HCU_F16, 2, 8, 8, 4, p, p, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_center_table(p, _lib.HCU_F64, 2, 8, 8, -3, p, p, None) == _lib.HCU_ERR_INVALID

    assert L.hcu_vector_to_center(p, 2, 8, 8, None, 4, p, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_vector_to_center(p, 2, 8, 8, _VP(4100), 4, p, None) == _lib.HCU_ERR_INVALID   # centres: 16-byte rows
    assert L.hcu_vector_to_center(p, 0, 8, 8, p, 4, p, None) == _lib.HCU_ERR_SHAPE

    assert L.hcu_colormask_binary(p, _lib.HCU_U8, 2, 8, 8, None, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_colormask_binary(p, _lib.HCU_F64, 2, 8, 8, p, None) == _lib.HCU_ERR_INVALID
    assert L.hcu_colormask_binary(p, _lib.HCU_U16, 1 << 11, 1 << 10, 1 << 10, p, None) == _lib.HCU_ERR_UNSUPPORTED
