"""Drop-in hcat.train.train_utils: the training targets the reference's
preprocess_manual_masks.py derives from an instance-label stack, computed on
the device (csrc/targets.hip).

  makePWL                hcat/train/train_utils.py:9-93     pixel-weight map, float64 [Z,Y,X]
  colormask_to_mask      :175-187                           binary mask, uint8 [Z,Y,X]
  CalculateCenterOfMass  :190-237                           (centre volume float64, id stack uint32)
  VectorToCenter         :240-274                           vectors to the centre, float64 [Z,Y,X,3]

Same call conventions and returned numpy types as the reference.  Added:
where the reference takes a path, an ndarray or a device tensor is accepted
too; `reader=` (any callable path -> ndarray, as hcat.dataloader.Stack)
replaces skimage.io.imread; `as_tensor=True` returns device tensors without a
host copy of any volume.  `makeMask` is not provided: its create_mask scan
(:147-172) reads neighbours it has already overwritten, a sequential
dependence along x and y, and stays the reference's own.

Every result is bit for bit the reference's: the kernels do integer work and
look float64 values up in tables computed here with the reference's numpy
expressions (`pwl_offsets`, `pwl_values`); the centre of mass is an exact
integer sum per id divided and rounded here in float64 as
scipy.ndimage.center_of_mass and np.round do (every sum of a stack below 2^31
voxels stays below 2^53).

Label stacks: a colour stack [Z,Y,X,3] uint8 / uint16, or an id stack [Z,Y,X]
uint8 / uint16 / int32 / uint32 (int64 ids are narrowed), Z*Y*X < 2^31.
torch has no arithmetic on uint16 / uint32: a device tensor of int16 / int32
is read as the same bits, and with as_tensor=True the id stack comes back as
int32.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

W0, SIGMA = 11, 5   # makePWL.find_closest :67-68

_NP_CODES = {np.dtype(np.uint8): _lib.HCU_U8, np.dtype(np.uint16): _lib.HCU_U16,
             np.dtype(np.int32): _lib.HCU_I32, np.dtype(np.uint32): _lib.HCU_U32}
_NP_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
_TORCH_CODES = {torch.uint8: _lib.HCU_U8, torch.int16: _lib.HCU_U16, torch.uint16: _lib.HCU_U16,
                torch.int32: _lib.HCU_I32, torch.uint32: _lib.HCU_U32}


def pwl_offsets(dedup=True):
    """The probe offsets of find_closest (:70-74): (offsets int32 [n,2] of
    (dx, dy), ring_begin int32 [10]); radius l owns rows ring_begin[l-1] ..
    ring_begin[l].  dedup drops an offset a ring has already probed: the
    result depends only on which keys a ring shows and on the first key seen,
    and first occurrences keep their order (tests/test_targets.py)."""
    angles = np.linspace(0, 2 * np.pi, 63)
    offsets, begin = [], [0]
    for l in np.arange(1, 10):
        ring = []
        for theta in angles:
            d = (int(np.rint(l * np.cos(theta))), int(np.rint(l * np.sin(theta))))
            if not dedup or d not in ring:
                ring.append(d)
        offsets += ring
        begin.append(len(offsets))
    return np.array(offsets, dtype=np.int32), np.array(begin, dtype=np.int32)


def pwl_values():
    """float64 [9,9]: the value of (l0, l1) as :91 computes it from the radii
    (numpy integers of np.arange(1, 10))."""
    radii = np.arange(1, 10)
    v = np.zeros((9, 9), dtype=np.float64)
    for i, l0 in enumerate(radii):
        for j, l1 in enumerate(radii):
            v[i, j] = W0 * np.exp(-1 * ((l0 + l1) ** 2) / (2 * (SIGMA ** 2)))
    return v


_TABLES = None


def _pwl_tables():
    global _TABLES
    if _TABLES is None:
        off, begin = pwl_offsets()
        _TABLES = (np.ascontiguousarray(off), np.ascontiguousarray(begin), np.ascontiguousarray(pwl_values()))
    return _TABLES


def _read(x, reader):
    """A path through `reader` (default: as hcat.dataloader.Stack reads)."""
    if isinstance(x, (str, os.PathLike)):
        if reader is None:
            from .dataloader import _default_reader
            reader = _default_reader()
            if reader is None:
                raise ImportError('hcat.train.train_utils reads .tif stacks with skimage.io or tifffile; '
                                  'neither is installed (pass reader=callable, or an array)')
        return reader(x)
    return x


def _device_of(x):
    if isinstance(x, torch.Tensor) and x.device.type == 'cuda':
        return x.device
    return torch.device('cuda', torch.cuda.current_device())


def _label_code(x, what):
    """The HCU dtype code of a label stack (host check, before any device work)."""
    if isinstance(x, torch.Tensor):
        code = _lib.HCU_I32 if x.dtype == torch.int64 else _TORCH_CODES.get(x.dtype)
    else:
        dt = np.asarray(x).dtype
        code = _lib.HCU_I32 if dt.kind in 'iu' and dt.itemsize == 8 else _NP_CODES.get(dt)
    if code is None:
        raise TypeError(f'{what}: expected uint8, uint16, int32 or uint32 labels, got {x.dtype}')
    return code


def _labels(x, device, what):
    """(contiguous device tensor holding the stack's bits, its HCU dtype code)."""
    code = _label_code(x, what)
    if isinstance(x, torch.Tensor):
        t = x.to(torch.int32) if x.dtype == torch.int64 else x
    else:
        a = np.asarray(x)
        if a.dtype.itemsize == 8:
            a = a.astype(np.int32)
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(_NP_VIEW.get(a.dtype, a.dtype)))
    return t.to(device).contiguous(), code


def check_centres(present, hits):
    """ValueError unless every present id (`present` bool [n], id 0 ignored)
    has exactly one centre voxel (`hits` int [n])."""
    present = np.array(present, dtype=bool)
    present[0] = False
    bad = np.nonzero(present & (np.asarray(hits) != 1))[0]
    if bad.size:
        raise ValueError('VectorToCenter: every id of colormask needs exactly one voxel in center; '
                         + ', '.join(f'id {i} has {hits[i]}' for i in bad[:8]) + (' ...' if bad.size > 8 else ''))
    return present


def _dims(t, what):
    if t.dim() == 4 and t.shape[3] == 3:
        return tuple(int(s) for s in t.shape[:3]), 3
    if t.dim() == 3:
        return tuple(int(s) for s in t.shape), 1
    raise ValueError(f'{what}: expected a [Z,Y,X,3] colour stack or a [Z,Y,X] id stack, got {tuple(t.shape)}')


def _keys(t, code, map_first, what):
    """int64 [Z,Y,X]: one key per voxel (hcu_label_keys; below 2^48, so the
    signed order is the key order)."""
    (Z, Y, X), channels = _dims(t, what)
    keys = _lib.empty((Z, Y, X), torch.int64, t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().hcu_label_keys(_lib.ptr(t), code, Z, Y, X, channels, int(map_first),
                                             _lib.ptr(keys), _lib.stream_handle(t.device)), what)
    return keys


def _moments(ids, n_ids):
    """int64 [n_ids,4] on the device: count, sum z, sum y, sum x per id."""
    Z, Y, X = (int(s) for s in ids.shape)
    m = _lib.empty((n_ids, 4), torch.int64, ids.device)
    with torch.cuda.device(ids.device):
        _lib.check(_lib.lib().hcu_label_moments(_lib.ptr(ids), Z, Y, X, n_ids, _lib.ptr(m),
                                                _lib.stream_handle(ids.device)), 'label_moments')
    return m


class makePWL:
    """makePWL()(imagepath) -> float64 [Z,Y,X]: 0 on labelled voxels; on a
    background voxel 11 * exp(-(l0 + l1)**2 / 50) of the radii (<= 9) at which
    its ray scan meets the nearest and the next other cell, 0 when it does not
    meet two."""

    def __init__(self, reader=None, as_tensor=False):
        self.reader = reader
        self.as_tensor = as_tensor

    def __call__(self, imagepath):
        x = _read(imagepath, self.reader)
        t, code = _labels(x, _device_of(x), 'makePWL')
        keys = _keys(t, code, False, 'makePWL')
        Z, Y, X = (int(s) for s in keys.shape)
        off, begin, values = _pwl_tables()
        out = _lib.empty((Z, Y, X), torch.float64, t.device)
        with torch.cuda.device(t.device):
            _lib.check(_lib.lib().hcu_pwl_scan(
                _lib.ptr(keys), Z, Y, X, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                begin.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                values.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _lib.ptr(out),
                _lib.stream_handle(t.device)), 'makePWL')
        return out if self.as_tensor else out.cpu().numpy()


def colormask_to_mask(colormask, as_tensor=False):
    """Every voxel of the [Z,Y,X,3] colour mask with a non-zero channel becomes
    (1, 1, 1) IN PLACE (an ndarray is written back); returns uint8 [Z,Y,X],
    channel 0 * 255."""
    if isinstance(colormask, torch.Tensor):
        shape = colormask.shape
    else:
        colormask = np.asarray(colormask)
        shape = colormask.shape
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f'colormask_to_mask: expected a [Z,Y,X,3] colour mask, got {tuple(shape)}')
    device = _device_of(colormask)
    t, code = _labels(colormask, device, 'colormask_to_mask')
    Z, Y, X = (int(s) for s in t.shape[:3])
    mask = _lib.empty((Z, Y, X), torch.uint8, device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().hcu_colormask_binary(_lib.ptr(t), code, Z, Y, X, _lib.ptr(mask),
                                                   _lib.stream_handle(device)), 'colormask_to_mask')
    if isinstance(colormask, torch.Tensor):
        if t.data_ptr() != colormask.data_ptr():   # a host, strided or int64 tensor: t is a copy
            colormask.copy_(t)
    else:
        back = t.cpu().numpy()   # (uint16 / uint32 travel as the signed type of their width)
        colormask[...] = back.view(colormask.dtype) if back.dtype.itemsize == colormask.dtype.itemsize else back
    return mask if as_tensor else mask.cpu().numpy()


class CalculateCenterOfMass:
    """CalculateCenterOfMass()(imagepath) -> (center_of_mass float64 [Z,Y,X],
    new_image uint32 [Z,Y,X]).  The colour of voxel [0,0,0] is background; the
    distinct colours in lexicographic order are the ids 0, 1, ... of new_image;
    center_of_mass holds each id at the rounded (half to even) mean voxel of
    its cell, written in id order (a later id at the same voxel wins)."""

    def __init__(self, reader=None, as_tensor=False):
        self.reader = reader
        self.as_tensor = as_tensor

    def __call__(self, imagepath):
        x = _read(imagepath, self.reader)
        t, code = _labels(x, _device_of(x), 'CalculateCenterOfMass')
        # a [Z,Y,X] stack stacked to three equal channels (:197-198) orders as its one channel does
        keys = _keys(t, code, True, 'CalculateCenterOfMass')
        Z, Y, X = (int(s) for s in keys.shape)
        uniq, inverse = torch.unique(keys, sorted=True, return_inverse=True)   # torch as plumbing
        ids = inverse.to(torch.int32)
        n = int(uniq.numel())
        m = _moments(ids, n).cpu().numpy()
        count = m[:, 0]   # > 0: every id has a voxel
        # scipy.ndimage.center_of_mass: float64 sum of the coordinates / the voxel count
        cz, cy, cx = (np.round(m[:, k].astype(np.float64) / count).astype(np.int64) for k in (1, 2, 3))
        lin = (cz * Y + cy) * X + cx
        # center_of_mass[z, y, x] = id in id order: the last id of a voxel stays
        where, last = np.unique(lin[::-1], return_index=True)
        winner = (n - 1 - last).astype(np.float64)
        if self.as_tensor:
            com = torch.zeros((Z, Y, X), dtype=torch.float64, device=t.device)
            com.view(-1)[torch.from_numpy(where).to(t.device)] = torch.from_numpy(winner).to(t.device)
            return com, ids
        com = np.zeros((Z, Y, X), dtype=np.float64)
        com.reshape(-1)[where] = winner
        return com, ids.cpu().numpy().view(np.uint32)


class VectorToCenter:
    """VectorToCenter()(center, colormask, mask) -> float64 [Z,Y,X,3]: for a
    voxel of id i of `colormask` ([Z,Y,X] ids), ((z - cz) / Z, (y - cy) / Y,
    (x - cx) / X) with (cz, cy, cx) the one voxel of `center` equal to i; 0 for
    id 0.  `mask` is not read (as in the reference).

    Raises ValueError where an id of `colormask` has no voxel or more than one
    voxel in `center` (the reference fails there with a broadcasting
    ValueError, or an IndexError for a one-voxel cell)."""

    def __init__(self, as_tensor=False):
        self.as_tensor = as_tensor

    def __call__(self, center, colormask, mask=None):
        if not isinstance(colormask, torch.Tensor):
            colormask = np.asarray(colormask)
        if not isinstance(center, torch.Tensor):
            center = np.asarray(center)
        if len(colormask.shape) != 3:
            raise ValueError(f'VectorToCenter: expected a [Z,Y,X] id stack, got {tuple(colormask.shape)}')
        if tuple(center.shape) != tuple(colormask.shape):
            raise ValueError(f'VectorToCenter: center {tuple(center.shape)} and colormask '
                             f'{tuple(colormask.shape)} differ')
        _label_code(colormask, 'VectorToCenter')
        centre_f64 = center.dtype == (torch.float64 if isinstance(center, torch.Tensor) else np.float64)
        if not centre_f64:
            _label_code(center, 'VectorToCenter (center)')
        device = _device_of(colormask) if isinstance(colormask, torch.Tensor) else _device_of(center)
        t, code = _labels(colormask, device, 'VectorToCenter')
        Z, Y, X = (int(s) for s in t.shape)
        if code in (_lib.HCU_I32, _lib.HCU_U32):
            ids = t.view(torch.int32)
        else:
            ids = _keys(t, code, False, 'VectorToCenter').to(torch.int32)
        n = int(ids.max()) + 1
        if n < 1:
            raise ValueError('VectorToCenter: negative ids')
        present = _moments(ids, n)[:, 0].cpu().numpy() > 0
        if centre_f64:
            c = center if isinstance(center, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(center))
            c, ccode = c.to(device).contiguous(), _lib.HCU_F64
        else:
            c, ccode = _labels(center, device, 'VectorToCenter')
        index = _lib.empty((n,), torch.int32, device)
        hits = _lib.empty((n,), torch.int32, device)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().hcu_center_table(_lib.ptr(c), ccode, Z, Y, X, n, _lib.ptr(index),
                                                   _lib.ptr(hits), _lib.stream_handle(device)), 'VectorToCenter')
        index, hits = index.cpu().numpy().astype(np.int64), hits.cpu().numpy()
        present = check_centres(present, hits)
        table = np.zeros((n, 4), dtype=np.int32)
        table[:, 0], table[:, 1], table[:, 2] = index // (Y * X), index // X % Y, index % X
        table[:, 3] = present
        table[~present] = 0
        centres = torch.from_numpy(table).to(device)
        out = _lib.empty((Z, Y, X, 3), torch.float64, device)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().hcu_vector_to_center(_lib.ptr(ids), Z, Y, X, _lib.ptr(centres), n,
                                                       _lib.ptr(out), _lib.stream_handle(device)),
                       'VectorToCenter')
        return out if self.as_tensor else out.cpu().numpy()
