"""Drop-in hcat.segment.generate_cell_objects (reference hcat/segment.py:
508-560) and the device tables behind it (csrc/cells.hip): what the reference
computes per id with a full-volume mask and np.indices on the host.

For each id of the label volume other than 0, in ascending order:

  box      x0..x1, y0..y1, z0..z1, the inclusive extent of the id's voxels;
           image_coords = [x0, y0, z0, x1, y1, z1]
  centre   [x0 + (x1-x0)/2 + x_ind_chunk, y0 + (y1-y0)/2 + y_ind_chunk,
           (z1-z0)/2]: QUIRK kept, the z term carries no z0 (:550)
  clipped  image and mask are sliced x0:x1, y0:y1, z0:z1 (:552-553), so the
           maximum face of every axis is dropped (QUIRK kept) and a cell of
           extent 1 along an axis has an empty clipped box; everything below
           is over the clipped box
  volume, statistics   hcunet_amd/haircell.py

cell_table returns device tensors, one row per id: ids, boxes int32 [n,6],
count int32 [n], plane_count int32 [n,Z], box_min fp32 [n], mean and std
float64 [n,C], median fp32 [n,C,2] (the two middle order statistics).  The
float64 mean and std are the tables' own precision; HairCell.from_table rounds
them to the float32 the reference reports.

Differences from the reference: an image batch other than 1 raises ValueError
(the reference slices every sample but reads sample 0); the progress prints are
dropped; a median that is a zero may carry the other sign (the device orders
-0 below +0, numpy's sort leaves them as they came).
"""
import collections

import numpy as np
import torch

from . import _lib
from .haircell import CHANNELS, HairCell
from .instances import _as_tensor, _device_of

CellTable = collections.namedtuple('CellTable', 'ids boxes count plane_count box_min mean std median')

_IMAGE_CODES = {torch.float32: _lib.HCU_F32, torch.float16: _lib.HCU_F16, torch.bfloat16: _lib.HCU_BF16}
_LABEL_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float64)
_WIDE_UNSIGNED = tuple(getattr(torch, n) for n in ('uint16', 'uint32', 'uint64') if hasattr(torch, n))


def _labels_3d(labels, shape):
    """The label volume as a [X,Y,Z] tensor of a dtype torch.unique takes."""
    t = _as_tensor(labels)
    if t.dim() == 5 and tuple(t.shape[:2]) == (1, 1):
        t = t[0, 0]
    if t.dim() != 3 or tuple(int(s) for s in t.shape) != shape:
        raise ValueError(f'cell_table: labels {tuple(t.shape)} do not match the volume {shape}')
    if t.dtype in _WIDE_UNSIGNED:
        t = t.to(torch.int64)
    if t.dtype not in _LABEL_DTYPES:
        raise TypeError(f'cell_table: labels are of an integer dtype or float64, got {t.dtype}')
    return t


def dense_ids(labels):
    """(ids, dense, n_ids): the label volume's distinct values other than 0 in
    ascending order, the int32 volume that holds i + 1 where labels == ids[i]
    and 0 where labels == 0, and len(ids) + 1.  All on labels' device."""
    values, inverse = torch.unique(labels, return_inverse=True)
    cell = values != 0
    rank = torch.cumsum(cell, 0) * cell          # 0 for the background, 1.. for the cells
    dense = rank.to(torch.int32)[inverse].contiguous()
    ids = values[cell]
    return ids, dense, int(ids.numel()) + 1


def _channels(image, device):
    """(tensor [C,X,Y,Z] on the device whose channel volumes are contiguous,
    channel stride): a channel slice of a wider tensor is used in place."""
    t = image[0].to(device)
    X, Y, Z = (int(s) for s in t.shape[1:])
    if tuple(t.stride()[1:]) != (Y * Z, Z, 1) or (t.shape[0] > 1 and t.stride(0) < X * Y * Z):
        t = t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else X * Y * Z)


def cell_table(image, labels):
    """cell_table(image, labels) -> CellTable of device tensors (module
    docstring).  image [1,C,X,Y,Z] fp32 / fp16 / bf16; labels [X,Y,Z] or
    [1,1,X,Y,Z] of any integer dtype or float64 (pixel_vec_to_cell's); numpy
    arrays, host tensors or device tensors.  Id values are arbitrary."""
    image = _as_tensor(image)
    shape = tuple(int(s) for s in image.shape)
    if len(shape) != 5:
        raise ValueError(f'cell_table: expected a [1,C,X,Y,Z] image, got {shape}')
    if shape[0] != 1:
        raise ValueError(f'cell_table: one volume at a time, got a batch of {shape[0]}')
    if min(shape[1:]) < 1:
        raise ValueError(f'cell_table: empty image {shape}')
    code = _IMAGE_CODES.get(image.dtype)
    if code is None:
        raise TypeError(f'cell_table: the image is fp32, fp16 or bf16, got {image.dtype}')
    C, (X, Y, Z) = shape[1], shape[2:]
    labels = _labels_3d(labels, (X, Y, Z))
    device = _device_of(image, labels)
    ids, dense, n_ids = dense_ids(labels.to(device))
    if n_ids == 1:   # background only: no launch
        def none(dtype, *tail):
            return torch.empty((0,) + tail, dtype=dtype, device=device)
        return CellTable(ids, none(torch.int32, 6), none(torch.int32), none(torch.int32, Z), none(torch.float32),
                         none(torch.float64, C), none(torch.float64, C), none(torch.float32, C, 2))
    t, stride = _channels(image, device)
    boxes = _lib.empty((n_ids, 6), torch.int32, device)
    count = _lib.empty((n_ids,), torch.int32, device)
    plane_count = _lib.empty((n_ids, Z), torch.int32, device)
    box_min = _lib.empty((n_ids,), torch.float32, device)
    mean = _lib.empty((n_ids, C), torch.float64, device)
    std = _lib.empty((n_ids, C), torch.float64, device)
    median = _lib.empty((n_ids, C, 2), torch.float32, device)
    with torch.cuda.device(device):
        stream = _lib.stream_handle(device)
        _lib.check(_lib.lib().hcu_cell_boxes(_lib.ptr(dense), X, Y, Z, n_ids, _lib.ptr(boxes), stream), 'cell_boxes')
        _lib.check(_lib.lib().hcu_cell_stats(_lib.ptr(dense), _lib.ptr(boxes), _lib.ptr(t), code, stride, C, X, Y, Z,
                                             n_ids, _lib.ptr(count), _lib.ptr(plane_count), _lib.ptr(box_min),
                                             _lib.ptr(mean), _lib.ptr(std), _lib.ptr(median), stream), 'cell_stats')
    return CellTable(ids, boxes[1:], count[1:], plane_count[1:], box_min[1:], mean[1:], std[1:], median[1:])


def _to_host(table):
    """The tables as numpy arrays after ONE device-to-host copy: every table
    widened to 8-byte words (int32 and fp32 are exact in float64; the ids
    travel as their own bits) and packed into one buffer."""
    ids = table.ids
    as_bits = ids.dtype != torch.float64
    parts = [ids.to(torch.int64).view(torch.float64) if as_bits else ids]
    parts += [x.to(torch.float64).reshape(-1) for x in table[1:]]
    flat = torch.cat(parts).cpu().numpy()
    out, at = [], 0
    for x in table:
        n = x.numel()
        out.append(flat[at:at + n].reshape(tuple(x.shape)))
        at += n
    host_ids = out[0].view(np.int64).astype(torch.empty(0, dtype=ids.dtype).numpy().dtype) if as_bits else out[0]
    return CellTable(host_ids, out[1].astype(np.int64), out[2].astype(np.int64), out[3].astype(np.int64),
                     out[4].astype(np.float32), out[5], out[6], out[7].astype(np.float32))


def generate_cell_objects(image, unique_mask, cell_candidates, x_ind_chunk, y_ind_chunk):
    """generate_cell_objects(image, unique_mask, cell_candidates, x_ind_chunk,
    y_ind_chunk) -> [HairCell], one per id of unique_mask other than 0 in
    ascending order.  image [1,C,X,Y,Z] with C >= 4; unique_mask [X,Y,Z] or
    [1,1,X,Y,Z]; cell_candidates is ignored, as in the reference."""
    if len(image.shape) == 5 and image.shape[1] < len(CHANNELS):
        raise IndexError(f'generate_cell_objects: the image has {image.shape[1]} channels, '
                         f'a cell reads {len(CHANNELS)}')
    t = _to_host(cell_table(image, unique_mask))
    cells = []
    for i, id in enumerate(t.ids):
        x0, y0, z0, x1, y1, z1 = t.boxes[i]
        center = [(x0 + (x1 - x0) / 2) + x_ind_chunk, y0 + ((y1 - y0) / 2) + y_ind_chunk, (z1 - z0) / 2]
        cells.append(HairCell.from_table([x0, y0, z0, x1, y1, z1], center, id, t.count[i], t.plane_count[i],
                                         t.mean[i], t.std[i], t.median[i]))
    return cells
