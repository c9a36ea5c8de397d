"""Drop-in hcat.segment.pixel_vec_to_cell and hist3d: RDCNet's vector field
turned into instance labels on the device (csrc/instances.hip).  The inverse
of VectorToCenter: every voxel votes for the centre it points at, the smoothed
votes' local maxima are the cells, and every voxel takes the cell its own vote
lies nearest to.

  pixel_vec_to_cell  hcat/segment.py:563-628   label volume, float64 [X,Y,Z]
  hist3d             :631-658                  normalised vote volume, float64 [X,Y,Z]

Stage by stage (v = vector[0], channels reversed as :591-593 do):

  1. votes (:590-593, :640-658)  c = (x + v[2], y + v[1], z + v[0]) in fp32;
     ind = floor(c); the vote is dropped unless 0 <= ind < shape on every
     axis (compared as floats, so a NaN or Inf component drops it: the
     reference's int(nan) there is undefined); count[ind] += 1; hist =
     (1 + count) / (1 + max count) in float64, one division.
  2. maximum_filter(hist, size=2, mode='constant') (:602)  the maximum over
     the offsets {-1,0}^3; outside reads 0 and never wins (hist > 0).  Taken
     on the integer counts: the maximum commutes with the normalisation.
  3. skimage.filters.gaussian(., sigma=5) (:603)  scipy's gaussian_filter,
     mode='nearest', truncate 4 (radius 20, 41 taps), float64, axes 0, 1, 2.
     The weights are computed here with scipy's expression (gaussian_weights)
     and each pass sums in the order of scipy's symmetric correlate1d: centre
     term first, then the pairs from the outermost inwards.
  4. peak_local_max(., min_distance=1, num_peaks=100) (:605)  a candidate
     equals the maximum of its 3x3x3 neighbourhood, is > min(h) and lies off
     the outermost layer of every axis (device); candidates by descending
     value, ties in C order, one within Chebyshev distance 1 of an earlier
     kept one dropped, the first num_peaks kept (select_peaks, here).  This
     stage restates skimage, which is not a dependency; `peaks=` replaces it.
  5. labels (:609-626)  d = sqrt((c0-p0)^2 + (c1-p1)^2 + (c2-p2)^2) in fp32;
     peak i wins where d is strictly below the running minimum, which starts
     at 100000; a NaN distance never wins; label = 0 where float(mask) < 0.2.

QUIRK kept from the reference: peak 0 is labelled 0, the background's value
(:609, :620), so the first cell cannot be told from background.  The default
label_offset=0 reproduces that bit for bit; label_offset=1 gives cell i the
label i + 1.

Added keywords: as_tensor=True returns the float64 device tensor without a
host copy; peaks= an integer [n,3] array (n <= num_peaks) used instead of
stage 4, e.g. skimage's own peak_local_max result; num_peaks, sigma
(radius int(4 * sigma + 0.5) <= 20), label_offset.  The reference's two shape
prints are dropped, its count line is kept.  A batch other than 1 raises
ValueError (the reference's squeeze(0) then fails on a shape mismatch).

Whole stacks (no counterpart in the reference, whose RDCNet code only ever
sees one training crop): windows() cuts a stack into cores with clipped halos,
stitch_vec_to_cell runs stages 1-4 per window and hcu_vec_label_paste, which
fuses stage 5 with the renumbering to stack-wide ids and the write into one
int32 label volume (the rule: stitch_vec_to_cell's docstring);
paste_window is the per-window step hcunet_amd.segment.predict_instance_mask
shares.
"""
import ctypes

import numpy as np
import torch

from . import _lib

NUM_PEAKS = 100            # :605
CANDIDATE_ROOM = 1 << 16   # first size of the candidate list; grown when the device reports more

_VEC_CODES = {torch.float32: _lib.HCU_F32, torch.float16: _lib.HCU_F16, torch.bfloat16: _lib.HCU_BF16}
_MASK_CODES = {torch.uint8: _lib.HCU_U8, torch.bool: _lib.HCU_U8, torch.float32: _lib.HCU_F32,
               torch.float16: _lib.HCU_F16, torch.bfloat16: _lib.HCU_BF16, torch.float64: _lib.HCU_F64}


def gaussian_weights(sigma, truncate=4.0):
    """(float64 [2r+1], r): scipy.ndimage's Gaussian kernel of order 0,
    exp(-0.5 / sigma^2 * k^2) over k = -r..r divided by its sum, r =
    int(truncate * sigma + 0.5)."""
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / (sd * sd) * x ** 2)
    return phi_x / phi_x.sum(), radius


def select_peaks(index, value, shape, num_peaks=NUM_PEAKS):
    """The host half of stage 4: int64 [n,3] from a candidate list in any
    order (linear indices into `shape`, their values)."""
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    value = np.asarray(value, dtype=np.float64).reshape(-1)
    order = np.lexsort((index, -value))   # by (-value, index): the stable sort of the C-ordered list
    coords = np.stack(np.unravel_index(index[order], shape), axis=1).reshape(-1, 3)
    kept = np.zeros((0, 3), dtype=np.int64)
    for c in coords:
        if len(kept) >= num_peaks:
            break
        if len(kept) == 0 or np.abs(kept - c).max(axis=1).min() > 1:
            kept = np.concatenate([kept, c[None].astype(np.int64)])
    return kept


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.device.type == 'cuda':
            return x.device
    return torch.device('cuda', torch.cuda.current_device())


def _as_tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def _field_shape(vector, what):
    """Host checks of a [1,3,X,Y,Z] field; the [X,Y,Z] shape."""
    shape = tuple(int(s) for s in vector.shape)
    if len(shape) != 5 or shape[1] != 3:
        raise ValueError(f'{what}: expected a [1,3,X,Y,Z] vector field, got {shape}')
    if shape[0] != 1:
        raise ValueError(f'{what}: one volume at a time, got a batch of {shape[0]}')
    if min(shape[2:]) < 1:
        raise ValueError(f'{what}: empty volume {shape}')
    return shape[2:]


def _planes(v3, device, what):
    """(tensor [3,X,Y,Z] on the device whose channel planes are contiguous,
    dtype code, channel stride): a channel slice of a contiguous network
    output is used in place."""
    t = _as_tensor(v3)
    if t.dtype == torch.float64:
        t = t.float()
    code = _VEC_CODES.get(t.dtype)
    if code is None:
        raise TypeError(f'{what}: the vector field is fp32, fp16 or bf16, got {t.dtype}')
    t = t.to(device)
    X, Y, Z = (int(s) for s in t.shape[1:])
    if tuple(t.stride()[1:]) != (Y * Z, Z, 1) or t.stride(0) < X * Y * Z:
        t = t.contiguous()
    return t, code, int(t.stride(0))


class _Votes:
    """The zeroed counters of one call: counts [X*Y*Z] and the maximum, one
    int32 buffer (torch.zeros: zero is their contract, hcu_vec_votes adds)."""

    def __init__(self, t, code, stride, points=False):
        self.shape = tuple(int(s) for s in t.shape[1:])
        self.device = t.device
        n = self.shape[0] * self.shape[1] * self.shape[2]
        self.buf = torch.zeros(n + 1, dtype=torch.int32, device=t.device)
        self.counts, self.top = self.buf[:n], self.buf[n:]
        X, Y, Z = self.shape
        with torch.cuda.device(t.device):
            _lib.check(_lib.lib().hcu_vec_votes(_lib.ptr(t), code, stride, int(points), X, Y, Z,
                                                _lib.ptr(self.counts), _lib.ptr(self.top),
                                                _lib.stream_handle(t.device)), 'vec_votes')

    def hist(self):
        X, Y, Z = self.shape
        out = _lib.empty(self.shape, torch.float64, self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hcu_vote_hist(_lib.ptr(self.counts), _lib.ptr(self.top), X, Y, Z,
                                                _lib.ptr(out), _lib.stream_handle(self.device)), 'vote_hist')
        return out

    def smooth(self, sigma):
        X, Y, Z = self.shape
        w, radius = gaussian_weights(sigma)
        half = np.ascontiguousarray(w[:radius + 1])
        out = _lib.empty(self.shape, torch.float64, self.device)
        scratch = _lib.empty(self.shape, torch.float64, self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().hcu_vote_smooth(
                _lib.ptr(self.counts), _lib.ptr(self.top), X, Y, Z,
                half.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), radius, _lib.ptr(out), _lib.ptr(scratch),
                _lib.stream_handle(self.device)), 'vote_smooth')
        return out


def smooth_f64(volume, sigma=5):
    """Stage 3 alone: the Gaussian of a float64 [X,Y,Z] device tensor."""
    _lib.require_device(volume, 'smooth_f64 volume')
    if volume.dtype != torch.float64 or volume.dim() != 3:
        raise ValueError('smooth_f64: expected a float64 [X,Y,Z] tensor')
    volume = volume.contiguous()
    X, Y, Z = (int(s) for s in volume.shape)
    w, radius = gaussian_weights(sigma)
    half = np.ascontiguousarray(w[:radius + 1])
    out, scratch = _lib.empty_like(volume), _lib.empty_like(volume)
    with torch.cuda.device(volume.device):
        _lib.check(_lib.lib().hcu_smooth_f64(
            _lib.ptr(volume), X, Y, Z, half.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), radius,
            _lib.ptr(out), _lib.ptr(scratch), _lib.stream_handle(volume.device)), 'smooth_f64')
    return out


def peak_candidates(h, capacity=CANDIDATE_ROOM, grow=True):
    """The device half of stage 4 on a float64 [X,Y,Z] device tensor: (linear
    indices int64, values float64) on the host, in no particular order.  The
    list is sized by `capacity`; when the device finds more, grow=True sizes
    it to what was found and repeats, grow=False raises RuntimeError."""
    _lib.require_device(h, 'peak_candidates volume')
    h = h.contiguous()
    X, Y, Z = (int(s) for s in h.shape)
    found = ctypes.c_int(0)
    while True:
        index = _lib.empty((capacity,), torch.int32, h.device)
        value = _lib.empty((capacity,), torch.float64, h.device)
        state = _lib.empty((2,), torch.int64, h.device)
        with torch.cuda.device(h.device):
            rc = _lib.lib().hcu_peak_candidates(_lib.ptr(h), X, Y, Z, _lib.ptr(index), _lib.ptr(value), capacity,
                                                _lib.ptr(state), ctypes.byref(found), _lib.stream_handle(h.device))
        if rc == _lib.HCU_ERR_WORKSPACE and grow:
            capacity = int(found.value)
            continue
        _lib.check(rc, 'peak_candidates')
        n = int(found.value)
        return index[:n].cpu().numpy().astype(np.int64), value[:n].cpu().numpy()


def vec_label(t, code, stride, peaks, mask, label_offset=0):
    """Stage 5 on the planes of _planes(): float64 [X,Y,Z] device tensor."""
    X, Y, Z = (int(s) for s in t.shape[1:])
    peaks = np.ascontiguousarray(np.asarray(peaks).reshape(-1, 3), dtype=np.int32)
    n = len(peaks)
    table = torch.from_numpy(peaks).to(t.device) if n else None
    mcode = 0
    if mask is not None:
        mcode = _MASK_CODES.get(mask.dtype)
        if mcode is None:
            raise TypeError(f'pixel_vec_to_cell: the mask is bool, uint8 or floating, got {mask.dtype}')
        mask = mask.to(t.device).contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
    label = _lib.empty((X, Y, Z), torch.float64, t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().hcu_vec_label(_lib.ptr(t), code, stride, X, Y, Z, _lib.ptr(table), n,
                                            _lib.ptr(mask), mcode, int(label_offset), _lib.ptr(label),
                                            _lib.stream_handle(t.device)), 'vec_label')
    return label


def vote_counts(vector3):
    """Stage 1 alone: int32 [X,Y,Z] device tensor of votes per voxel of a
    [3,X,Y,Z] field."""
    t, code, stride = _planes(vector3, _device_of(vector3), 'vote_counts')
    v = _Votes(t, code, stride)
    return v.counts.view(v.shape)


def smoothed_votes(vector3, sigma=5):
    """Stages 1-3: float64 [X,Y,Z] device tensor."""
    t, code, stride = _planes(vector3, _device_of(vector3), 'smoothed_votes')
    return _Votes(t, code, stride).smooth(sigma)


def hist3d(mat):
    """hist3d(mat) -> float64 [X,Y,Z]: `mat` [3,X,Y,Z] holds one point (c0,
    c1, c2) per voxel; each point inside the volume adds 1 to the voxel
    floor(c), and the result is (1 + count) / (1 + max count).  A numpy array
    gives a numpy array, a tensor a device tensor."""
    if len(mat.shape) != 4 or mat.shape[0] != 3:
        raise ValueError(f'hist3d: expected a [3,X,Y,Z] array, got {tuple(mat.shape)}')
    t, code, stride = _planes(mat, _device_of(mat), 'hist3d')
    v = _Votes(t, code, stride, points=True)
    out = v.hist()
    return out if isinstance(mat, torch.Tensor) else out.cpu().numpy()


def _check_mask(mask, shape, what):
    mask = _as_tensor(mask)
    if mask.dim() == 5:
        mask = mask[0, 0]
    if tuple(int(s) for s in mask.shape) != shape:
        raise ValueError(f'{what}: mask {tuple(mask.shape)} does not match the volume {shape}')
    if mask.dtype not in _MASK_CODES:
        raise TypeError(f'{what}: the mask is bool, uint8 or floating, got {mask.dtype}')
    return mask


def windows(shape, tile, halo):
    """The windows of a tiled stack `shape` = (X, Y, Z), a list of dicts with
    core_lo, core_hi, lo, hi (3-tuples, half-open).  On every axis the cores
    are [k * tile, min((k + 1) * tile, n)), a partition; a window is its core
    grown by `halo` on both sides and clipped to [0, n) (clipped, not
    reflected: a mirrored halo would hold mirror-image cells).  tile[a] None:
    the whole axis.  x is the slowest index of the list and z the fastest;
    this is the order of the launches and of the ids."""
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or len(tile) != 3 or len(halo) != 3:
        raise ValueError('windows: shape, tile and halo have three entries each')
    if min(shape) < 1:
        raise ValueError(f'windows: empty volume {shape}')
    axes = []
    for n, t, h in zip(shape, tile, halo):
        t = n if t is None else int(t)
        h = int(h)
        if t <= 0:
            raise ValueError(f'windows: tile sizes are positive, got {tuple(tile)}')
        if h < 0:
            raise ValueError(f'windows: halos are not negative, got {tuple(halo)}')
        axes.append([(c, min(c + t, n), max(c - h, 0), min(min(c + t, n) + h, n)) for c in range(0, n, t)])
    return [dict(core_lo=(x[0], y[0], z[0]), core_hi=(x[1], y[1], z[1]), lo=(x[2], y[2], z[2]),
                 hi=(x[3], y[3], z[3])) for x in axes[0] for y in axes[1] for z in axes[2]]


def vote_bounds(window, shape):
    """Rule (d) of the stitch as six floats {lo0, hi0, lo1, hi1, lo2, hi2}:
    floor(c) of a written voxel keeps one voxel off every face of the window
    that is not a face of the volume; a face of the volume is open (+-Inf)."""
    out = []
    for a in range(3):
        w = window['hi'][a] - window['lo'][a]
        out += [1.0 if window['lo'][a] > 0 else -np.inf, float(w - 1) if window['hi'][a] < shape[a] else np.inf]
    return np.array(out, dtype=np.float32)


def owned_ids(peaks, window, first_id):
    """(int32 [n] ids, int64 [m,3] stack-wide positions of the owned peaks):
    a peak is owned when window lo + peak lies inside the window's core; owned
    peaks take first_id, first_id + 1, ... in peak order, the others 0."""
    pos = np.asarray(peaks, dtype=np.int64).reshape(-1, 3) + np.asarray(window['lo'], dtype=np.int64)
    own = np.all((pos >= np.asarray(window['core_lo'])) & (pos < np.asarray(window['core_hi'])), axis=1)
    ids = np.zeros(len(pos), dtype=np.int32)
    ids[own] = first_id + np.arange(int(own.sum()), dtype=np.int32)
    return ids, pos[own]


def paste_window(t, code, stride, mask, window, labels, first_id, sigma=5, num_peaks=NUM_PEAKS):
    """One window of the stitch: stages 1-4 on the window's planes (_planes()),
    then paste_peaks."""
    wshape = tuple(int(s) for s in t.shape[1:])
    h = _Votes(t, code, stride).smooth(sigma)
    peaks = select_peaks(*peak_candidates(h), wshape, num_peaks)
    return paste_peaks(t, code, stride, mask, peaks, window, labels, first_id)


def paste_peaks(t, code, stride, mask, peaks, window, labels, first_id):
    """hcu_vec_label_paste of one window into `labels` (int32 [X,Y,Z] device
    tensor of the whole stack).  t, code, stride: the window's planes
    (_planes()); mask: the window's, a contiguous device tensor; peaks: the
    window's, int [n,3] in window-local coordinates.  Returns the stack-wide
    positions of the peaks this window owns, int64 [m,3]; their ids are
    first_id .. first_id + m - 1."""
    wshape = tuple(int(s) for s in t.shape[1:])
    ids, centres = owned_ids(peaks, window, first_id)
    n = len(peaks)
    if not ids.any():
        return centres          # no peak of this window's own: nothing would be written
    table = _lib.empty((4 * n,), torch.int32, t.device)   # the peaks [n,3], then their ids [n]
    table.copy_(torch.from_numpy(np.concatenate([peaks.astype(np.int32).reshape(-1), ids])))
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    bounds = vote_bounds(window, tuple(int(s) for s in labels.shape))
    X, Y, Z = wshape
    DX, DY, DZ = (int(s) for s in labels.shape)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().hcu_vec_label_paste(
            _lib.ptr(t), code, stride, X, Y, Z, _lib.ptr(table), _lib.ptr(table[3 * n:]), n, _lib.ptr(mask),
            _MASK_CODES[mask.dtype], bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _lib.ptr(labels),
            DX, DY, DZ, *window['lo'], _lib.stream_handle(t.device)), 'vec_label_paste')
    return centres


def stitch_vec_to_cell(vector, mask, *, tile, halo, sigma=5, num_peaks=NUM_PEAKS, as_tensor=False):
    """Instance labels of a whole stack from its vector field, window by
    window: (labels int32 [X,Y,Z], centres int64 [n,3]); row g - 1 of centres
    is the stack-wide position of id g.  vector [1,3,X,Y,Z] and mask as
    pixel_vec_to_cell takes them, on the host or the device; as_tensor=True
    returns the labels as a device tensor.

    For each window of windows(shape, tile, halo), in order: stages 1-4 of
    pixel_vec_to_cell on the window's crop (window-local coordinates; sigma
    and num_peaks are per window); a peak is owned by the window whose core
    holds it and owned peaks take consecutive ids from 1; a voxel is written
    with its nearest peak's id where a peak won, float(mask) >= 0.2, the id is
    not 0 and floor of its own vote keeps one voxel off every interior face of
    the window (vote_bounds: the layer where no peak is ever reported); a
    later window overwrites an earlier one, unwritten voxels stay 0.  One
    window over the whole volume gives int32(pixel_vec_to_cell(...,
    label_offset=1)).  A cell is whole only if it fits into core + halo of the
    window that owns it; a peak that two windows place in different cores is
    doubled or lost."""
    what = 'stitch_vec_to_cell'
    shape = _field_shape(vector, what)
    mask = _check_mask(mask, shape, what)
    wins = windows(shape, tile, halo)
    device = _device_of(vector, mask)
    v = _as_tensor(vector)[0]
    if v.dtype == torch.float64:
        v = v.float()
    if v.dtype not in _VEC_CODES:
        raise TypeError(f'{what}: the vector field is fp32, fp16 or bf16, got {v.dtype}')
    v, mask = v.to(device), mask.to(device)
    labels = torch.zeros(shape, dtype=torch.int32, device=device)
    centres = []
    count = 0
    for w in wins:
        box = tuple(slice(a, b) for a, b in zip(w['lo'], w['hi']))
        wshape = tuple(b - a for a, b in zip(w['lo'], w['hi']))
        crop = _lib.empty((3,) + wshape, v.dtype, device)
        crop.copy_(v[(slice(None),) + box])
        mcrop = _lib.empty(wshape, mask.dtype, device)
        mcrop.copy_(mask[box])
        t, code, stride = _planes(crop, device, what)
        got = paste_window(t, code, stride, mcrop, w, labels, count + 1, sigma, num_peaks)
        centres.append(got)
        count += len(got)
    print(f'Predicted {count} cell from runet output')
    centres = np.concatenate(centres).reshape(-1, 3) if centres else np.zeros((0, 3), dtype=np.int64)
    return (labels if as_tensor else labels.cpu().numpy()), centres


def pixel_vec_to_cell(vector, mask, *, as_tensor=False, peaks=None, num_peaks=NUM_PEAKS, sigma=5,
                      label_offset=0):
    """pixel_vec_to_cell(vector, mask) -> float64 [X,Y,Z]: the index of the
    cell each voxel belongs to (module docstring).  vector [1,3,X,Y,Z] fp32 /
    fp16 / bf16, mask [1,1,X,Y,Z] or [X,Y,Z] bool / uint8 / floating, on the
    host or the device."""
    shape = _field_shape(vector, 'pixel_vec_to_cell')
    mask = _check_mask(mask, shape, 'pixel_vec_to_cell')
    if peaks is not None:
        peaks = np.asarray(peaks)
        if peaks.ndim != 2 or peaks.shape[1] != 3 or peaks.dtype.kind not in 'iu':
            raise ValueError('pixel_vec_to_cell: peaks is an integer [n,3] array')
        if len(peaks) > num_peaks:
            raise ValueError(f'pixel_vec_to_cell: {len(peaks)} peaks, num_peaks is {num_peaks}')
    device = _device_of(vector, mask)
    t, code, stride = _planes(_as_tensor(vector)[0], device, 'pixel_vec_to_cell')
    if peaks is None:
        h = _Votes(t, code, stride).smooth(sigma)
        peaks = select_peaks(*peak_candidates(h), shape, num_peaks)
    print(f'Predicted {len(peaks)} cell from runet output')
    label = vec_label(t, code, stride, peaks, mask, label_offset)
    return label if as_tensor else label.cpu().numpy()
