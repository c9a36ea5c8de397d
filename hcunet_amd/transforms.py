"""Drop-in hcat.transforms for the input path: to_float,
reshape, normalize and to_tensor, and the reference's crop, rotation and
intensity augmentations -- random_crop, nul_crop, random_rotate,
random_intensity, drop_channel, clean_image, remove_channel, random_gamma,
spekle -- with the reference's names, constructor signatures, call convention (joint lists through
`joint_transform`, which also draws the reference's per-call numpy seed,
hcat/transforms.py:15-91), exception types and draws from numpy's global RNG
in the reference's order.

The MI355X path is lazy: a transform only records on the `PendingVolume` what
it would do to the raw stack -- a window or keep list per axis, a channel
selection, at most one nearest-neighbour rotation in the (x, y) plane, and an
ordered program of at most 8 per-voxel steps -- and
to_tensor runs the whole chain of every volume it is given as ONE device pass
(csrc/augment.hip, `hcu_ingest_jobs`): the window of the raw uint16 / uint8
stack is read from HBM, scaled, transposed [Z,Y,X,C] -> [C,X,Y,Z], run through
the program in float64 in recorded order and rounded once to fp16.  The result
is bit-identical to the reference's eager chain wherever that is deterministic
given numpy's RNG, with two documented exceptions:

* `spekle` draws ONE integer from numpy's stream as a key and generates its
  normal noise on the device with a counter-based generator (Philox-4x32-10,
  Box-Muller in float64, rounded to float32 as the reference's
  np.float32(noise)).  Same distribution, deterministic given the numpy seed,
  but not the reference's per-voxel np.random.normal stream -- the one place
  where the RNG stream departs from the reference.
* `random_gamma` is pinned to numpy's float64 power, v ** factor, which is
  what skimage.exposure.adjust_gamma computes for a float image (scale 1,
  gain 1); scikit-image itself was not available to pin against, and the
  device's float64 pow may differ from the host's in the last bit.

`random_rotate` is scipy.ndimage.rotate(order=0, mode='constant',
reshape=False) restated (`rotate_nearest`): float64 source coordinates with
every product and sum rounded on its own, scipy.special's cosdg / sindg (the
360 integer angles from the committed table cosdg_sindg.txt), zeros outside.
The device gathers with the same arithmetic, so it is bit-identical too.  The
package does not import scipy.ndimage; only a non-integer angle imports
scipy.special.

Whatever the device program cannot hold (a float64 or 2-D image, a ninth step,
random_gamma after normalize, a rotation before reshape or to_float, a second
rotation, nul_crop after a rotation, ...) runs on the host exactly as the reference's
numpy code would: `PendingVolume.to_ndarray()` restates every recorded step
eagerly, taking the window from the raw stack before converting.  Steps are
never reordered.

Reference: to_float hcat/transforms.py:94-116, to_tensor :118-137,
reshape :139-157, spekle :159-183, random_gamma :186-197, normalize :257-283,
drop_channel :285-298, random_intensity :301-334, random_crop :337-396,
random_affine :200-227 (its constructor raises), random_rotate :230-254,
nul_crop :460-489, remove_channel :590-613, clean_image :616-631.
elastic_deform and the Faster-RCNN box transforms of that file are not
provided.
"""
import copy
import ctypes
import functools
import os

import numpy as np
import torch

from . import _lib

_RAW = {np.dtype(np.uint16): _lib.HCU_U16, np.dtype(np.uint8): _lib.HCU_U8,
        np.dtype(np.float64): _lib.HCU_F64}
_TORCH_RAW = {torch.uint16: _lib.HCU_U16, torch.int16: _lib.HCU_U16, torch.uint8: _lib.HCU_U8,
              torch.float64: _lib.HCU_F64}
_INT_CODES = (_lib.HCU_U16, _lib.HCU_U8)

NORMALIZE, INTENSITY, DROP, CLEAN, GAMMA, SPEKLE = (_lib.AUG_NORMALIZE, _lib.AUG_INTENSITY, _lib.AUG_DROP,
                                                    _lib.AUG_CLEAN, _lib.AUG_GAMMA, _lib.AUG_SPEKLE)


class Step:
    """One per-voxel step of a volume's program: kind, per-channel float64
    operands a / b (indexed by the volume's current channels), noise key."""

    def __init__(self, kind, a=None, b=None, key=0):
        self.kind, self.a, self.b, self.key = kind, a, b, key


class Rotation:
    """A recorded random_rotate: cosine and sine of the angle, the extents
    (nx, ny) of the view it rotated, the number of per-voxel steps recorded
    before it, and the window (px, py, ox, oy) that later crops left of the
    rotated view."""

    def __init__(self, c, s, nx, ny, after):
        self.c, self.s, self.nx, self.ny, self.after = c, s, nx, ny, after
        self.px, self.py, self.ox, self.oy = 0, 0, nx, ny


def rotation_terms(c, s, nx, ny):
    """scipy.ndimage.rotate's matrix [[c, s], [-s, c]] and offset
    centre - matrix @ centre (float64, numpy's matmul as scipy calls it) for an
    (nx, ny) plane rotated about its centre without reshaping."""
    m = np.array([[c, s], [-s, c]], dtype=np.float64)
    centre = (np.array([nx, ny]) - 1) / 2
    return m, centre - m @ centre


def rotate_nearest(a, c, s):
    """scipy.ndimage.rotate(a, axes=(0, 1), reshape=False, order=0,
    mode='constant', prefilter=False) of the float array a for the angle whose
    cosdg / sindg are c / s: output (u, v) takes input (floor(cx + .5),
    floor(cy + .5)), cx = (u c + v s) + off_x, cy = (u (-s) + v c) + off_y with
    each product and sum rounded on its own, when 0 <= cx <= nx - 1 and
    0 <= cy <= ny - 1, else 0."""
    nx, ny = a.shape[:2]
    m, off = rotation_terms(c, s, nx, ny)
    u = np.arange(nx, dtype=np.float64)[:, None]
    v = np.arange(ny, dtype=np.float64)[None, :]
    cx = (u * m[0, 0] + v * m[0, 1]) + off[0]
    cy = (u * m[1, 0] + v * m[1, 1]) + off[1]
    inside = (cx >= 0) & (cx <= nx - 1) & (cy >= 0) & (cy <= ny - 1)
    ix = np.where(inside, np.floor(cx + 0.5), 0).astype(np.intp)
    iy = np.where(inside, np.floor(cy + 0.5), 0).astype(np.intp)
    out = a[ix, iy]
    out[~inside] = 0
    return out


_COS_SIN = None


def cos_sin(angle):
    """(scipy.special.cosdg(angle), sindg(angle)) as float64: the integer
    angles 0..359 from the committed table (cosdg_sindg.txt, written by
    make_cosdg_sindg.py; numpy's cos(deg2rad()) differs in the last bit for
    most of them), any other angle from scipy.special itself."""
    global _COS_SIN
    if float(angle).is_integer() and 0 <= angle < 360:
        if _COS_SIN is None:
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cosdg_sindg.txt')) as f:
                rows = [ln.split() for ln in f if ln.strip() and not ln.startswith('#')]
            _COS_SIN = [(float.fromhex(r[1]), float.fromhex(r[2])) for r in rows]
        return _COS_SIN[int(angle)]
    try:
        from scipy import special
    except ImportError as e:
        raise ImportError('random_rotate needs scipy (scipy.special.cosdg / sindg) for an angle that is not one '
                          f'of the integers 0..359: {angle}') from e
    return float(special.cosdg(angle)), float(special.sindg(angle))


class PendingVolume:
    """A raw [Z,Y,X,C] (or [Y,X,C]) stack plus the recorded steps, materialised
    by to_tensor on the device: to_float / reshape flags, per raw axis a window
    (start, n) or an int32 keep list, a channel selection, at most one
    `Rotation` of the (x, y) plane and the program.  With a rotation the
    windows / keep lists of x and y describe the view BEFORE it; crops recorded
    after it move the window (px, py, ox, oy) inside the rotated view."""

    def __init__(self, raw, np_dtype=None, source=None):
        self.raw = raw
        self.np_dtype = np_dtype   # dtype of the file's array when raw holds its bits
        self.source = source       # the dataloader's stack record (device residency, keep-list cache)
        self.to_float = False
        self.reshaped = False
        self.mean = None
        self.std = None
        self.sel = [None] * (raw.ndim - 1)   # per raw spatial axis: None (all), (start, n) or int32 array
        self.chan = None                     # source channel of each current channel, or None (all)
        self.steps = []
        self.rot = None                      # a Rotation, or None

    @property
    def ndim(self):  # joint_transform compares ndim across the list (:67-72)
        return self.raw.ndim

    def _raw_shape(self):
        s = list(self.raw.shape)
        for i, w in enumerate(self.sel):
            if w is not None:
                s[i] = w[1] if isinstance(w, tuple) else len(w)
        if self.chan is not None:
            s[-1] = len(self.chan)
        return tuple(s)

    @property
    def shape(self):
        s = self._raw_shape()
        if self.reshaped:
            s = (s[-2],) + s[1:-2] + (s[0], s[-1])
        if self.rot is not None:   # (recorded only on a reshaped [Z,Y,X,C] stack)
            s = (self.rot.ox, self.rot.oy) + s[2:]
        return s

    def uncropped(self):
        return all(w is None for w in self.sel)

    def _raw_axis(self, axis):
        """The raw axis behind axis `axis` of the current view (reshape swaps
        axis 0 with axis ndim - 2)."""
        if self.reshaped:
            last = self.raw.ndim - 2
            return last if axis == 0 else (0 if axis == last else axis)
        return axis

    def take(self, axis, start=None, n=None, keep=None):
        """Record a window [start, start + n) or the keep list `keep` (indices
        into the current view) along axis `axis` of the current view.  After a
        rotation a window along x or y moves inside the rotated view."""
        if self.rot is not None and axis in (0, 1):
            if keep is not None:
                raise NotImplementedError('a keep list after a rotation (nul_crop takes the host path)')
            if axis == 0:
                self.rot.px, self.rot.ox = self.rot.px + int(start), int(n)
            else:
                self.rot.py, self.rot.oy = self.rot.py + int(start), int(n)
            return
        r = self._raw_axis(axis)
        old = self.sel[r]
        if keep is not None:
            keep = np.asarray(keep, dtype=np.int64)
            if old is None:
                new = keep
            elif isinstance(old, tuple):
                new = old[0] + keep
            else:
                new = old[keep]
            self.sel[r] = np.ascontiguousarray(new, dtype=np.int32)
        else:
            if old is None:
                self.sel[r] = (int(start), int(n))
            elif isinstance(old, tuple):
                self.sel[r] = (old[0] + int(start), int(n))
            else:
                self.sel[r] = np.ascontiguousarray(old[int(start):int(start) + int(n)])

    def select_channels(self, index):
        index = [int(i) for i in index]
        C = self.shape[-1]
        index = [i + C if i < 0 else i for i in index]
        if any(i < 0 or i >= C for i in index):
            raise IndexError(f'index {index} is out of bounds for axis with size {C}')
        cur = list(range(C)) if self.chan is None else self.chan
        self.chan = [cur[i] for i in index]
        for st in self.steps:   # the operands follow their channels
            st.a = None if st.a is None else [st.a[i] for i in index]
            st.b = None if st.b is None else [st.b[i] for i in index]
        if self.mean is not None:
            self.mean = [self.mean[i] for i in index]
            self.std = [self.std[i] for i in index]

    def raw_ndarray(self):
        """The raw stack as the file's ndarray (no copy of a host tensor)."""
        raw = self.raw
        if isinstance(raw, torch.Tensor):
            a = raw.detach().cpu().numpy()
            if self.np_dtype is not None and np.dtype(self.np_dtype) != a.dtype:
                a = a.view(self.np_dtype)
            elif raw.dtype == torch.int16:
                a = a.view(np.uint16)
            return a
        return np.asarray(raw)

    def windowed_raw(self):
        """The window, keep lists and channel selection applied to the raw stack."""
        a = self.raw_ndarray()
        for i, w in enumerate(self.sel):
            if isinstance(w, tuple):
                a = a[(slice(None),) * i + (slice(w[0], w[0] + w[1]),)]
            elif w is not None:
                a = np.take(a, w, axis=i)
        if self.chan is not None:
            a = a[..., self.chan]
        return a

    def to_ndarray(self):
        """The ndarray the reference's eager chain would hold at this point
        (host numpy, same arithmetic: to_float :104-115, reshape :139-156, the
        crops' indexing and every recorded step as the reference's own numpy
        code), for transforms that need a real array (the reference's random
        augmentations check isinstance(image, np.ndarray)).  The window is taken
        from the raw stack before converting.  A recorded device spekle step is
        restated with numpy normals from a generator seeded with its key.
        A recorded rotation (`self.rot`: c, s, nx, ny, after, px, py, ox, oy) is
        restated by `rotate_nearest` on the (nx, ny) view after the first
        `after` steps, cut to its window [px, px + ox) x [py, py + oy), and
        followed by the remaining steps."""
        a = self.windowed_raw()
        if self.to_float and a.dtype == np.uint16:
            a = a.astype(np.float64) / 2 ** 16
        elif self.to_float and a.dtype == np.uint8:
            a = a.astype(np.float64) / 2 ** 8
        else:
            a = a.copy()
        if self.reshaped:
            a = a.swapaxes(a.ndim - 2, 0)
        if self.steps:
            a = np.ascontiguousarray(a)
        R = self.rot
        for st in self.steps[:len(self.steps) if R is None else R.after]:
            a = _eager_step(a, st)
        if R is not None:
            a = rotate_nearest(a, R.c, R.s)[R.px:R.px + R.ox, R.py:R.py + R.oy]
            if len(self.steps) > R.after:
                a = np.ascontiguousarray(a)
            for st in self.steps[R.after:]:
                a = _eager_step(a, st)
        return a

    def _dtype_code(self):
        if self.np_dtype is not None:
            return _RAW.get(np.dtype(self.np_dtype))
        if isinstance(self.raw, torch.Tensor):
            code = _TORCH_RAW.get(self.raw.dtype)
        else:
            code = _RAW.get(np.dtype(self.raw.dtype))
        return code

    def recordable(self, need_float=True):
        """Whether a per-voxel step can join the device program: an integer raw
        [Z,Y,X,C] stack (scaled by to_float when the step needs a float image)
        of at most 16 channels, and a free program slot."""
        return (self.raw.ndim == 4 and self._dtype_code() in _INT_CODES and (self.to_float or not need_float)
                and self.shape[-1] <= _lib.INGEST_MAX_C and len(self.steps) < _lib.AUG_MAX_STEPS)

    def non_negative(self):
        """The program so far guarantees values >= 0 (no normalize yet)."""
        return all(st.kind != NORMALIZE for st in self.steps)


def _eager_step(a, st):
    """Step `st` on the float64 ndarray a ([..., C]) as the reference computes it."""
    C = a.shape[-1]
    if st.kind == NORMALIZE:        # :273-279
        for c in range(C):
            a[..., c] += -st.a[c]
            a[..., c] /= st.b[c]
    elif st.kind == INTENSITY:      # :318-332
        for c in range(C):
            if st.b[c]:
                a[..., c] -= st.a[c]
        a[a < 0] = 0
        a[np.isnan(a)] = 0
        a[np.isinf(a)] = 1
    elif st.kind == DROP:           # :297
        for c in range(C):
            if st.a[c]:
                a[..., c] = 0
    elif st.kind == CLEAN:          # :628-629
        a[np.isnan(a)] = 0
        a[np.isinf(a)] = 1
    elif st.kind == GAMMA:          # adjust_gamma on a float image: ((v / 1) ** gamma) * 1 * 1
        a = a ** st.a[0]
    elif st.kind == SPEKLE:         # :177-181
        noise = np.float32(np.random.RandomState(st.key).normal(0, st.a[0], a.shape))
        a = a + noise
        a[a < 0] = 0
        a[a > 1] = 1
    return a


def _wrap(image):
    return image if isinstance(image, PendingVolume) else PendingVolume(image)


def _host(image):
    """The ndarray the reference would hold (host path of a transform)."""
    return image.to_ndarray() if isinstance(image, PendingVolume) else image


def joint_transform(func):
    """hcat/transforms.py:15-91: apply `func(self, image, seed)` to one image or
    to each image of a list with one seed drawn from numpy's global RNG."""
    @functools.wraps(func)
    def wrapper(*args):
        image_list = args[-1]
        if not type(image_list) == list:
            image_list = [image_list]
        if len(image_list) > 1:
            for i in range(len(image_list) - 1):
                if not image_list[i].ndim == image_list[i + 1].ndim:
                    raise ValueError('Images in joint transforms do not contain identical dimensions.'
                                     + f'Im {i}.ndim:{image_list[i].ndim} != Im {i + 1}.ndim:'
                                     f'{image_list[i + 1].ndim} ')
        seed = np.random.randint(0, 1e8, 1)   # :78, keeps numpy's RNG stream aligned
        out = [func(args[0], image=im, seed=seed) if len(args) > 1 else func(image=im, seed=seed)
               for im in image_list]
        return out[0] if len(out) == 1 else out
    return wrapper


class to_float:
    """uint16 / 2**16, uint8 / 2**8, float64 unchanged; other dtypes: TypeError."""

    @joint_transform
    def __call__(self, image, seed=None):
        v = _wrap(image)
        if v.to_float or v.mean is not None:
            return v
        code = v._dtype_code()
        if code is None:
            raise TypeError('Expected image datatype of uint8 or uint16 ')
        v.to_float = True
        return v


class reshape:
    """[Z,Y,X,C] -> [X,Y,Z,C] (swapaxes(ndim - 2, 0))."""

    @joint_transform
    def __call__(self, image, seed=None):
        if not isinstance(image, (np.ndarray, PendingVolume, torch.Tensor)):
            raise TypeError(f'Expected input type of np.ndarray but got {type(image)}')
        v = _wrap(image)
        if v.rot is not None:   # the rotation plane would no longer be raw (X, Y): the rest on the host
            v = PendingVolume(v.to_ndarray())
        if v.reshaped:   # a second swap undoes the first
            v.reshaped = False
        else:
            v.reshaped = True
        return v


class normalize:
    """Per channel (v + -mean) / std on a float image (defaults 0.5 / 0.5)."""

    def __init__(self, mean=None, std=None):
        self.mean = [0.5, 0.5, 0.5, 0.5] if mean is None else mean
        self.std = [0.5, 0.5, 0.5, 0.5] if std is None else std

    def __call__(self, image):
        if isinstance(image, list):   # :268-269: only the first image of a list
            image = image[0]
        v = _wrap(image)
        if v.ndim not in (3, 4):
            raise ValueError(f'Expected a 3 or 4 dimensional image not: {v.ndim} with shape: {v.shape}')
        if not v.to_float and v._dtype_code() != _lib.HCU_F64:
            raise TypeError('normalize expects a float image (apply to_float first)')
        if v.mean is not None:
            raise NotImplementedError('normalize applied twice to one volume')
        C = v.shape[-1]
        mean = [float(self.mean[c]) for c in range(C)]
        std = [float(self.std[c]) for c in range(C)]
        if len(v.steps) >= _lib.AUG_MAX_STEPS:   # the program is full: the rest of the chain on the host
            v = PendingVolume(v.to_ndarray())
        v.mean, v.std = mean, std
        v.steps.append(Step(NORMALIZE, mean, std))
        return v


class to_tensor:
    """[x,y,z,c] -> fp16 [1,c,x,y,z] on the current ROCm device; the volumes of
    a list go through one hcu_ingest_jobs launch."""

    def __call__(self, image_list):
        vols = image_list if type(image_list) == list else [image_list]
        for i in range(len(vols) - 1):   # joint_transform's check and seed draw (:67-78)
            if not vols[i].ndim == vols[i + 1].ndim:
                raise ValueError('Images in joint transforms do not contain identical dimensions.'
                                 + f'Im {i}.ndim:{vols[i].ndim} != Im {i + 1}.ndim:{vols[i + 1].ndim} ')
        np.random.randint(0, 1e8, 1)
        for image in vols:
            if not isinstance(image, (np.ndarray, PendingVolume)):
                raise TypeError(f'Expected list but got {type(image)}')
        out = materialise_many([_wrap(image) for image in vols])
        return out[0] if len(out) == 1 else out


class random_crop:
    """A random window of `dim` voxels of an [x,y,z,c] volume, the same for
    every volume of a joint list (:337-396): re-seeds numpy's global RNG with
    the joint seed (:354) and keeps the reference's dim-shrinking rules
    (:358-366, :370-373).  Recorded as a window on the raw stack; a [x,y,c]
    image takes the reference's 2-D branch on the host."""

    def __init__(self, dim):
        self.dim = np.array(dim)

    @joint_transform
    def __call__(self, image, seed):
        if not isinstance(image, (np.ndarray, PendingVolume)):
            raise ValueError(f'Expected input to be list but got {type(image)}')
        dim = copy.copy(self.dim)
        np.random.seed(seed)
        shp = tuple(image.shape)
        if not np.all(shp[0:-1:1] >= np.array(dim)):
            if shp[-2] < dim[-1]:        # only a short Z shrinks the request ...
                dim[-1] = shp[-2]
            elif shp[0] >= dim[0]:       # ... else an axis that is large enough is taken whole
                dim[0] = shp[0]
            elif shp[1] >= dim[1]:
                dim[1] = shp[1]
            else:
                raise IndexError(f'Output dimensions: {dim} are larger than input image: {shp}')
        if image.ndim == 4:
            shape = shp[0:-1]
            for i, short in enumerate(shape < dim):
                if short:
                    dim[i] = shape[i]
            x = int(np.random.randint(0, shape[0] - dim[0] + 1, 1)[0])
            y = int(np.random.randint(0, shape[1] - dim[1] + 1, 1)[0])
            if dim[2] < shape[2]:
                z = int(np.random.randint(0, shape[2] - dim[2] + 1, 1)[0])
            else:
                z = 0
                dim[2] = shape[2]
            v = _wrap(image)
            for axis, (o, n) in enumerate(((x, dim[0]), (y, dim[1]), (z, dim[2]))):
                v.take(axis, start=o, n=min(int(n), shape[axis] - o))
            return v
        if image.ndim == 3:   # the reference's 2-D branch, as it is written (:387-391)
            a = _host(image)
            shape = a.shape
            x = np.random.randint(0, dim[0] - shape[0] + 1, 1)
            y = np.random.randint(0, dim[1] - shape[1] + 1, 1)
            return PendingVolume(a[x:x + dim[0] - 1:1, y:y + dim[1] - 1:1, :])
        raise IndexError(f'Image must have dimensions 3 or 4. Not {image.ndim}')


def _keep_lists(mask):
    """nul_crop's keep lists of a lazy integer [.,.,.,1] mask: rows of the
    current view's axis 0 whose sum is > 1, then rows of axis 1 of the
    row-filtered mask (:478-485).  On the to_float-scaled mask `sum > 1` is
    exactly `integer sum > 2**bits` (sums of multiples of 2**-16 are exact in
    float64), so the raw integers are summed."""
    cache = key = None
    if mask.source is not None and mask.uncropped():
        cache = mask.source.keep_lists
        key = (mask.to_float, mask.reshaped)
        if key in cache:
            return cache[key]
    m = mask.windowed_raw()
    if mask.reshaped:
        m = m.swapaxes(m.ndim - 2, 0)
    thr = (2 ** (8 * m.dtype.itemsize)) if mask.to_float else 1
    lr = m.sum(axis=(1, 2, 3), dtype=np.int64) > thr
    ud = m[lr].sum(axis=(0, 2, 3), dtype=np.int64) > thr
    lists = (np.flatnonzero(lr), np.flatnonzero(ud))
    if cache is not None:
        cache[key] = lists
    return lists


class nul_crop:
    """Drops the x rows, then the y rows, where the mask (image_list[1]) is
    empty, from every volume of the list (:460-489).  Recorded as keep lists on
    the raw stacks; the lists come from the raw integer mask on the host and are
    cached per stack while the volume is uncropped.  Float masks take the host
    path, and so does a list with a recorded rotation (the keep lists would
    need the rotated mask)."""

    def __init__(self, rate=1):
        self.rate = rate

    def __call__(self, image_list):
        if not isinstance(image_list, list):
            raise ValueError(f'Expected input to be list but got {type(image_list)}')
        if not np.random.random() < self.rate:
            return image_list
        mask = image_list[1]
        lazy = (all(isinstance(v, PendingVolume) and v.raw.ndim == 4 and v.rot is None for v in image_list)
                and mask._dtype_code() in _INT_CODES and mask.shape[-1] == 1 and not mask.steps
                and (not isinstance(mask.raw, torch.Tensor) or mask.raw.device.type == 'cpu'))
        if lazy:
            lr, ud = _keep_lists(mask)
            for v in image_list:
                n0, n1 = v.shape[0], v.shape[1]
                if n0 != mask.shape[0]:   # numpy's boolean index error (:480)
                    raise IndexError(f'boolean index did not match indexed array along axis 0; size of axis is '
                                     f'{n0} but size of corresponding boolean axis is {mask.shape[0]}')
                if n1 != mask.shape[1]:
                    raise IndexError(f'boolean index did not match indexed array along axis 1; size of axis is '
                                     f'{n1} but size of corresponding boolean axis is {mask.shape[1]}')
            out = []
            for v in image_list:
                v.take(0, keep=lr)
                v.take(1, keep=ud)
                out.append(v)
            return out
        arrays = [_host(v) for v in image_list]
        m = arrays[1]
        lr = m.sum(axis=1).sum(axis=1).flatten() > 1
        arrays = [a[lr, :, :, :] for a in arrays]
        m = arrays[1]
        ud = m.sum(axis=0).sum(axis=1).flatten() > 1
        return [PendingVolume(a[:, ud, :, :]) for a in arrays]


class random_rotate:
    """scipy.ndimage.rotate of the (x, y) plane by `angle` degrees, nearest
    neighbour, same extents, zeros outside (:230-254); the same angle for every
    volume of a joint list.  `if not self.angle` (None and 0 alike) re-seeds
    numpy's global RNG with the joint seed and draws randint(0, 360); a given
    angle draws nothing.  Recorded for the device on an integer [Z,Y,X,C] stack
    with to_float and reshape applied and no rotation yet: the kernel gathers
    with `rotate_nearest`'s arithmetic.  Anything else is rotated on the host."""

    def __init__(self, angle=None):
        self.angle = angle

    @joint_transform
    def __call__(self, image, seed):
        if not isinstance(image, (np.ndarray, PendingVolume)):
            raise TypeError(f'Expected list of images as input, but got {type(image)}')
        if not self.angle:
            np.random.seed(seed)
            theta = np.random.randint(0, 360, 1)[0]
        else:
            theta = self.angle
        c, s = cos_sin(theta)
        v = _wrap(image)
        if (v.raw.ndim == 4 and v._dtype_code() in _INT_CODES and v.to_float and v.reshaped and v.rot is None
                and v.raw.shape[-1] <= _lib.INGEST_MAX_C):
            nx, ny = v.shape[:2]
            v.rot = Rotation(c, s, nx, ny, len(v.steps))
            return v
        return PendingVolume(rotate_nearest(_host(v).astype(np.float64), c, s))


class random_affine:
    """The reference's constructor fails before anything else (:200-203): it
    raises the NotImplemented constant, which is not callable, so a TypeError."""

    def __init__(self):
        raise NotImplemented('hcat.transforms.random_affine is unusable in the reference and not provided')


class random_intensity:
    """Per channel v -= randint(range) / 100 where a uniform draw exceeds
    `chance`; then v < 0 -> 0, NaN -> 0, Inf -> 1 over the whole image (:301-334)."""

    def __init__(self, range=(-30, 30), chance=0):
        self.range = range
        self.chance = chance

    def __call__(self, image):
        if not isinstance(image, (np.ndarray, PendingVolume)):
            raise TypeError(f'Expected image to be of type np.ndarray, not {type(image)}')
        C = image.shape[-1]
        val = np.random.randint(self.range[0], self.range[1], C) / 100
        if image.ndim not in (3, 4):
            raise IndexError(f'Image should have 3 or 4 dimmensions, not {image.ndim} with shape {image.shape}')
        on = [bool(np.random.random() > self.chance) for _ in range(C)]
        st = Step(INTENSITY, [float(val[c]) if on[c] else 0.0 for c in range(C)], [float(o) for o in on])
        v = _wrap(image)
        if v.recordable():
            v.steps.append(st)
            return v
        return PendingVolume(_eager_step(_host(v), st))


class drop_channel:
    """With probability 1 - chance one random channel is set to 0 (:285-298)."""

    def __init__(self, chance):
        self.chance = chance

    def __call__(self, image):
        if not np.random.random() > self.chance:
            return image
        C = image.shape[-1]
        i = np.random.randint(0, C)
        v = _wrap(image)
        if v.recordable(need_float=False):
            v.steps.append(Step(DROP, [float(c == i) for c in range(C)]))
            return v
        a = _host(v)
        a[:, :, :, i] = 0
        return PendingVolume(a)


class clean_image:
    """NaN -> 0, +-Inf -> 1 (:616-631)."""

    @joint_transform
    def __call__(self, image, seed):
        v = _wrap(image)
        if v.recordable(need_float=False):
            v.steps.append(Step(CLEAN, [0.0] * v.shape[-1]))
            return v
        a = _host(v)
        dtype = a.dtype
        a[np.isnan(a)] = 0
        a[np.isinf(a)] = 1
        return PendingVolume(a.astype(dtype=dtype))


class remove_channel:
    """Keeps the channels `remaining_channel_index` of the last axis (:590-613)."""

    def __init__(self, remaining_channel_index=(0, 2, 3)):
        self.index_remain = remaining_channel_index

    def __call__(self, image):
        if image.shape[-1] == len(self.index_remain):
            return image
        if isinstance(image, PendingVolume):
            if image.ndim in (3, 4, 5):
                image.select_channels(self.index_remain)
            return image
        if image.ndim == 3:
            image = image[:, :, self.index_remain]
        elif image.ndim == 4:
            image = image[:, :, :, self.index_remain]
        elif image.ndim == 5:
            image = image[:, :, :, :, self.index_remain]
        return image


class random_gamma:
    """v ** factor, factor uniform in gamma_range (:186-197).  The reference
    calls skimage.exposure.adjust_gamma, which for a float image computes
    ((v / 1) ** gamma) * 1 * 1 and raises ValueError for negative values; this
    transform is pinned to numpy's float64 power, not to scikit-image.  The step
    joins the device program only while the values are known to be >= 0 (integer
    raw stack, no normalize yet); otherwise the host path checks and raises."""

    def __init__(self, gamma_range=(.8, 1.2)):
        self.gamma_range = gamma_range

    def __call__(self, image):
        v = _wrap(image)
        if not (v._dtype_code() == _lib.HCU_F64 or (v.to_float and v._dtype_code() in _INT_CODES)):
            raise TypeError(f'Expected image dataype to be float but got {v.raw_ndarray().dtype}')
        factor = np.random.uniform(self.gamma_range[0], self.gamma_range[1], 1)
        if factor < 0:
            factor = 0
        g = float(np.asarray(factor).reshape(-1)[0])
        if v.recordable() and v.non_negative():
            v.steps.append(Step(GAMMA, [g] * v.shape[-1]))
            return v
        a = _host(v)
        if np.any(a < 0):
            raise ValueError('Image Correction methods work correctly only on non-negative images. '
                             'Use skimage.exposure.rescale_intensity.')
        return PendingVolume(a ** factor)


class spekle:
    """v + float32(N(0, gamma)), clipped to [0, 1] (:159-183).  On the device
    path ONE np.random.randint is drawn as a key and the per-voxel normals come
    from a counter-based generator keyed by it (same distribution, deterministic
    given the numpy seed, a different stream than the reference's per-voxel
    np.random.normal); on the host path the noise is np.random.normal's, as in
    the reference."""

    def __init__(self, gamma=.1):
        self.gamma = gamma

    def __call__(self, image):
        v = _wrap(image)
        if not (v._dtype_code() == _lib.HCU_F64 or (v.to_float and v._dtype_code() in _INT_CODES)):
            raise TypeError(f'Expected image datatype to be float but got {v.raw_ndarray().dtype}')
        if self.gamma > 1:
            raise ValueError(f'Maximum spekle gamma should be less than 1 [ gamma =/= {self.gamma} ]')
        if v.recordable():
            key = int(np.random.randint(0, 2 ** 31 - 1))
            v.steps.append(Step(SPEKLE, [float(self.gamma)] * v.shape[-1], key=key))
            return v
        a = _host(v)
        noise = np.float32(np.random.normal(0, self.gamma, np.shape(a)))
        a = a + noise
        a[a < 0] = 0
        a[a > 1] = 1
        return PendingVolume(a)


def _to_device_raw(raw, device):
    if isinstance(raw, torch.Tensor):
        t = raw
    else:
        a = np.ascontiguousarray(raw)
        if a.dtype == np.uint16:
            t = torch.from_numpy(a.view(np.int16))   # raw bits; the kernel reads uint16
        else:
            t = torch.from_numpy(a)
    if t.device.type != 'cuda':
        t = t.contiguous().pin_memory().to(device, non_blocking=True)
    return t.contiguous()


def _device_raw(v, device):
    """The raw stack in HBM: the dataloader's resident copy, or a copy of this item."""
    if v.source is not None:
        t = v.source.resident(device)
        if t is not None:   # (the dataloader adds the mask's channel axis as a view)
            return t.unsqueeze(t.dim()) if t.dim() < v.raw.ndim else t
    return _to_device_raw(v.raw, device)


def _ingest_volume(v, device):
    """One volume through hcu_ingest_volume (float64 and [Y,X,C] stacks, and
    volumes without reshape): fp16 [1,C,X,Y,Z] (reshape applied) or [1,C,Z,Y,X]."""
    code = v._dtype_code()
    if code is None:
        raise TypeError('Expected image datatype of uint8 or uint16 ')
    if (not v.uncropped() or v.chan is not None or v.rot is not None or len(v.steps) > 1
            or any(st.kind != NORMALIZE for st in v.steps)):
        v = PendingVolume(v.to_ndarray())   # the recorded steps on the host; the device pass only rounds
        code = v._dtype_code()
        if code is None:
            raise TypeError('Expected image datatype of uint8 or uint16 ')
    raw = _device_raw(v, device)
    shp = tuple(raw.shape)
    two_d = len(shp) == 3
    if two_d:          # [Y,X,C] image: a Z = 1 volume
        shp = (1,) + shp
    if len(shp) != 4:
        raise ValueError(f'Expected a [Z,Y,X,C] or [Y,X,C] stack, got shape {tuple(raw.shape)}')
    Z, Y, X, C = shp
    if v.reshaped:
        out = _lib.empty((1, C, X, Y, Z), torch.float16, device)
    else:
        out = _lib.empty((1, C, Z, Y, X), torch.float16, device)
    mean = std = None
    if v.mean is not None:
        mean = (ctypes.c_double * C)(*v.mean)
        std = (ctypes.c_double * C)(*v.std)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().hcu_ingest_volume(
            _lib.ptr(raw), code, 1, Z, Y, X, C, int(v.to_float), int(v.reshaped), mean, std,
            _lib.ptr(out), _lib.stream_handle(device)), 'to_tensor')
    if two_d:          # [1,C,X,Y,1] -> [1,C,X,Y] / [1,C,1,Y,X] -> [1,C,Y,X]
        out = out[..., 0] if v.reshaped else out[:, :, 0]
    return out


def _is_job(v):
    """Volumes hcu_ingest_jobs takes: integer [Z,Y,X,C] stacks with reshape
    applied, a plain z window and at most 16 channels (a recorded rotation
    implies all of these)."""
    return (v.raw.ndim == 4 and v._dtype_code() in _INT_CODES and v.reshaped
            and not isinstance(v.sel[0], np.ndarray) and v.raw.shape[-1] <= _lib.INGEST_MAX_C)


def _fill_job(job, v, raw, dst, maps, host_base, dev_base):
    Z, Y, X, C = (int(s) for s in raw.shape)
    code = v._dtype_code()
    job.src, job.dst = raw.data_ptr(), dst.data_ptr()
    job.src_dtype, job.Z, job.Y, job.X, job.C = code, Z, Y, X, C
    oz, oy, ox, nc = v._raw_shape()
    R = v.rot
    if R is not None:   # the window / maps below describe the pre-rotation view of ox by oy voxels
        m, off = rotation_terms(R.c, R.s, ox, oy)
        job.rot, job.fill_after = 1, R.after
        job.rot_m[:] = [float(x) for x in m.reshape(-1)]
        job.rot_off[:] = [float(x) for x in off]
        job.rot_nx, job.rot_ny, job.rot_px, job.rot_py = ox, oy, R.px, R.py
        ox, oy = R.ox, R.oy
    job.ox, job.oy, job.oz = ox, oy, oz
    job.z0 = 0 if v.sel[0] is None else v.sel[0][0]
    for name, w in (('y', v.sel[1]), ('x', v.sel[2])):
        if isinstance(w, np.ndarray):
            off = maps[w.tobytes()][0]
            setattr(job, name + 'map_dev', dev_base + off)
            setattr(job, name + 'map_host', host_base + off)
        else:
            setattr(job, name + '0', 0 if w is None else w[0])
    chan = list(range(C)) if v.chan is None else v.chan
    job.n_chan = nc
    for c in range(nc):
        job.chan[c] = chan[c]
    job.scale = (2.0 ** -16 if code == _lib.HCU_U16 else 2.0 ** -8) if v.to_float else 1.0
    job.n_steps = len(v.steps)
    for s, st in enumerate(v.steps):
        js = job.steps[s]
        js.kind, js.key = st.kind, st.key
        for c in range(nc):
            js.a[c] = st.a[c]
            if st.b is not None:
                js.b[c] = st.b[c]


def materialise_many(vols, dsts=None, device=None):
    """Run the recorded chains of `vols` on the device: fp16 [1,C,X,Y,Z] each
    (into dsts[i], a contiguous [C,X,Y,Z]-sized tensor, when given).  Every
    integer [Z,Y,X,C] stack with reshape applied is a job of ONE
    hcu_ingest_jobs launch, whose job table and keep lists (each distinct list
    once) travel in one pinned buffer and one copy; float64 and 2-D stacks go
    through hcu_ingest_volume one by one."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    outs = [None] * len(vols)
    jobs = [i for i, v in enumerate(vols) if _is_job(v)]
    for i, v in enumerate(vols):
        if i not in jobs:
            out = _ingest_volume(v, device)
            if dsts is not None:
                dsts[i].view(out.shape).copy_(out)
                out = dsts[i]
            outs[i] = out
    if jobs:
        table_bytes = ctypes.sizeof(_lib.IngestJob) * len(jobs)
        nbytes = table_bytes
        maps = {}   # keep list bytes -> (offset in the buffer, array)
        for i in jobs:
            for w in vols[i].sel[1:]:
                if isinstance(w, np.ndarray) and maps.setdefault(w.tobytes(), (nbytes, w))[0] == nbytes:
                    nbytes += (w.nbytes + 15) // 16 * 16
        host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        host[:table_bytes].zero_()
        for off, w in maps.values():
            ctypes.memmove(host.data_ptr() + off, w.ctypes.data, w.nbytes)
        table = (_lib.IngestJob * len(jobs)).from_address(host.data_ptr())
        with torch.cuda.device(device):
            dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
            raws = []
            for k, i in enumerate(jobs):
                v = vols[i]
                raws.append(_device_raw(v, device))
                ox, oy, oz, nc = v.shape
                out = _lib.empty((1, nc, ox, oy, oz), torch.float16, device) if dsts is None else dsts[i]
                _fill_job(table[k], v, raws[-1], out, maps, host.data_ptr(), dev.data_ptr())
                outs[i] = out
            dev.copy_(host, non_blocking=True)
            _lib.check(_lib.lib().hcu_ingest_jobs(host.data_ptr(), dev.data_ptr(), len(jobs),
                                                  _lib.stream_handle(device)), 'to_tensor')
    return outs


def materialise(v, device=None):
    """Run the recorded chain on the device: fp16 [1,C,X,Y,Z] (reshape applied)
    or [1,C,Z,Y,X] (not applied), as the reference's to_tensor returns."""
    return materialise_many([v], device=device)[0]


def ingest(raw, mean=None, std=None, device=None):
    """Batched input path: raw [B,Z,Y,X,C] (or one [Z,Y,X,C] stack) uint16 /
    uint8 -> fp16 [B,C,X,Y,Z] = to_float -> reshape -> normalize(mean, std)
    -> to_tensor of each volume, in one launch."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    t = _to_device_raw(raw, device)
    if t.dim() == 4:
        t = t.unsqueeze(0)
    if t.dim() != 5:
        raise ValueError(f'Expected [B,Z,Y,X,C] or [Z,Y,X,C], got {tuple(t.shape)}')
    code = _TORCH_RAW.get(t.dtype)
    if code is None:
        raise TypeError('Expected image datatype of uint8 or uint16 ')
    B, Z, Y, X, C = t.shape
    out = _lib.empty((B, C, X, Y, Z), torch.float16, device)
    m = s = None
    if mean is not None:
        m = (ctypes.c_double * C)(*[float(x) for x in mean[:C]])
        s = (ctypes.c_double * C)(*[float(x) for x in std[:C]])
    with torch.cuda.device(device):
        _lib.check(_lib.lib().hcu_ingest_volume(_lib.ptr(t), code, B, Z, Y, X, C, 1, 1, m, s, _lib.ptr(out),
                                                _lib.stream_handle(device)), 'ingest')
    return out
