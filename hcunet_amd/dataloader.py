"""Drop-in hcat.dataloader.Stack (hcat/dataloader.py:17-92) feeding the device
input path.

Same constructor, file discovery (`{path}/*.mask.tif` + `.tif` + `.pwl.tif`),
errors and __getitem__ order of transforms as the reference.  What changes:
* the raw stacks are kept as read (uint16 / uint8) in page-locked host memory,
  so a host->device copy is one asynchronous DMA of the raw bytes;
* the default out_transforms is hcunet_amd.transforms.to_tensor, which runs
  the to_float -> reshape -> normalize -> to_tensor chain as one device pass
  and returns fp16 tensors already on the GPU;
* `prefetch(order)` yields items while the next one is copied and converted
  on a side stream (the reference converts on the host and copies float
  tensors, segment.py:89 / the training loop's .cuda());
* `resident_bytes=` keeps the raw stacks in HBM after their first use, so a
  random crop reads its window from device memory instead of copying the
  whole stack per item;
* `batches(batch_size)` yields fp16 (image, mask, pwl) batches [B,C,X,Y,Z]:
  the transform lists run per item (recording crops and augmentations, with
  the reference's RNG draws in item order) and all volumes of a batch are
  converted by one hcu_ingest_jobs launch on a side stream.
Files are read with skimage.io.imread (as the reference) or tifffile when
importable; `reader=` takes any callable path -> ndarray.

RecursiveStack (hcat/dataloader.py:190-278) is the same loader with two more
volumes per item, the centre-of-mass stack and the unpickled vector field.
"""
import glob
import os
import pickle

import numpy as np
import torch

from . import _lib
from . import transforms as t


def _default_reader():
    try:
        from skimage import io   # the reference's reader (hcat/dataloader.py:3)
        return io.imread
    except ImportError:
        pass
    try:
        import tifffile
        return tifffile.imread
    except ImportError:
        pass
    return None


def _pinned(a):
    """The raw bits as a page-locked tensor (uint16 held as int16: same bytes);
    without a ROCm device (construction on a CPU host) the tensor stays pageable."""
    a = np.ascontiguousarray(a)
    t_ = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    if torch.cuda.is_available():
        t_ = t_.pin_memory()
    return t_, a.dtype, a.ndim


class _Raw:
    """A pinned raw stack that behaves like the ndarray the reference holds
    for expand_dims / ndim / dtype purposes and hands the pinned tensor to the
    device path."""

    def __init__(self, a, stack=None):
        self.tensor, self.np_dtype, _ = _pinned(a)
        self.stack = stack
        self.keep_lists = {}    # nul_crop's keep lists of the uncropped mask (it never changes)
        self.device_copy = {}   # device -> (resident raw tensor, event of its upload)

    def pending(self, expand=False):
        r = self.tensor.unsqueeze(self.tensor.dim()) if expand else self.tensor
        return t.PendingVolume(r, np_dtype=self.np_dtype, source=self)

    def resident(self, device):
        """The raw stack in HBM, uploaded on first use and kept while the
        Stack's resident_bytes budget lasts; None: copy this item as it comes."""
        hit = self.device_copy.get(device)
        if hit is None:
            nbytes = self.tensor.numel() * self.tensor.element_size()
            if self.stack is None or not self.stack._reserve(nbytes):
                return None
            d = self.tensor.to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
            hit = self.device_copy[device] = (d, ev)
        d, ev = hit
        torch.cuda.current_stream(device).wait_event(ev)   # (an upload on another stream)
        return d


_LAZY = (t.to_float, t.reshape, t.normalize, t.to_tensor, t.random_crop, t.nul_crop, t.random_intensity,
         t.drop_channel, t.clean_image, t.remove_channel, t.random_gamma, t.spekle, t.random_rotate)


def _arrays_for(transform, items):
    """The lazy device chain understands PendingVolume; any other transform
    (the reference's random augmentations, a caller's own) gets the ndarray
    the reference's eager chain would hold at that point."""
    if isinstance(transform, _LAZY):
        return items
    return [x.to_ndarray() if isinstance(x, t.PendingVolume) else x for x in items]


class Stack(torch.utils.data.Dataset):
    """Dataloader for hcat.unet: 3D stacks with mask and pixel-weight maps."""

    def __init__(self, path, image_transforms, joint_transforms, out_transforms=None, reader=None,
                 resident_bytes=None):
        # raw bytes kept in HBM after their first use: None all stacks, 0 none
        # (every item copies its stacks); stacks beyond the budget are copied per item
        self.resident_left = float('inf') if resident_bytes is None else int(resident_bytes)
        if out_transforms is None:
            out_transforms = [t.to_tensor()]
        self.image_transforms = image_transforms
        self.out_transforms = out_transforms
        self.joint_transforms = joint_transforms
        self.files = glob.glob(f'{path}{os.sep}*.mask.tif')
        if len(self.files) == 0:
            raise FileExistsError('No Valid Mask Files Found')
        reader = reader or _default_reader()
        if reader is None:
            raise ImportError('hcat.dataloader.Stack reads .tif stacks with skimage.io or tifffile; '
                              'neither is installed (pass reader=callable)')
        self.image, self.mask, self.pwl = [], [], []
        for mask_path in self.files:
            file_with_mask = os.path.splitext(mask_path)[0]
            image_data_path = os.path.splitext(file_with_mask)[0] + '.tif'
            pwl_data_path = os.path.splitext(file_with_mask)[0] + '.pwl.tif'
            self.image.append(_Raw(reader(image_data_path), self))
            m = reader(mask_path)
            try:   # some masks are [Z,Y,X,C], others [Z,Y,X] (:57-61)
                m = m[:, :, :, 0]
            except IndexError:
                pass
            self.mask.append(_Raw(m, self))
            self.pwl.append(_Raw(reader(pwl_data_path), self))

    def __len__(self):
        return len(self.files)

    def _reserve(self, nbytes):
        if nbytes > self.resident_left:
            return False
        self.resident_left -= nbytes
        return True

    def _recorded(self, item):
        """The joint and image transforms of one item (:79-86)."""
        # channel axis last (:80-81), on the pinned raw tensors (no copy)
        image = self.image[item].pending()
        mask = self.mask[item].pending(expand=True)
        pwl = self.pwl[item].pending(expand=True)
        for jt in self.joint_transforms:
            image, mask, pwl = _arrays_for(jt, [image, mask, pwl])
            image, mask, pwl = jt([image, mask, pwl])
        for it in self.image_transforms:
            image = _arrays_for(it, [image])[0]
            image = it(image)
        return image, mask, pwl

    def __getitem__(self, item):
        image, mask, pwl = self._recorded(item)
        for ot in self.out_transforms:
            image, mask, pwl = _arrays_for(ot, [image, mask, pwl])
            image, mask, pwl = ot([image, mask, pwl])
        return image, mask, pwl

    def prefetch(self, order=None, device=None):
        """Yield self[i] for i in `order`, converting item k+1 on a side stream
        while item k is consumed on the current stream."""
        order = list(range(len(self))) if order is None else list(order)
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        side = torch.cuda.Stream(device)
        main = torch.cuda.current_stream(device)

        def launch(i):
            with torch.cuda.stream(side):
                items = self[i]
            ev = torch.cuda.Event()
            ev.record(side)
            return items, ev

        nxt = launch(order[0]) if order else None
        for k in range(len(order)):
            items, ev = nxt
            if k + 1 < len(order):
                nxt = launch(order[k + 1])
            main.wait_event(ev)
            for x in items:
                if isinstance(x, torch.Tensor):
                    x.record_stream(main)
            yield items

    def _batch(self, items, device):
        """fp16 (image [B,C,X,Y,Z], mask, pwl) of the items, one launch."""
        vols = []
        for i in items:   # RNG draws in item order, to_tensor's joint seed included: the stream of self[i]
            vols.append([t._wrap(x) for x in self._recorded(i)])
            np.random.randint(0, 1e8, 1)
        n = len(vols[0])   # 3 volumes per item; RecursiveStack: 5
        outs = []
        for k in range(n):
            shapes = [v[k].shape for v in vols]
            if any(len(s) != 4 for s in shapes):
                raise ValueError(f'Stack.batches expects [x,y,z,c] volumes, got {shapes} for items {items}')
            if len(set(shapes)) != 1:
                raise ValueError('Stack.batches: the items of one batch end with different extents: '
                                 + ', '.join(f'item {i}: {s}' for i, s in zip(items, shapes)))
            X, Y, Z, C = shapes[0]
            outs.append(_lib.empty((len(items), C, X, Y, Z), torch.float16, device))
        flat = [v[k] for v in vols for k in range(n)]
        t.materialise_many(flat, [outs[k][b] for b in range(len(items)) for k in range(n)], device)
        return tuple(outs)

    def batches(self, batch_size, order=None, device=None):
        """Yield fp16 (image [B,C,X,Y,Z], mask [B,1,X,Y,Z], pwl [B,1,X,Y,Z]) on
        the device for consecutive groups of `batch_size` items of `order`
        (a short last batch as it is).  The joint and image transform lists run
        per item; every volume of a batch is a job of one launch (the device
        pass replaces out_transforms); batch k+1 is prepared on a side stream
        while batch k is consumed, as in `prefetch`.  ValueError when the items
        of a batch end with different extents."""
        order = list(range(len(self))) if order is None else list(order)
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        groups = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
        side = torch.cuda.Stream(device)
        main = torch.cuda.current_stream(device)

        def launch(items):
            with torch.cuda.stream(side):
                out = self._batch(items, device)
            ev = torch.cuda.Event()
            ev.record(side)
            return out, ev

        nxt = launch(groups[0]) if groups else None
        for k in range(len(groups)):
            out, ev = nxt
            if k + 1 < len(groups):
                nxt = launch(groups[k + 1])
            main.wait_event(ev)
            for x in out:
                x.record_stream(main)
            yield out


class RecursiveStack(Stack):
    """Drop-in hcat.dataloader.RecursiveStack (hcat/dataloader.py:190-278), the
    dataloader of hcat.r_unet: per `*.mask.tif` also `.labels.com.tif` (kept
    with a channel axis, :243) and the unpickled `.labels.vector.pkl`; items
    are (image, mask, pwl, com, vec).  Same constructor, file discovery and
    __getitem__ order (joint, image, out transforms) as the reference, and a
    stack whose files are incomplete is reported and skipped the same way: the
    message is printed and the lists go on (:245-246).  `reader=`,
    `resident_bytes=`, `prefetch` and `batches` as Stack; the five volumes go
    through the lazy device chain, the float64 `vec` by hcu_ingest_volume."""

    def __init__(self, path, image_transforms, joint_transforms, out_transforms=None, reader=None,
                 resident_bytes=None):
        self.resident_left = float('inf') if resident_bytes is None else int(resident_bytes)
        if out_transforms is None:
            out_transforms = [t.to_tensor()]
        self.image_transforms = image_transforms
        self.out_transforms = out_transforms
        self.joint_transforms = joint_transforms
        self.files = glob.glob(f'{path}{os.sep}*.mask.tif')
        if len(self.files) == 0:
            raise FileExistsError('No Valid Mask Files Found')
        reader = reader or _default_reader()
        if reader is None:
            raise ImportError('hcat.dataloader.RecursiveStack reads .tif stacks with skimage.io or tifffile; '
                              'neither is installed (pass reader=callable)')
        self.image, self.mask, self.pwl, self.com, self.vec = [], [], [], [], []
        for mask_path in self.files:
            try:
                base = os.path.splitext(os.path.splitext(mask_path)[0])[0]
                self.image.append(_Raw(reader(base + '.tif'), self))
                m = reader(mask_path)
                try:   # some masks are [Z,Y,X,C], others [Z,Y,X] (:237-240)
                    m = m[:, :, :, 0]
                except IndexError:
                    pass
                self.mask.append(_Raw(m, self))
                self.pwl.append(_Raw(reader(base + '.pwl.tif'), self))
                self.com.append(_Raw(reader(base + '.labels.com.tif')[:, :, :, np.newaxis], self))
                with open(base + '.labels.vector.pkl', 'rb') as f:
                    self.vec.append(_Raw(pickle.load(f), self))
            except FileNotFoundError:
                print(f'ISSUE WITH: {os.path.splitext(mask_path)[0]}')

    def _recorded(self, item):
        """The joint and image transforms of one item (:257-274)."""
        vols = [self.image[item].pending(), self.mask[item].pending(expand=True),
                self.pwl[item].pending(expand=True), self.com[item].pending(), self.vec[item].pending()]
        for jt in self.joint_transforms:
            vols = list(jt(_arrays_for(jt, vols)))
        for it in self.image_transforms:
            vols[0] = it(_arrays_for(it, [vols[0]])[0])
        return tuple(vols)

    def __getitem__(self, item):
        image, mask, pwl, com, vec = self._recorded(item)
        for ot in self.out_transforms:
            image, mask, pwl, com, vec = _arrays_for(ot, [image, mask, pwl, com, vec])
            image, mask, pwl, com, vec = ot([image, mask, pwl, com, vec])
        return image, mask, pwl, com, vec
