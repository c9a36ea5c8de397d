"""Drop-in hcat.haircell.HairCell (reference hcat/haircell.py:5-85): one
segmented cell, its bounding box, centre, volume and the mean, standard
deviation and median of the four stain channels inside it.

Two ways in.  The reference's constructor, HairCell(image_coords, center,
image, mask, id), computes everything on the host with numpy as the reference
does: for code that builds a cell by hand from an image slice and its mask.
HairCell.from_table(...) fills the same attributes from one row of the device
tables of hcunet_amd.cells.cell_table, which is what generate_cell_objects
uses: no per-cell pass over the volume on the host.

Kept from the reference: `volume` starts as the int 0 and adds 1000e-9 * n_z *
(289e-9)**2 per z plane of the mask in order (float64); a mask with at most one
voxel makes the cell `is_bad`, every statistic {'mean': nan, 'std': nan,
'median': nan} without 'num_samples', and sets `unique_mask` to torch.zeros(10);
the values are mapped to g * 0.5 + 0.5 when the minimum of the whole image
slice handed in (all channels, voxels outside the mask included) is below 0.
"""
import numpy as np
import torch

CHANNELS = ['dapi', 'gfp', 'myo7a', 'actin']
GFP = 1
_NAN_STATS = ('mean', 'std', 'median')


def plane_volume(n):
    """The volume one z plane of n voxels adds (haircell.py:20)."""
    return 1000e-9 * n * ((289e-9) ** 2)


class HairCell:
    def __init__(self, image_coords, center, image, mask, id, type=None):
        self._start(image_coords, center, id, type)
        for z in range(mask.shape[-1]):
            self.volume += plane_volume((mask[:, :, z] > 0).sum())
        if isinstance(image, torch.Tensor):
            image = image.numpy()
        good = mask.sum() > 1
        if not good:
            self._bad()
        for i, channel in enumerate(CHANNELS):
            self.signal_stats[channel] = self._calculate_gfp_statistics(image, mask, i) if good else self._nan()
        self.gfp_stats = self._calculate_gfp_statistics(image, mask) if good else self._nan()

    def _start(self, image_coords, center, id, type):
        self.image_coords = image_coords   # [x0, y0, z0, x1, y1, z1]
        self.center = center               # [x, y, z]
        self.type = type
        self.distance_from_apex = []
        self.unique_id = id
        self.is_bad = False
        self.signal_stats = {}
        self.volume = 0

    def _bad(self):
        self.unique_mask = torch.zeros(10)
        self.is_bad = True

    @staticmethod
    def _nan():
        return {k: np.nan for k in _NAN_STATS}

    @classmethod
    def from_table(cls, image_coords, center, id, count, plane_count, mean, std, median, type=None):
        """A cell from one row of cell_table's tables (host arrays): count,
        plane_count [Z], mean [C] and std [C] float64, median [C,2] float32, C
        >= 4.  mean and std become np.float32 of the float64 values, the median
        the float32 mean of the two middle order statistics as np.median forms
        it, the volume is summed here from plane_count over z0:z1."""
        self = cls.__new__(cls)
        self._start(image_coords, center, id, type)
        for z in range(int(image_coords[2]), int(image_coords[5])):
            self.volume += plane_volume(np.int64(plane_count[z]))
        n = int(count)
        if n <= 1:
            self._bad()

        def stats(c):
            if n <= 1:
                return cls._nan()
            lo, hi = np.float32(median[c][0]), np.float32(median[c][1])
            return {'mean': np.float32(mean[c]), 'std': np.float32(std[c]),
                    'median': np.float32(lo + hi) / np.float32(2), 'num_samples': (n,)}

        for i, channel in enumerate(CHANNELS):
            self.signal_stats[channel] = stats(i)
        self.gfp_stats = stats(GFP)
        return self

    def set_frequency(self, cochlea_curve, percentage):
        """The place along the cochlea nearest to the cell's centre:
        cochlea_curve [2,n] (x row, y row), percentage [n]."""
        # (the centre's second coordinate against the x row, its first against the y row: kept)
        d0 = self.center[1] - cochlea_curve[0, :]
        d1 = self.center[0] - cochlea_curve[1, :]
        i = np.argmin(np.sqrt(d0 ** 2 + d1 ** 2))
        self._place_percentage = percentage[i]
        self._closest_place = cochlea_curve[:, i]
        self.frequency = [self._closest_place, self._place_percentage]

    @staticmethod
    def _calculate_gfp_statistics(image, mask, channel=GFP):
        """{'mean', 'std', 'median', 'num_samples'} of image[0, channel] inside
        mask > 0 (image: numpy [1,C,x,y,z]; mask: [x,y,z])."""
        if isinstance(image, torch.Tensor):
            image = image.numpy()
        if isinstance(mask, torch.Tensor):
            mask = mask.numpy()
        inside = np.asarray(mask) > 0
        g = image[0, channel][inside]
        if image.min() < 0:   # of the whole slice, not of g
            g = g * 0.5 + 0.5
        return {'mean': g.mean(), 'std': g.std(), 'median': np.median(g), 'num_samples': g.shape}
