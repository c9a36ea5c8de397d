"""hcat.transforms: the input-path transforms, crops, rotation and intensity augmentations on the MI355X path
(hcat/transforms.py:15-396,460-489,590-631)."""
from hcunet_amd.transforms import (PendingVolume, clean_image, drop_channel, joint_transform,  # noqa: F401
                                   normalize, nul_crop, random_affine, random_crop, random_gamma,
                                   random_intensity, random_rotate, remove_channel, reshape, spekle, to_float, to_tensor)
