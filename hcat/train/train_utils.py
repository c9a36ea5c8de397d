"""hcat.train.train_utils: makePWL, CalculateCenterOfMass, VectorToCenter and colormask_to_mask on the
device (hcunet_amd/train_utils.py; reference hcat/train/train_utils.py:9-93, :175-274).  makeMask stays the
reference's own (a sequential scan)."""
from hcunet_amd.train_utils import (CalculateCenterOfMass, VectorToCenter, colormask_to_mask,  # noqa: F401
                                    makePWL, pwl_offsets, pwl_values)
