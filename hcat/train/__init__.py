"""hcat.train: the training-target generators on the MI355X path (hcat/train/train_utils.py)."""
from hcat.train import train_utils  # noqa: F401
from hcat.train.train_utils import (CalculateCenterOfMass, VectorToCenter, colormask_to_mask,  # noqa: F401
                                    makePWL)
