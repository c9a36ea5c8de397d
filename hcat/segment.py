"""hcat.segment: re-export of the MI355X-native tiled inference driver
(hcunet_amd/segment.py; reference hcat/segment.py:21-136), of RDCNet's
post-processing, vector field to instance labels (hcunet_amd/instances.py;
reference :563-658): pixel_vec_to_cell and hist3d, and of the cell objects
built from those labels (hcunet_amd/cells.py; reference :508-560):
generate_cell_objects, with HairCell as the reference module imports it.
stitch_vec_to_cell and predict_instance_mask (no counterpart in the
reference) label a whole stack window by window with stack-wide ids.  The
watershed / RCNN post-processing of the reference module stays out of scope
(DESIGN.md): skimage's watershed is a sequential priority flood."""
from hcat.haircell import HairCell  # noqa: F401
from hcunet_amd.cells import generate_cell_objects  # noqa: F401
from hcunet_amd.instances import hist3d, pixel_vec_to_cell, stitch_vec_to_cell  # noqa: F401
from hcunet_amd.segment import predict_instance_mask, predict_segmentation_mask  # noqa: F401
