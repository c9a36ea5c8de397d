"""hcat.haircell: re-export of the cell record (hcunet_amd/haircell.py;
reference hcat/haircell.py:5-85)."""
from hcunet_amd.haircell import HairCell  # noqa: F401
