"""hcat.dataloader: Stack and RecursiveStack on the MI355X input path (hcat/dataloader.py:17-92, :190-278)."""
from hcunet_amd.dataloader import RecursiveStack, Stack  # noqa: F401
