"""descriptools.cost -- descriptools_amd.cost (cost distance, cost allocation and back-links over a friction raster;
net-new, the reference has no such module) under the reference's package name, beside the modules a caller of the
reference imports."""
from descriptools_amd.cost import *  # noqa: F401,F403
from descriptools_amd import cost as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
