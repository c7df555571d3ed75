"""descriptools.flowpath -- descriptools_amd.flowpath (the extreme of a value raster over everything upslope of a cell or
along its path downstream; net-new, the reference has no such module) under the reference's package name, beside the
modules a caller of the reference imports."""
from descriptools_amd.flowpath import *  # noqa: F401,F403
from descriptools_amd import flowpath as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
