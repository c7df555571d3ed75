"""descriptools.resample -- descriptools_amd.resample (raster resampling: warp, align, resize and aggregate; net-new,
the reference has no such module) under the reference's package name, beside the modules a caller of the reference
imports."""
from descriptools_amd.resample import *  # noqa: F401,F403
from descriptools_amd import resample as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
