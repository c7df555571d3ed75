"""descriptools.inundation -- descriptools_amd.inundation (local-inertial 2-D flood inundation: rain, inflow hydrographs
and HAND stage maps routed over the DEM; net-new, the reference has no such module) under the reference's package name,
beside the modules a caller of the reference imports."""
from descriptools_amd.inundation import *  # noqa: F401,F403
from descriptools_amd import inundation as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
