"""descriptools.vector -- descriptools_amd.vector (vector rasterisation: polygons, lines and points onto the grid, and
polygonisation: label rasters back to polygon rings; net-new, the reference has no such module) under the reference's
package name, beside the modules a caller of the reference imports."""
from descriptools_amd.vector import *  # noqa: F401,F403
from descriptools_amd import vector as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
