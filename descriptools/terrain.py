"""descriptools.terrain -- descriptools_amd.terrain (gradient, aspect, curvatures and hillshade of a windowed quadratic
fit; net-new, the reference has no such module) under the reference's package name, beside the modules a caller of the
reference imports."""
from descriptools_amd.terrain import *  # noqa: F401,F403
from descriptools_amd import terrain as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
