"""descriptools.harmonic -- descriptools_amd.harmonic (harmonic interpolation: void filling, channel network base level
and the vertical distance to channel network; net-new, the reference has no such module) under the reference's package
name, beside the modules a caller of the reference imports."""
from descriptools_amd.harmonic import *  # noqa: F401,F403
from descriptools_amd import harmonic as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
