"""descriptools.morphology -- descriptools_amd.morphology (geodesic reconstruction: seeded fill, h-minima / h-maxima,
regional extrema, opening and closing by reconstruction; net-new, the reference has no such module) under the
reference's package name, beside the modules a caller of the reference imports."""
from descriptools_amd.morphology import *  # noqa: F401,F403
from descriptools_amd import morphology as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
