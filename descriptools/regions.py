"""descriptools.regions -- descriptools_amd.regions (connected regions of a mask: labels, sizes, seeded and sieved
selection; net-new, the reference has no such module) under the reference's package name, beside the modules a caller of
the reference imports."""
from descriptools_amd.regions import *  # noqa: F401,F403
from descriptools_amd import regions as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
