"""descriptools.wetness -- descriptools_amd.wetness (the SAGA wetness index: suction, modified catchment area and the
index on it; net-new, the reference has no such module) under the reference's package name, beside the modules a caller
of the reference imports."""
from descriptools_amd.wetness import *  # noqa: F401,F403
from descriptools_amd import wetness as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
