"""descriptools.horizon -- descriptools_amd.horizon (geomorphon landforms, topographic openness and the sky-view factor
along eight lines of sight; net-new, the reference has no such module) under the reference's package name, beside the
modules a caller of the reference imports."""
from descriptools_amd.horizon import *  # noqa: F401,F403
from descriptools_amd import horizon as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
