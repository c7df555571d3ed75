"""descriptools.routing -- descriptools_amd.routing (decayed, retention-limited and transport-limited accumulation;
net-new, the reference has no such module) under the reference's package name, beside the modules a caller of the
reference imports."""
from descriptools_amd.routing import *  # noqa: F401,F403
from descriptools_amd import routing as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
