"""descriptools.mfd -- descriptools_amd.mfd (multiple-flow-direction shares and contributing area; net-new, the
reference has no such module) under the reference's package name, beside the modules a caller of the reference
imports."""
from descriptools_amd.mfd import *  # noqa: F401,F403
from descriptools_amd import mfd as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
