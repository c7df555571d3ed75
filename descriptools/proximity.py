"""descriptools.proximity -- descriptools_amd.proximity (Euclidean nearest-river distance, allocation and HAND; net-new,
the reference has no such module) under the reference's package name, beside the modules a caller of the reference
imports."""
from descriptools_amd.proximity import *  # noqa: F401,F403
from descriptools_amd import proximity as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
