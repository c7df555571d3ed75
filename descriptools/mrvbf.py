"""descriptools.mrvbf -- descriptools_amd.mrvbf (multi-resolution valley bottom and ridge top flatness MRVBF / MRRTF,
the elevation percentile and one generalisation step; net-new, the reference has no such module) under the reference's
package name, beside the modules a caller of the reference imports."""
from descriptools_amd.mrvbf import *  # noqa: F401,F403
from descriptools_amd import mrvbf as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
