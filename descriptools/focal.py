"""descriptools.focal -- descriptools_amd.focal (focal mean and standard deviation at any radius, TPI, DEV and the
multi-scale DEVmax; net-new, the reference has no such module) under the reference's package name, beside the modules a
caller of the reference imports."""
from descriptools_amd.focal import *  # noqa: F401,F403
from descriptools_amd import focal as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
