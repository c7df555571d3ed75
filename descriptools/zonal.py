"""descriptools.zonal -- descriptools_amd.zonal (zonal statistics, label compaction, per-zone histograms,
cross-tabulation and painting a table onto its zones; net-new, the reference has no such module) under the reference's
package name, beside the modules a caller of the reference imports."""
from descriptools_amd.zonal import *  # noqa: F401,F403
from descriptools_amd import zonal as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
