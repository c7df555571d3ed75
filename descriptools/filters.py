"""descriptools.filters -- descriptools_amd.filters (window minimum, maximum and range with opening and closing, the
window percentile and feature-preserving denoising; net-new, the reference has no such module) under the reference's
package name, beside the modules a caller of the reference imports."""
from descriptools_amd.filters import *  # noqa: F401,F403
from descriptools_amd import filters as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
