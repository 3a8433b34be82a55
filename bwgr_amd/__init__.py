"""bwgr_amd -- MI355X (gfx950) Gibbs sweep engine behind bWGR's wgr()/KMUP and Bayes* samplers.

The numerical path is libbwgr_hip.so (hand-written HIP, C ABI in include/bwgr.h); this package is the host-side
mirror of the reference's R interface.  Importing the package does not need a GPU; calling it does.
"""
from . import api
from .api import *  # noqa: F401,F403  (api.__all__ is the one list of public names)

__all__ = list(api.__all__)
