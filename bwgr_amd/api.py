"""Host-side mirror of the reference's R interface for the Gibbs hot path.

Same names, argument order, defaults and return-list element names/order as
  KMUP(X,b,d,xx,e,L,Ve,pi)                          R/RcppExports.R:4-6
  BayesA/BayesL/BayesRR/BayesCpi/BayesDpi(y,X,it=1500,bi=500,df=5,R2=0.5)   R/RcppExports.R:48-74
  BayesB/BayesC(y,X,it=1500,bi=500,pi=0.95,df=5,R2=0.5)
  wgr(y,X,it=1500,bi=500,th=1,bag=1,rp=FALSE,iv=FALSE,de=FALSE,pi=0,df=5,R2=0.5,eigK=NULL,VarK=0.95,verb=FALSE)
                                                    R/wgr.R:2-8
R is not available in the build image, so the host layer above the C ABI is Python (see
INTEGRATION.md for the R .Call shim that binds the same entry points).  Everything numerical happens in
libbwgr_hip.so on the GPU; this module only marshals arrays.  `seed=None` draws the seed from numpy's
global stream, so numpy.random.seed() plays the role of R's set.seed().
"""
from ._lib import BwgrError, device_count
from ._marshal import X_I8, X_F32, X_F64, HOST, DEVICE  # noqa: F401
from .panel import Panel, panel_xb
from .samplers import (MODELS, SWEEP_PLAN_FIELDS, Chain, KMUP, KMUP2, BayesA, BayesB, BayesC, BayesL, BayesRR, BayesCpi, BayesDpi, BayesA2, BayesB2,  # noqa: F401
                       BayesRR2, mcmcCV, fit_many, sample_rows, debug_variates, debug_live, sweep_plan)
from .group import Group
from .wgr_em import wgr, emRR, emBA, emBB, emBC, emBCpi, emDE, emBL, emEN, emML, lasso, em_order
from .mtfit import (MRR_KEYS, PEGS_KEYS, PEGSX_KEYS, MRR3, MRR3F, mrr, mrr_float, K2X, mkr, mrr_dense_plan, PEGS, PEGSZ, PEGSX, PEGS_sparse,  # noqa: F401
                    PEGSZ_sparse, dense, sparse, pegs_plan, pegs_sparse_plan, pegsx_plan, pegs_launch_plan, pegsx_timing)
from .uvfit import (UVB_KEYS, UVB2_KEYS, UVB_VARIANTS, uvbeta, uvb_plan, uvbeta_dense, uvbd_plan, XSEMF, ZSEMF, YSEMF, uvbeta2, solver2x, MEGA,  # noqa: F401
                    GSEM, solver1x, solver1xF, UVBETA, FUVBETA, XFUVBETA, ZFUVBETA)
from .kernels import KERNELS, KERNELS2, GRM, GAU, EigenGRM, EigenGAU, EigenARC, crossprod, crossprod2, EigenArcZ, EigenGauZ
# the helpers that tests and tools call stage by stage stay reachable here under the names they had before the split
from .samplers import _CV_FITS, _CV_NAMES, _cor_last  # noqa: F401
from .mtfit import _MRR_OPTS, _Eff, _pegs_effect  # noqa: F401
from .uvfit import _uvb_inputs, _uvb_panel, _uvb_dense, _uvb2_panel, _sem_latent, _mega_latent, _sem, _sem2  # noqa: F401

# The package's public names (bwgr_amd/__init__.py imports by this list).  The families live in panel, samplers, group, wgr_em, mtfit, uvfit and
# kernels, as the library's host files do; the constants imported above beside them are reached as bwgr_amd.api.NAME.
__all__ = ["Panel", "Chain", "Group", "KMUP", "KMUP2", "BayesA", "BayesB", "BayesC", "BayesL", "BayesRR", "BayesCpi", "BayesDpi", "BayesA2", "BayesB2", "BayesRR2", "mcmcCV", "fit_many", "emRR", "emBA", "emBB", "emBC", "emBCpi", "emDE", "emBL", "emEN", "emML", "lasso", "em_order", "sample_rows", "wgr",
           "MODELS", "BwgrError", "device_count", "debug_variates", "debug_live", "MRR3", "MRR3F", "mrr", "mrr_float", "K2X", "mkr", "mrr_dense_plan", "sweep_plan", "PEGS", "PEGSZ", "PEGSX", "PEGS_sparse", "PEGSZ_sparse", "dense", "sparse", "pegs_plan", "pegs_sparse_plan", "pegsx_plan", "pegs_launch_plan", "pegsx_timing", "uvbeta", "uvb_plan", "uvbeta_dense", "uvbd_plan", "panel_xb", "XSEMF", "ZSEMF", "YSEMF", "uvbeta2", "solver2x", "MEGA", "GSEM", "solver1x", "solver1xF", "UVBETA", "FUVBETA", "XFUVBETA", "ZFUVBETA", "GRM", "GAU", "EigenGRM", "EigenGAU", "EigenARC", "crossprod", "KERNELS", "crossprod2", "EigenArcZ", "EigenGauZ", "KERNELS2"]
