"""bwgr_amd -- MI355X (gfx950) Gibbs sweep engine behind bWGR's wgr()/KMUP and Bayes* samplers.

The numerical path is libbwgr_hip.so (hand-written HIP, C ABI in include/bwgr.h); this package is the host-side
mirror of the reference's R interface.  Importing the package does not need a GPU; calling it does.
"""
from .api import (Panel, Chain, Group, KMUP, KMUP2, BayesA, BayesB, BayesC, BayesL, BayesRR, BayesCpi, BayesDpi, BayesA2, BayesB2, BayesRR2, mcmcCV, fit_many, sample_rows, wgr, MODELS, emRR, emBA, emBB, emBC, emBCpi, emDE, emBL, emEN, emML, lasso, em_order,
                  debug_variates, debug_live, MRR3, MRR3F, mrr, mrr_float, K2X, mkr, mrr_dense_plan, sweep_plan, PEGS, PEGSZ, PEGSX, PEGS_sparse, PEGSZ_sparse, dense, sparse, pegs_plan, pegs_sparse_plan, pegsx_plan, pegs_launch_plan, pegsx_timing, uvbeta, uvb_plan, uvbeta_dense, uvbd_plan, panel_xb, XSEMF, ZSEMF, YSEMF, uvbeta2, solver2x, MEGA, GSEM, solver1x, solver1xF, UVBETA, FUVBETA, XFUVBETA, ZFUVBETA, GRM, GAU, EigenGRM, EigenGAU, EigenARC, crossprod, KERNELS, crossprod2, EigenArcZ, EigenGauZ, KERNELS2)
from ._lib import BwgrError, device_count

__all__ = ["Panel", "Chain", "Group", "KMUP", "KMUP2", "BayesA", "BayesB", "BayesC", "BayesL", "BayesRR", "BayesCpi", "BayesDpi", "BayesA2", "BayesB2", "BayesRR2", "mcmcCV", "fit_many", "emRR", "emBA", "emBB", "emBC", "emBCpi", "emDE", "emBL", "emEN", "emML", "lasso", "em_order", "sample_rows", "wgr",
           "MODELS", "BwgrError", "device_count", "debug_variates", "debug_live", "MRR3", "MRR3F", "mrr", "mrr_float", "K2X", "mkr", "mrr_dense_plan", "sweep_plan", "PEGS", "PEGSZ", "PEGSX", "PEGS_sparse", "PEGSZ_sparse", "dense", "sparse", "pegs_plan", "pegs_sparse_plan", "pegsx_plan", "pegs_launch_plan", "pegsx_timing", "uvbeta", "uvb_plan", "uvbeta_dense", "uvbd_plan", "panel_xb", "XSEMF", "ZSEMF", "YSEMF", "uvbeta2", "solver2x", "MEGA", "GSEM", "solver1x", "solver1xF", "UVBETA", "FUVBETA", "XFUVBETA", "ZFUVBETA", "GRM", "GAU", "EigenGRM", "EigenGAU", "EigenARC", "crossprod", "KERNELS", "crossprod2", "EigenArcZ", "EigenGauZ", "KERNELS2"]
