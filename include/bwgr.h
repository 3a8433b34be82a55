/*
 * include/bwgr.h -- C ABI of libbwgr_hip.so, the MI355X (gfx950) Gibbs sweep engine that stands
 * behind bWGR's wgr()/KMUP and the standalone Bayes* samplers.
 *
 * Plain pointers and sizes only; no torch / Rcpp / Eigen types.  Every entry point names the
 * reference interface it replaces (paths relative to the bWGR source tree).  The reference-side
 * binding (an R .Call shim, plus the ctypes stub used by this repo's host layer) is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - All functions return 0 (BWGR_OK) or a bwgr_status code; bwgr_last_error() gives the text.
 *     HIP failures never abort the process (the reference's BEGIN_RCPP/END_RCPP turns C++
 *     exceptions into R conditions, src/RcppExports.cpp:17,30; the shim maps non-zero to Rf_error).
 *   - Inputs are never modified unless documented as in/out; outputs are caller-allocated
 *     (the Rcpp glue passes every Eigen argument by value, src/RcppExports.cpp:20-27).
 *   - X is column-major n x p with leading dimension ldx (R / Eigen::MatrixXf layout).
 *   - `seed` replaces R's global RNG stream (Rcpp::RNGScope, src/RcppExports.cpp:19); the R
 *     front-end derives it from unif_rand() so set.seed() still governs repeatability.
 *   - There is no CPU fallback: without a gfx950 device every compute entry returns BWGR_ENODEV.
 */
#ifndef BWGR_H
#define BWGR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BWGR_ABI_VERSION 1

enum bwgr_status {
  BWGR_OK = 0,
  BWGR_EINVAL = 1,   /* bad argument */
  BWGR_EHIP = 2,     /* a HIP runtime call failed */
  BWGR_ENOMEM = 3,
  BWGR_ETIMEOUT = 4, /* an in-kernel workgroup exchange gave up (bounded spin) */
  BWGR_ENODEV = 5,   /* no usable GPU */
  BWGR_ERANGE = 6    /* a fixed-point sweep left its range and could NOT be redone.  Since round 3 a sweep of the single-chain entry
                        points that leaves the range is redone on the fp64 residual from the state it started with and the chain goes
                        on (bwgr_chain_redo_count says how often); this status remains for the paths without that recovery: a pair
                        sweep (bwgr_chain_run_pair -- run the two chains unpaired instead; the host layer's fit_many does), the debug
                        abort hook, and a recovery whose snapshot could not be allocated.  The chain's state is then invalid. */
};
enum bwgr_xtype { BWGR_X_I8 = 0, BWGR_X_F32 = 1, BWGR_X_F64 = 2 }; /* F64 (an R numeric matrix) is narrowed
                                                                     to float on upload, as the Rcpp glue does
                                                                     on every call (src/RcppExports.cpp:20) */
enum bwgr_memloc { BWGR_HOST = 0, BWGR_DEVICE = 1 };
enum bwgr_model {
  BWGR_BAYESA = 0,   /* src/Rcpp20260726ai.cpp:589-635 */
  BWGR_BAYESB = 1,   /* :638-699 */
  BWGR_BAYESC = 2,   /* :702-759 */
  BWGR_BAYESL = 3,   /* :762-809 */
  BWGR_BAYESRR = 4,  /* :812-855 */
  BWGR_BAYESCPI = 5, /* :858-921 */
  BWGR_BAYESDPI = 6  /* :924-987 */
};
enum bwgr_rng_mode { BWGR_RNG_PHILOX = 0, BWGR_RNG_DEGENERATE = 1 /* z=0, chi2=mean, u=0.5 (tests) */ };

typedef struct bwgr_panel bwgr_panel; /* genotype matrix resident in HBM + per-marker setup */
typedef struct bwgr_chain bwgr_chain; /* one MCMC chain: residual, effects, variances, posterior sums */

int bwgr_abi_version(void);
const char *bwgr_last_error(void);
int bwgr_device_count(int *count);

/* ---- panel: X staged once, column-major in HBM ------------------------------------------------
 * Replaces the per-call SEXP -> Eigen::MatrixXf conversion of X (src/RcppExports.cpp:20, :198 ...).
 * block = markers per exact block (0 = auto, <= 128); nwg = row-slab workgroups (0 = auto).
 * Builds xx, vx, MSx (src/Rcpp20260726ai.cpp:593-598) and the block-diagonal Gram used by the
 * blocked sweep.
 * The Gram arrays of an int8 panel are exact int32 sums over all rows, so an int8 panel needs
 * n * max(max|x|, 1)^2 < 2^31 (131 071 rows at |x| = 128, 536 870 911 on 0/1/2 codes); one that does not is
 * refused with BWGR_EINVAL ("... does not fit the int32 Gram").  The same bound, with the rows of the
 * subsample and the panel's max|x|, holds for the scratch panels of bwgr_kmup2 and of bwgr_wgr's bagging,
 * whose row count may exceed n, and refuses those calls the same way. */
int bwgr_panel_create(bwgr_panel **out, const void *X, int xtype, int memloc, int64_t n, int64_t p, int64_t ldx,
                      int device, int block, int nwg);
int bwgr_panel_destroy(bwgr_panel *P);
int bwgr_panel_set_stream(bwgr_panel *P, void *hip_stream); /* NULL = the default stream */
/* A second handle on the same resident genotypes: shares X, the Gram arrays and xx/vx with `src` (read-only during
 * sweeps) and owns its own sweep scratch and its own non-blocking stream, so chains on `src` and on its clones run
 * side by side on disjoint compute units (a sweep occupies nwg + 1 + feeders of the 256).  This is how the callers
 * that fit many models on one X -- mcmcCV's folds x models loop, R/cv.R:113-216 -- fill the chip.  Destroy the clones
 * before `src`.  bwgr_panel_max_concurrent: how many sweeps of this geometry fit at once; for selection models on a panel
 * with k_sweep3 it counts the larger of the two engines a chain may run (K3 + 1, or nwg + 1 + feeders above the engine
 * threshold).  bwgr_panel_max_pairs: how many pairs (bwgr_chain_run_pair, K3 + 2 units each) fit, 0 without k_sweep3.
 *
 * Occupancy guard: a sweep's workgroups wait for one another, so all of them have to be resident at once, beside the
 * sweeps other handles (panels, clones, pairs) have in flight on other streams of the same device.  Every sweep entry
 * point checks that before it enqueues anything -- grid against hipOccupancyMaxActiveBlocksPerMultiprocessor x compute
 * units, less the units of the sweeps in flight -- and returns BWGR_EINVAL if the launch would not fit (the chain is left
 * as it was; wait for the others and call again).  Without the guard such a launch spins to BWGR_ETIMEOUT.
 * BWGR_OCC_GUARD=0 switches it off.  bwgr_debug_occupancy_fits is the guard's arithmetic (a host function: `grid`
 * workgroups at `per_cu` per unit need ceil(grid / per_cu) units, which must fit `cus` less `busy`). */
int bwgr_panel_clone(bwgr_panel **out, bwgr_panel *src);
int bwgr_panel_max_concurrent(const bwgr_panel *P, int selection, int *count);
int bwgr_panel_max_pairs(const bwgr_panel *P, int *pairs);
int bwgr_debug_occupancy_fits(int grid, int per_cu, int cus, int busy, int *need);
/* host arithmetic of one more launch rule: the LDS-DMA streamers of k_sweep3 address a launch's columns by 32-bit lane offsets, so a
 * launch over `ncols` columns of `slab_rows`-row slabs takes them only while ncols * slab_rows < 2^32 (else the register-path streamers
 * with 64-bit offsets).  Returns 1 / 0. */
int bwgr_debug_stream3_dma(int64_t ncols, int64_t slab_rows);
/* which instantiation of the trajectory engine a selection sweep of the whole panel is launched as, the panel as it stands (clones alive, centred or
 * not): *which = 0 none (another engine's), 1 k_sweep3 (any shape), 2 k_sweep3f (the fixed shape: 128-marker blocks, 16-bit Gram entries, 128-row DMA
 * streamers; BWGR_FIXED3=0 when the root panel is made: never).  Both run the same chain bit for bit. */
int bwgr_debug_sweep3_kernel(const bwgr_panel *P, int *which);
/* geometry actually chosen: info[0]=n, [1]=p, [2]=ld (padded rows), [3]=block, [4]=nwg, [5]=slab rows,
 * [6]=bytes of X resident, [7]=bytes of Gram resident */
int bwgr_panel_info(const bwgr_panel *P, int64_t info[8]);
/* how a sweep over this panel is pipelined (no reference counterpart; reporting only): info[0]=kernel generation (1 k_sweep,
 * 2 k_sweep2, 3 k_sweep3 -- selection sweeps of sparse chains --, 4 k_sweep2w -- affine sweeps as a triangular product --),
 * [1]=pipeline depth in blocks (a block's dots lag the chain by this many blocks), [2]=q feeder workgroups,
 * [3]=bits of the Gram entries the sequencer stages (16|32; 0 for float panels).  selection != 0: BayesB/C/Cpi/Dpi-type
 * sweeps (inclusion indicators), else the affine ones (BayesA/L/RR). */
int bwgr_panel_pipeline(const bwgr_panel *P, int selection, int info[4]);
/* xx[j] = |X_j|^2, vx[j] = fvar(X_j), MSx = sum vx   (host outputs; any may be NULL) */
int bwgr_panel_stats(bwgr_panel *P, float *xx, float *vx, float *MSx);

/* ---- KMUP: one Gibbs sweep over all markers ---------------------------------------------------
 * Replaces SEXP KMUP(X,b,d,xx,e,L,Ve,pi), src/Rcpp20260726ai.cpp:12-38 / _bWGR_KMUP,
 * src/RcppExports.cpp:16-31.  b, d (p) and e (n) are in/out host vectors; xx, L (p) inputs.
 * `iter` is the iteration word of the RNG counter (wgr passes its loop index - 1).
 * Inclusion probability uses the stable form 1/(1+pi/(1-pi)*exp(C(|e2|^2-|e1|^2))), which equals the
 * reference's cj/(cj+dj) wherever that does not underflow to NaN. */
int bwgr_kmup(bwgr_panel *P, float *b, float *d, const float *xx, float *e, const float *L, float Ve, float pi,
              uint64_t seed, uint32_t iter, int rng_mode);

/* ---- KMUP2: the same sweep on a row subsample -----------------------------------------------------
 * Replaces SEXP KMUP2(X,Use,b,d,xx,E,L,Ve,pi), src/Rcpp20260726ai.cpp:41-77 / _bWGR_KMUP2,
 * src/RcppExports.cpp:34-50 (R/RcppExports.R:8-10).  Use: nuse 0-based row ids of the resident panel (wgr passes
 * sort(sample(n, n*bag, rp)) - 1, R/wgr.R:68); b, d (p) in/out; xx, L (p) and E (the panel's n rows) inputs; e_out
 * receives the nuse residuals of the subsample (:76).  Reference quirks kept: the conditional mean's numerator adds b0,
 * not xx*b0, and the denominator is xx*bg + L with bg = n/nuse (:47, :59). */
int bwgr_kmup2(bwgr_panel *P, const int *Use, int64_t nuse, float *b, float *d, const float *xx, const float *E,
               float *e_out, const float *L, float Ve, float pi, uint64_t seed, uint32_t iter, int rng_mode);

/* ---- fused chains: BayesA/B/C/L/RR/Cpi/Dpi ---------------------------------------------------------
 * Replaces SEXP Bayes*(y, X, it, bi, [pi,] df, R2), src/Rcpp20260726ai.cpp:589-987 /
 * _bWGR_BayesA.._bWGR_BayesDpi, src/RcppExports.cpp:177-290.  y: n floats (host or device per
 * memloc).  it/bi are floats cast to int, as in the reference (:611, :642).  pi is ignored by
 * A/L/RR/Cpi/Dpi. */
int bwgr_chain_create(bwgr_chain **out, bwgr_panel *P, int model, const float *y, int memloc, float it, float bi,
                      float pi, float df, float R2, uint64_t seed, int rng_mode);
int bwgr_chain_destroy(bwgr_chain *C);
/* run the next `iters` MCMC iterations (sweep + intercept + variance draws + posterior sums);
 * asynchronous on the panel's stream */
int bwgr_chain_run(bwgr_chain *C, int iters);
/* Two chains of one resident panel (one on the panel, one on a clone of it -- or on two clones) advanced in lockstep, `iters`
 * iterations each: one set of streamer workgroups, one pass over the genotypes, serves both (k_sweep3p); each chain's results are
 * bit-identical to a run of its own.  Selection models (BayesB/C/Cpi/Dpi) on int8 panels that have k_sweep3; BWGR_EINVAL otherwise.
 * No reference counterpart: this is how the callers that fit many models on one X (mcmcCV, /root/reference/R/cv.R:113-216; replicate
 * chains) use fewer compute units per chain. */
int bwgr_chain_run_pair(bwgr_chain *C0, bwgr_chain *C1, int iters);
/* wait for the stream and report in-kernel exchange failures */
int bwgr_chain_sync(bwgr_chain *C);
/* iterations completed so far */
int bwgr_chain_iterations(const bwgr_chain *C, int *done);
/* posterior means and fitted values, the reference's return list (host outputs, any may be NULL):
 *   mu, b[p], d[p], hat[n], vb[p] (A/B/L/Dpi) or vb[1] (C/RR/Cpi), ve, h2, MSx, pi (Cpi/Dpi), PVAL[p] */
int bwgr_chain_result(bwgr_chain *C, float *mu, float *b, float *d, float *hat, float *vb, float *ve, float *h2,
                      float *MSx, float *pi, float *pval);
/* current chain state (host outputs, any may be NULL): b[p], d[p], e[n], vb[p] (common variance
 * replicated), scal[4] = {mu, ve, vb_common, pi} */
int bwgr_chain_state(bwgr_chain *C, float *b, float *d, float *e, float *vb, float *scal);
/* device-time of the sweep kernel alone, averaged over the launches since the last call (ms);
 * measured with hipEvents on the stream the kernel runs on */
int bwgr_chain_sweep_ms(bwgr_chain *C, float *avg_ms, int *launches);
/* sweeps of this chain that left the fixed-point range of their engine and were redone on the fp64 residual (the reference's update,
 * src/Rcpp20260726ai.cpp:681, has no such failure: the redo keeps the chain the same chain; this only reports how often it happened) */
int bwgr_chain_redo_count(bwgr_chain *C, int *count);

/* ---- marker-sharded chains (one rank per GPU) ----------------------------------------
 * The panel holds this rank's columns [marker0, marker0 + p_local) of a p_total-marker panel; the residual is
 * replicated on every rank in e_ext (device, `ld` doubles from bwgr_panel_info, caller-owned, e.g. a torch tensor,
 * so that the caller can all-reduce residual deltas with RCCL between block ranges).  RNG counters use global marker
 * ids, MSx_total is the all-rank sum of the panels' MSx.  An iteration is then
 *     for each range: bwgr_chain_sweep_blocks(C, lo, hi); <caller: all-reduce (e - e_at_range_start)>;
 *     bwgr_chain_get_sums(C, s); <caller: all-reduce s>; bwgr_chain_end_iteration(C, s_total);
 * With one rank and one range this is exactly bwgr_chain_run(C, 1).  With several ranks markers on different ranks
 * are updated against a residual that is only synchronised at range boundaries: a partitioned Gibbs sampler, NOT
 * the reference's chain (parity is statistical). */
int bwgr_chain_create_sharded(bwgr_chain **out, bwgr_panel *P, int model, const float *y, int memloc, float it, float bi,
                              float pi, float df, float R2, uint64_t seed, int rng_mode, int64_t marker0,
                              int64_t p_total, float MSx_total, double *e_ext);
int bwgr_chain_sweep_blocks(bwgr_chain *C, int blk_begin, int blk_end);
/* one exchange round in two calls: round_sweep remembers e, sweeps [blk_begin, blk_end) (empty range: nothing) and writes
 * delta = e - e_before to delta_dev (ld doubles, device); the caller all-reduces delta; round_apply sets e = e_before + delta */
int bwgr_chain_round_sweep(bwgr_chain *C, int blk_begin, int blk_end, double *delta_dev);
/* device-side forms of get_sums / end_iteration(sums_total): sums_dev = two doubles on the chain's device, all-reduced in place */
int bwgr_chain_get_sums_dev(bwgr_chain *C, double *sums_dev);
int bwgr_chain_end_iteration_dev(bwgr_chain *C, const double *sums_total_dev);
int bwgr_chain_round_apply(bwgr_chain *C, const double *delta_dev);
int bwgr_chain_get_sums(bwgr_chain *C, double sums[2]);              /* {sum d, sum b^2} of this rank's sweep */
int bwgr_chain_end_iteration(bwgr_chain *C, const double sums_total[2]); /* NULL: use this rank's own sums */

/* one-call form: create + run(it) + result + destroy */
int bwgr_bayes(bwgr_panel *P, int model, const float *y, float it, float bi, float pi, float df, float R2,
               uint64_t seed, int rng_mode, float *mu, float *b, float *d, float *hat, float *vb, float *ve,
               float *h2, float *MSx, float *pi_out, float *pval);

/* ---- two-effect samplers ---------------------------------------------------------------------------
 * Replaces BayesA2 / BayesB2 / BayesRR2(y, X1, X2, it, bi, [pi,] df, R2), src/Rcpp20260726ai.cpp:990-1218: one
 * residual, two resident panels with the same rows swept one after the other in every iteration, each with its own
 * prior scale and variance(s).  base_model = BWGR_BAYESA, BWGR_BAYESB or BWGR_BAYESRR.  Both panels must have been
 * created on the same device with the same slab geometry (same n, block and nwg).  Panel-2 markers carry the RNG ids
 * p1 .. p1+p2-1.  Outputs as the reference's return lists: mu, b1[p1], b2[p2], vb1 / vb2 (p_k entries for A2 and B2,
 * one for RR2), d1[p1], d2[p2] (B2 only; may be NULL otherwise), ve, hat[n], h2. */
int bwgr_bayes2(bwgr_panel *P1, bwgr_panel *P2, int base_model, const float *y, float it, float bi, float pi, float df,
                float R2, uint64_t seed, int rng_mode, float *mu, float *b1, float *d1, float *vb1, float *b2, float *d2,
                float *vb2, float *ve, float *hat, float *h2);

/* Host-only helper of the RNG contract: the k row indices (0-based, ascending) that `sort(sample(n, k, rp))` selects
 * for (seed, iter) -- what wgr's bagging (R/wgr.R:68) and the cross-validation folds of mcmcCV (R/cv.R:118-121) draw
 * from R's stream in the reference.  Does not touch the GPU. */
int bwgr_sample_rows(uint64_t seed, uint32_t iter, int64_t n, int64_t k, int rp, int *rows);

/* ---- wgr(): the R-level driver, device-resident ---------------------------------------------------
 * Replaces the iteration body and setup/teardown of wgr(), R/wgr.R:41-168 (bag = 1, eigK = NULL in
 * this round).  y is the R numeric vector (double).  Outputs as wgr's return list: mu, b[p],
 * Vb[p] (iv/de) or Vb[1], d[p], Ve, hat[n], cxx. */
int bwgr_wgr(bwgr_panel *P, const double *y, int it, int bi, int th, int iv, int de, double pi, double df, double R2,
             uint64_t seed, int rng_mode, double *mu, double *b, double *Vb, double *d, double *Ve, double *hat,
             double *cxx);
/* wgr() with the polygenic kernel term (eigK, R/wgr.R:23-32,70-78,116-119,148-150): U = the first pk eigenvectors
 * of the kernel (n x pk doubles, column-major, host), V their eigenvalues (the caller applies VarK: pk =
 * which.max(cumsum(V)/length(V) > VarK)).  Each iteration first sweeps KMUP(U,h,dh,xxK = 1,e,Lk = Ve/(V*Vk),Ve,0),
 * then the markers.  Extra outputs as in wgr's list: u[n] = U %*% H, Vk.  U == NULL, bag == 1 is bwgr_wgr.
 * bag != 1 (R/wgr.R:20,46,68,85,121): every iteration sweeps KMUP2 (src/Rcpp20260726ai.cpp:41-77) on
 * sort(sample(n, n*bag, rp)) rows -- the subsample is drawn from the RNG contract (purpose 20), a panel of those rows
 * and its Gram blocks are rebuilt on the device per iteration, df is divided by bag^2 and xx multiplied by bag as in R.
 * bag != 1 together with eigK is refused: the reference indexes the subsampled residual out of bounds there. */
int bwgr_wgr_ex(bwgr_panel *P, const double *y, int it, int bi, int th, int iv, int de, double pi, double df, double R2,
                uint64_t seed, int rng_mode, const double *U, const double *V, int64_t pk, double bag, int rp, double *mu,
                double *b, double *Vb, double *d, double *Ve, double *hat, double *cxx, double *u, double *Vk);

/* ---- EM / Gauss-Seidel family --------------------------------------------------------
 * Replaces SEXP emRR(y,gen,df,R2) src/Rcpp20260726ai.cpp:308-354, emBA(y,gen,df,R2) :80-128, emBB(y,gen,df,R2,Pi) :131-187,
 * emBC(y,gen,df,R2,Pi) :190-247, emBCpi(y,gen,df,R2,Pi) :1502-1545, emDE(y,gen,R2) :250-305, emBL(y,gen,R2,alpha) :357-397,
 * emEN(y,gen,R2,alpha) :400-460, emML(y,gen,D) :463-521, lasso(y,gen) :1463-1500 (_bWGR_emRR ... in src/RcppExports.cpp).  Deterministic
 * coordinate updates in the marker order the reference re-shuffles before every sweep with std::shuffle(order,
 * std::mt19937(i)) (emBCpi sweeps in natural order): the library makes the same standard-library call, gathers the
 * resident panel into that order on the device, rebuilds the Gram blocks and runs the sweep kernel with the variates
 * switched off (affine members) or with the member's own coordinate update in the recurrence (soft selection: emBB /
 * emBC / emBCpi; soft threshold: emEN, emBL).  par = Pi (emBB / emBC / emBCpi; reference default 0.75) or alpha (emBL /
 * emEN; 0.02).  maxit = 0: the reference's count (200 sweeps; emDE / emML / emEN up to 300 with their convergence
 * tests).  D: emML's optional marker weights (p floats) or NULL.  Outputs (host): mu, b[p], d[p] (soft-selection
 * members; may be NULL), hat[n], vbvec[p] (emBA / emBB / emDE: Vb; may be NULL), scal[6] = emRR {Va, Ve, h2}, emBA / emBB /
 * emDE {0, Ve, h2}, emML {Vb, Ve, h2, Va}, emBC {Va, Ve, h2, Vg}, emBCpi {Va, Ve, h2, Vg, pi}, emBL {0, 0, h2},
 * emEN {Va, Ve, h2}, lasso {Lmb, 0, h2}; iters = sweeps run.  lasso(y,gen) :1463-1500 sweeps in natural order; its
 * penalty is re-estimated after every sweep from the per-marker yx the sweep hands back (host loop, as the reference). */
enum { BWGR_EM_RR = 0, BWGR_EM_BA = 1, BWGR_EM_DE = 2, BWGR_EM_ML = 3, BWGR_EM_BB = 4, BWGR_EM_BC = 5, BWGR_EM_BCPI = 6,
       BWGR_EM_BL = 7, BWGR_EM_EN = 8, BWGR_EM_LASSO = 9 };
int bwgr_em(bwgr_panel *P, int model, const float *y, float df, float R2, float par, const float *D, int maxit, float *mu,
            float *b, float *d, float *hat, float *vbvec, float *scal, int *iters);
/* the marker order of sweep `upto` (0-based): the identity shuffled with std::mt19937(0), (1), ... (upto) (host only) */
int bwgr_em_order(int64_t p, int upto, int32_t *order);

/* ---- multi-trait ridge regression (mrr / mrr_float) ------------------------------------------------------
 * Replaces SEXP MRR3(Y,X,maxit,tol,...) src/RcppEigen20230423.cpp:318-700 and MRR3F :704-1080 (R/mix.R:1271-1273: mrr = MRR3,
 * mrr_float = MRR3F).  With the non-linear factor at 0 the two are one algorithm; one fp64 engine serves both.  Y: n x k column-major
 * doubles, NaN = missing (Z = 0, :745-749); 1 <= k <= 16.  X: the panel's int8 genotypes, centred by their all-rows column means as
 * the reference does (:763-765), so an uncentred and a centred copy of the same genotypes give the same fit; a panel switched to
 * implicit centring (bwgr_panel_set_centred) gives the same result as before the switch.  fp32 panels are refused.
 * opts[BWGR_MRR_*] (nopts of them; the rest take the reference's defaults, which BWGR_MRR_DEFAULTS lists in order).  Supported:
 * maxit, tol, TH, HCS, XFA, ACS, NumXFA, R2, gc0, df0, updateMu, weight_prior_h2, weight_prior_gc, OneVarB, OneVarE, DeflateMax
 * (read only with DeflateBy), verbose (host prints); cores is not an option (ignored by the R front-ends).  Refused with
 * BWGR_EINVAL when not at their default: InnerGS, NoInv, NLfactor / NonLinearFactor, PenCor, MinCor, uncorH2below, roundGCupFrom,
 * roundGCupTo, roundGCdownFrom, roundGCdownTo, bucketGCfrom, bucketGCto, DeflateBy.
 * Outputs (host, caller-allocated, in the reference's order :1066-1078): mu[k], b[p x k], hat[n x k] (X_c b + mu for every row, the
 * missing ones included), h2[k], GC[k x k], vb[k x k], ve[k], MSx[k], cnvB / cnvH2 / cnvV [maxit] (the first *its are set), its.
 * b_Weights is all ones (no non-linear factor) and left to the caller. */
enum { BWGR_MRR_MAXIT = 0, BWGR_MRR_TOL, BWGR_MRR_TH, BWGR_MRR_NLFACTOR, BWGR_MRR_INNERGS, BWGR_MRR_NOINV, BWGR_MRR_HCS, BWGR_MRR_XFA,
       BWGR_MRR_ACS, BWGR_MRR_NUMXFA, BWGR_MRR_R2, BWGR_MRR_GC0, BWGR_MRR_DF0, BWGR_MRR_UPDATEMU, BWGR_MRR_WEIGHT_PRIOR_H2,
       BWGR_MRR_WEIGHT_PRIOR_GC, BWGR_MRR_PENCOR, BWGR_MRR_MINCOR, BWGR_MRR_UNCORH2BELOW, BWGR_MRR_ROUNDGCUPFROM, BWGR_MRR_ROUNDGCUPTO,
       BWGR_MRR_ROUNDGCDOWNFROM, BWGR_MRR_ROUNDGCDOWNTO, BWGR_MRR_BUCKETGCFROM, BWGR_MRR_BUCKETGCTO, BWGR_MRR_DEFLATEMAX,
       BWGR_MRR_DEFLATEBY, BWGR_MRR_ONEVARB, BWGR_MRR_ONEVARE, BWGR_MRR_VERBOSE, BWGR_MRR_NOPTS };
#define BWGR_MRR_MAXK 16
#define BWGR_MRR_DEFAULTS {500, 10e-9, 0, 0, 0, 0, 0, 0, 0, 3, 0.5, 0.5, 1.0, 0, 0.01, 0.01, 0, 1.0, 0, 1.0, 1.0, 1.0, 0, 1.0, 1.0, 0.9, 0, 0, 0, 0}
int bwgr_mrr(bwgr_panel *P, const double *Y, int k, const double *opts, int nopts, double *mu, double *b, double *hat, double *h2,
             double *GC, double *vb, double *ve, double *MSx, double *cnvB, double *cnvH2, double *cnvV, int *its);
/* host arithmetic of bwgr_mrr's LDS plan for k traits with npat distinct missingness patterns (1 <= npat <= k <= 16, else
 * BWGR_EINVAL; needs no GPU): linv_lds = 1 when the per-block solve keeps the markers' k x k inverses in LDS (else it fetches each
 * marker's row of its inverse from global memory, one marker ahead); ngl = how many of the block's per-pattern Gram matrices it stages
 * in LDS (patterns ngl..npat-1 are read from global memory); the dynamic LDS bytes of the solve and of the inverses' kernel.  Any
 * output may be NULL. */
int bwgr_debug_mrr_plan(int k, int npat, int *linv_lds, int *ngl, int64_t *solve_lds_bytes, int64_t *linv_lds_bytes);
/* ---- mrr on a dense fp64 design: mrr(Y, dense(X)), mkr(Y, K) = MRR3(Y, K2X(K)) (R/mix.R:1275) -------------------------
 * bwgr_mrr's algorithm, options, defaults, refusals and outputs (b is r x k) on an n x r matrix of doubles instead of a panel: real-valued
 * dosages, or the eigenvector design K2X makes of a relationship matrix (the host layers decompose; bwgr_amd.K2X, bwgr_amd.mkr).  X is
 * column-major with column stride ldx, in host memory (memloc = BWGR_HOST) or on `device` (BWGR_DEVICE); the engine keeps its own copy,
 * centred once by the all-rows column means (:763-765), so X is not changed.  A host X is checked for non-finite entries; for a device X
 * that is the caller's duty (a NaN or Inf there spreads through the fit).  The launch train is bwgr_mrr's with fp64 kernels (DESIGN.md
 * section 4.13); two calls give the same bits, and a device X gives the bits of the same values on the host.
 * BWGR_EINVAL: a null required pointer, a bad memloc, what bwgr_mrr refuses of k and the options, r < 1 or r > 2147483392, n < 2, ldx < n,
 * a non-finite entry of a host X, a trait of Y with fewer than two records, a workspace (bwgr_debug_mrr_dense_plan) beyond the device's
 * free memory. */
int bwgr_mrr_dense(int device, const double *X, int memloc, int64_t n, int64_t r, int64_t ldx, const double *Y, int k, const double *opts, int nopts,
                   double *mu, double *b, double *hat, double *h2, double *GC, double *vb, double *ve, double *MSx, double *cnvB, double *cnvH2,
                   double *cnvV, int *its);
/* host arithmetic of bwgr_mrr_dense's plan (needs no GPU) for n rows, r columns, k traits and npat missingness patterns (n >= 2,
 * 1 <= r <= 2147483392, 1 <= npat <= k <= 16, else BWGR_EINVAL).  out[0] ld, the rows padded to 128; out[1] the 64-column blocks of a
 * sweep; out[2] the columns of the last block; out[3] the 64-row tiles; out[4] the workgroups of k_mrrd_pass; out[5] the tiles one of them
 * takes at most; out[6] the workgroups of k_mrrd_centre and k_mrrd_setup (one column per wave); out[7] those of k_mrrd_hat; out[8] linv_lds
 * and out[9] ngl of the solve, as in bwgr_debug_mrr_plan, with 32 KB per pattern's Gram; out[10..13] the LDS bytes of k_mrrd_gram and
 * k_mrrd_pass (static), k_mrrd_solve and k_mrr_linv (dynamic); out[14] the bytes of the call's device workspace.  k_mrrd_gram runs
 * out[1] x npat workgroups. */
#define BWGR_MRR_DENSE_PLAN_NOUT 15
int bwgr_debug_mrr_dense_plan(int64_t n, int64_t r, int k, int npat, int64_t out[BWGR_MRR_DENSE_PLAN_NOUT]);
/* ---- mrr_svd: the multi-trait fit in the panel's principal components (src/RcppEigen20230423.cpp:1083-1260, R/RcppExports.R:188) ----
 * bwgr_mrr_svd_fit is the reference's Gauss-Seidel (:1103-1243) on a given n x r design X (for mrr_svd: U diag(d), the left singular vectors of
 * the centred marker matrix times its singular values; the host layers decompose, bwgr_amd.svd).  It is a fit with one effect on
 * bwgr_mrr_dense's block train: X, memloc, ldx, the engine's own copy, the workspace and two calls giving the same bits are as there.  Every sweep
 * walks the columns in their natural order 0 .. r-1 (:1176).  Start: ve = vy / 2, vb = diag(ve / MSx), h2 = 1 - ve / vy.  After a sweep:
 * ve_t = e_t'y_t / (n_t - 1) with no prior, h2 again, TildeHat = b'(Dinv o tilde) and TrDinvXSX_t = sum_j XSX_jt Dinv_jt with
 * Dinv_jt = 1 / (XSX_jt / ve_t + iG_tt), XSX the n_t-scaled one, this iteration's ve and the sweep's iG; vb_ii = TH_ii / Tr_i,
 * vb_ij = (TH_ij + TH_ji) / (Tr_i + Tr_j); where vb's smallest eigenvalue is below 0, fabs(1.1 min) goes onto its diagonal; iG = pinv(vb).
 * cnvB = log10 sum_jt (delta b_jt)^2 (the sum over the traits), cnvH2 and cnvV as :1220-1221 (maxit values each, or null); the loop ends at
 * cnvB < log10(tol) or at a NaN, which is counted in *its.  mu (the traits' means over their records) is never updated; GC = vb_ij /
 * sqrt(vb_ii vb_jj) at the end; hat = X b + mu for every row (n x k, or null); b is r x k.  The reference does not centre X; the train
 * centres its copy by the all-rows column means, which for the design above are 0 up to rounding (W_c has zero column sums, so 1'U = 0
 * wherever d > 0).  The reference's float arithmetic is fp64 here.
 * BWGR_EINVAL: what bwgr_mrr_dense refuses of its pointers, memloc, n, r, ldx, X, the traits and the workspace; k < 1 or k > 16; maxit < 0. */
int bwgr_mrr_svd_fit(int device, const double *X, int memloc, int64_t n, int64_t r, int64_t ldx, const double *Y, int k, int maxit, double tol, int verbose,
                     double *mu, double *b, double *hat, double *h2, double *GC, double *vb, double *ve, double *cnvB, double *cnvH2, double *cnvV, int *its);
/* out (p x k, column stride ldo >= p) = X'A on the raw codes of an int8 panel (centre = 0) or X_c'A with X_c = X - 1 xbar' (centre = 1);
 * A: n x k, column stride lda >= n; both in host memory (memloc = BWGR_HOST) or both on the panel's device (BWGR_DEVICE: the caller's arrays,
 * read and written on the panel's stream, asynchronously).  centre = 0: out[j, t] = sum_i x_ij a_it.  centre = 1: fma(-xbar_j, s_t, that sum),
 * xbar_j = the exact integer column sum divided by n, s_t = sum_i a_it summed on the device as 256 partial sums (partial q takes the rows
 * q, q + 256, ... in ascending order) added in ascending q: the panel stays int8.  Any k >= 1: the traits go in groups of 16, one pass over
 * X per group.  A workgroup owns whole columns over all rows, so nothing is reduced across workgroups and no sum is formed by atomics: the
 * order of an output's sum depends on n and the panel's slab height alone, two calls give the same bits, a host A and a device A give the same
 * bits, and a column gives the same bits in any panel of the same rows and slab height.
 * BWGR_EINVAL: a null pointer, k < 1 (or beyond 1 048 560), a bad memloc, lda < n, ldo < p, an fp32 panel, a non-finite entry of a host A
 * (for a device A that is the caller's duty). */
int bwgr_panel_xta(bwgr_panel *P, const double *A, int64_t lda, int64_t k, int centre, int memloc, double *out, int64_t ldo);
/* host arithmetic of bwgr_panel_xta's plan (needs no GPU) for n rows, p columns, k columns of A and slabs of R rows (a multiple of 128, at
 * most 4096; else BWGR_EINVAL): out[0] the trait groups; out[1] the columns a workgroup owns and out[2] those of one wave; out[3] the
 * workgroups per trait group and out[4] the column blocks one of them takes at most; out[5] the LDS bytes of k_xta (static); out[6] the rows
 * of a tile and out[7] the tiles; out[8] the bytes of the call's device workspace (a host call adds its copies of A and of the result). */
#define BWGR_XTA_PLAN_NOUT 9
int bwgr_debug_xta_plan(int64_t n, int64_t p, int64_t k, int64_t R, int64_t out[BWGR_XTA_PLAN_NOUT]);
/* ---- MLM: the multi-trait fit with fixed effects, Z projected off X (src/RcppEigen20230423.cpp:1260-1407, R/RcppExports.R:192) ----
 * bwgr_project: out = Zp = Z - X C, C = (X'X)^-1 X'Z over all n rows (:1287-1288).  Z is the int8 panel P (then Z, zloc and ldz are not read,
 * and n and p must be the panel's), or with P null an n x p fp64 matrix of column stride ldz >= n in host memory (zloc = BWGR_HOST) or on
 * `device` (BWGR_DEVICE).  X: n x f fp64 in host memory, column stride ldx >= n, 1 <= f <= 256.  out: n x p, column stride ldo >= n, in host
 * memory or on the device (oloc).  Z'X is bwgr_panel_xta's raw product on a panel and a kernel of the same summation order on a dense Z; X'X
 * and the f x f solve are fp64 on the host (a symmetric eigen-decomposition); Zp[i, j] is the chain acc = (double) z_ij; for l = 0 .. f-1:
 * acc = fma(-x_il, c_lj, acc), whose order depends on (i, j, f) alone: two calls, a host and a device Z, a column alone or within a wider call
 * and panels of different slab heights give the same bits.
 * bwgr_mlm: the fit.  Y: n x k, NaN = missing, 1 <= k <= 16.  Per trait MU_t = (M_t'M_t)^-1 M_t'Y_t on its rows (M_t: X there) and
 * y_t = (Y_t - M_t MU_t) o W_t; Zp as above, kept as the block train's padded fp64 copy (bwgr_mrr_dense's train, nothing centred): n p 8 bytes
 * and more, see bwgr_debug_mlm_plan.  ZZ_jt = sum of zp_ij^2 on trait t's rows, TrZSZ = colSums(ZZ), iN = 1 / (n_t - f), vy = y_t'y_t iN,
 * ve = vy / 2, vb = diag(ve / (TrZSZ iN)), Sb = df0 vb, Se = df0 ve, iNp = 1 / (n_t + df0 - f).  Sweep s walks the columns in the order of
 * bwgr_em_order(p, s) with LHS = iG + diag(ZZ_j / ve); then ve = (e'y + Se) iNp, vb_ii = (TH_ii + Sb_ii) / (TrZSZ_i + df0),
 * vb_ij = (TH_ij + TH_ji) / (TrZSZ_i + TrZSZ_j), bending (inflate becomes fabs(1.1 min) when vb's smallest eigenvalue is below 0.001 and that
 * exceeds inflate; it only grows and goes onto the diagonal in every sweep), iG = pinv(vb), cnv = log10 sum (delta u)^2.
 * The stopping rule is the reference's: with verb = 0 the loop stops only on a NaN, so it runs maxit sweeps; with verb = 1 it also stops at
 * cnv < logtol, and prints.  maxit = 0 returns the start: u = 0, cnv = 10, its = 0.
 * Outputs: b = MU (f x k), u (p x k), hat = Zp u + X MU on every row (n x k), h2 = 1 - ve / vy, GC, vb (k x k), ve, *cnv, *its; only u and its
 * are required.  The reference's float arithmetic is fp64 here; its (X'X)^-1 and (M_t'M_t)^-1 are fp64 symmetric solves, and a design whose
 * smallest eigenvalue is below f 2^-23 of its largest is refused (PEGSX's float rank rule) where the reference returns Inf.
 * BWGR_EINVAL, the device and the panel stay usable: a null required pointer, a bad zloc / oloc, f < 1 or f > 256, k < 1 or k > 16, maxit < 0,
 * an fp32 panel, rows of Z other than n, ldz / ldx / ldo < n, p < 1 or p > 2147483392, a non-finite entry of X or of a host Z (a device Z is
 * the caller's duty), a trait with n_t <= f records, a rank-deficient design (the message names the trait, or "all rows"), a workspace beyond
 * the device's free memory. */
int bwgr_project(int device, bwgr_panel *P, const double *Z, int zloc, int64_t n, int64_t p, int64_t ldz, const double *X, int64_t f, int64_t ldx,
                 double *out, int oloc, int64_t ldo);
int bwgr_mlm(int device, bwgr_panel *P, const double *Z, int zloc, int64_t n, int64_t p, int64_t ldz, const double *X, int64_t f, int64_t ldx,
             const double *Y, int k, int maxit, double logtol, double df0, int verb, double *b, double *u, double *hat, double *h2, double *GC,
             double *vb, double *ve, double *cnv, int *its);
/* host arithmetic of bwgr_mlm's plan (needs no GPU) for n rows, p columns of Z, f covariates, k traits and npat missingness patterns (n >= 2,
 * 1 <= p <= 2147483392, 1 <= f <= 256, 1 <= npat <= k <= 16, else BWGR_EINVAL): out[0..14] bwgr_debug_mrr_dense_plan's fields for the train on
 * Zp (ld, nblk, edge, tiles, pass_wg, trips, cols_wg, hat_wg, linv_lds, ngl, lds_gram, lds_pass, lds_solve, lds_linv and the train's own
 * workspace); out[15] and out[16] the grid of k_project (64-column blocks; row-tile workgroups per block); out[17] the row tiles one of them
 * takes at most; out[18] the f-pieces and out[19] the covariates of a piece; out[20] the LDS bytes of k_project (dynamic, at most 65536);
 * out[21] the trait groups of Z'X; out[22] the bytes the projection adds (X, its staged copy, Z'X and C); out[23] the whole device workspace
 * of a call on a panel or a device Z, the n p 8-byte copy of Zp included (a host Z is uploaded into that copy and projected in place). */
#define BWGR_MLM_PLAN_NOUT 24
/* probe hook: mode = 1 makes the projection's steps wait for the stream and keep their wall-clock milliseconds; out (or null) receives those of
 * the process's last bwgr_project or bwgr_mlm: out[0] X'X and its eigen-decomposition on the host, out[1] X onto the device, its staging and
 * Z'X, out[2] Z'X back, C on the host and C onto the device, out[3] k_project.  mode = 0 (the default) times nothing.  Else BWGR_EINVAL. */
#define BWGR_PROJECT_TIMING_NOUT 4
int bwgr_debug_project_timing(int mode, double out[BWGR_PROJECT_TIMING_NOUT]);
int bwgr_debug_mlm_plan(int64_t n, int64_t p, int64_t f, int k, int npat, int64_t out[BWGR_MLM_PLAN_NOUT]);
/* ---- per-trait ridge fits (UVBETA / FUVBETA family) -------------------------------------------------------
 * Replaces VectorXd solver1x(Y,X,maxit,tol,df0) src/RcppEigen20230423.cpp:1410-1443 and MatrixXd UVBETA(Y,X) :1506-1515; solver1xF :1613-1646 and
 * FUVBETA :1709-1718; xsolver1xF :1721-1743 and XFUVBETA :1746-1753; zsolver1xF :1771-1804 and ZFUVBETA :1807-1816 (R/RcppExports.R:196-238).
 * One randomized Gauss-Seidel ridge fit per column of Y, all on the panel's X: each trait is fitted on its own observed rows (NaN = missing;
 * the reference subsets X and Y per trait, :1495-1503), with its own column means over those rows, its own lambda and its own stopping sweep.
 * The marker order of sweep s is the EM family's (bwgr_em_order), so all traits share one gathered panel per sweep.  Y: n x k column-major
 * doubles; k >= 1 has no upper limit (the engine takes the traits 64 at a time).  variant: BWGR_UVB_D solver1x / UVBETA; BWGR_UVB_F solver1xF /
 * FUVBETA (the test XX_j > 1e-5, else b_j = 0, :1633-1635); BWGR_UVB_X xsolver1xF / XFUVBETA (lambda = mean XX_j, fixed; no variances: ve, vb
 * and h2 return NaN); BWGR_UVB_Z zsolver1xF / ZFUVBETA (its own variance updates, h2 = 1 - ve / vy).  The float variants run the fp64 engine;
 * the caller rounds Y (and tol, df0) to float, as for bwgr_mrr.  maxit, tol, df0: the solvers' arguments (reference defaults 100, 10e-7, 20;
 * xsolver1xF and zsolver1xF have them built in).  A trait stops when its own log10 sum (delta b)^2 < log10(tol), at maxit, or on NaN; a
 * stopped trait's state is not touched again.  tol = 0 never stops early; maxit = 0 returns b = 0.
 * Outputs (host; only b and its are required): b[p x k] column-major, mu[k], h2[k] (1 - ve / vy), ve[k], vb[k], its[k] (sweeps each trait
 * ran), cnv[k] (each trait's last convergence value), xb[n x k] = X b on the raw genotypes for every row, the unobserved ones included (what
 * GSEM / XSEMF / ZSEMF form next, :1586, :1758, :1822; bwgr_panel_xb forms it for any B).  A trait with no observed row gives a zero column of b, its = 0, mu = h2 = 0 and NaN
 * elsewhere, for every variant (XFUVBETA has no such test and would return NaN there).  A panel switched to implicit centring gives
 * bit-identical results (the fit reads the raw genotypes and centres per trait).
 * BWGR_EINVAL: an fp32 panel, an unknown variant, maxit < 0, k < 1, a trait with exactly one observed row (the reference divides by n - 1;
 * the message names the trait).  (The int32 pattern Grams are within bwgr_panel_create's bound n * max|x|^2 < 2^31.)
 * Degenerate traits are not refused and follow the reference's arithmetic: a trait that is constant on its observed rows has vy = 0, hence
 * ve = vb = 0 and lambda = 0 / 0, and its column comes back NaN with its = 1 (the NaN convergence value stops it, as in the reference); a trait
 * whose markers are all monomorphic on its rows has TrXSX = 0, hence vb = inf and lambda = 0: every marker takes the XX_j = 0 path and b stays
 * 0 (the reference's D and Z give 0 / 0 = NaN there).  For BWGR_UVB_X with TrXSX = 0 the library likewise returns b = 0 where the reference
 * returns NaN.  Neither affects the other traits of the call.
 * Not here: MEGA, GSEM and solver2x -- two designs inside one sweep, each with its own lambda, are bwgr_uvbeta2 (below), which runs this
 * entry's engine with a dense leg in front of it; fp32 panels; groups of traits sharded over GPUs.  XSEMF, ZSEMF and YSEMF are compositions
 * of this entry, bwgr_uvbeta_dense and bwgr_panel_xb (below) made by the host layers. */
enum { BWGR_UVB_D = 0 /* solver1x  / UVBETA   */, BWGR_UVB_F = 1 /* solver1xF / FUVBETA  */,
       BWGR_UVB_X = 2 /* xsolver1xF/ XFUVBETA */, BWGR_UVB_Z = 3 /* zsolver1xF/ ZFUVBETA */ };
int bwgr_uvbeta(bwgr_panel *P, const double *Y, int64_t k, int variant, int maxit, double tol, double df0,
                double *b /* p x k, column-major */, double *mu, double *h2, double *ve, double *vb,
                int *its /* k: sweeps each trait ran */, double *cnv /* k: each trait's last value */,
                double *xb /* n x k = X b on the raw genotypes, every row; may be NULL */);
/* host arithmetic of bwgr_uvbeta's plan (needs no GPU), in the style of bwgr_debug_mrr_plan, for n rows, p markers and k traits (each at
 * least 1, else BWGR_EINVAL): out[0..7] = W (traits per group), groups = ceil(k / W), traits per solve workgroup, Gram matrices a solve
 * workgroup stages in LDS (the patterns of its other traits are read from global memory), the solve's dynamic LDS bytes, the pass's, the
 * pass's workgroups, and an upper bound of the call's device workspace in bytes (rows padded to 128, every trait its own pattern, xb
 * requested). */
#define BWGR_UVB_PLAN_NOUT 8
int bwgr_debug_uvb_plan(int64_t n, int64_t p, int64_t k, int64_t out[BWGR_UVB_PLAN_NOUT]);
/* ---- the same fits on a small dense design, and X B on the panel: what XSEMF / ZSEMF / YSEMF are made of ---------------
 * SEXP XSEMF(Y,X,npc) src/RcppEigen20230423.cpp:1756-1769, ZSEMF :1819-1845, YSEMF :1848-1874 (R/RcppExports.R:232, 240, 244) fit every trait on the
 * panel (XFUVBETA / ZFUVBETA), form G = X BETA, take its thin SVD, fit every trait again on the latent design Z = (U diag(s)).leftCols(npc) and
 * map the coefficients back.  The SVD of the n x k matrix stays with the caller (the host layers: bwgr_amd.XSEMF ..., rshim/bwgr_hip.R).
 * bwgr_uvbeta_dense: bwgr_uvbeta's fits, all four variants and every rule of the comment above (own observed rows, own column means over them,
 * tilde on the raw columns, per-trait stopping with stopped traits left alone, tol = 0, maxit = 0, all-NaN traits, F's test XX_j > 1e-5 and
 * b_j = 0 where XX_j == 0 otherwise, the marker orders of bwgr_em_order(q, s)), on a dense design Z of n x q doubles, column-major with leading
 * dimension ldz, q small (npc <= k there; any q >= 1 is taken).  One workgroup per trait runs the trait's whole fit in one launch.  Y: n x k
 * column-major, NaN = missing.  Outputs as bwgr_uvbeta's (b is q x k; only b and its are required).  BWGR_EINVAL: a null pointer, n < 1,
 * q < 1, ldz < n, k < 1, an unknown variant, maxit < 0, a trait with exactly one observed row, an entry of Z that is not finite. */
int bwgr_uvbeta_dense(int device, const double *Z, int64_t n, int64_t q, int64_t ldz, const double *Y, int64_t k, int variant, int maxit,
                      double tol, double df0, double *b /* q x k */, double *mu, double *h2, double *ve, double *vb, int *its, double *cnv);
/* host arithmetic of bwgr_uvbeta_dense's plan (needs no GPU; n, q, k at least 1, else BWGR_EINVAL): out[0..4] = lds_rows (the largest n whose
 * residual stays in the workgroup's LDS), e_in_lds (1: n <= lds_rows; 0: the residuals live in a global workspace of n x k doubles), threads
 * per workgroup, dynamic LDS bytes, bytes of that workspace (0 when e is in LDS). */
#define BWGR_UVBD_PLAN_NOUT 5
int bwgr_debug_uvbd_plan(int64_t n, int64_t q, int64_t k, int64_t out[BWGR_UVBD_PLAN_NOUT]);
/* ---- two designs in one sweep: solver2x for every column of Y, the solver of MEGA and GSEM -----------------------------
 * Replaces VectorXd solver2x(Y,X1,X2,maxit,tol,df0) src/RcppEigen20230423.cpp:1446-1493 as SEXP MEGA(Y,X,npc) :1542-1579 and SEXP GSEM(Y,X,npc)
 * :1582-1610 call it (R/RcppExports.R:200, 208, 212): X1 = Z, a dense design of n x q doubles (the latent spaces; column-major, leading
 * dimension ldz), X2 = the panel.  One fit per column of Y (n x k, NaN = missing) on the trait's own observed rows, everything fp64.  Set-up
 * (:1449-1462): mu, y, tilde_1 = Z'y and tilde_2 = X'y on the raw columns; each design centred by the trait's own column means over its rows;
 * XX_i, TrXSX_i, MSx_i = TrXSX_i / (n_t - 1), vy, ve = vy / 2, vb_i = ve / MSx_i, lambda_i = ve / vb_i, vb0_i = vb_i df0, ve0 = ve df0.  Sweep s
 * (:1466-1487): the q columns of Z in the order bwgr_em_order(q, s), then the p markers in the order bwgr_em_order(p, s), against one
 * residual: b1 = (x_c'e + XX b0) / (XX + lambda_i), e -= x_c (b1 - b0) on the observed rows; then mu0 = mean(e), mu += mu0, e -= mu0,
 * ve = (e'e + e'y + ve0) / (2 n_t - 1 + df0), vb_i = (tilde_i'b_i + b_i'b_i + vb0_i) / (TrXSX_i + p_i + df0), lambda_i = ve / vb_i,
 * cnv = log10(sum (delta b_1)^2 + sum (delta b_2)^2).  A trait stops on cnv < log10(tol), at maxit, or on NaN, each trait by itself; a stopped
 * trait's state is not touched again by either leg.  The panel leg is bwgr_uvbeta's engine unchanged (variant D); the dense leg in front of
 * it runs one workgroup per running trait, with the trait's residual in LDS when n fits -- by bwgr_uvbeta_dense's plan exactly
 * (bwgr_debug_uvbd_plan: lds_rows, threads, LDS bytes), so there is no plan hook of its own.
 * Departures from the reference: (1) where XX_iJ is exactly 0 the coefficient is exactly 0 (threshold 0, both designs); (2) a design whose
 * TrXSX_i is 0 for a trait (every column constant on that trait's rows) is skipped for that trait: its coefficients stay 0, its lambda is
 * never formed and its vb_i returns NaN, and the other design runs as if alone (the reference divides by zero and returns NaN); (3) a trait
 * with no observed row returns zero columns, its = 0, mu = h2 = 0 and NaN elsewhere; (4) h2 is reported as 1 - ve / vy (the reference
 * computes none).
 * Outputs (host; b1, b2 and its are required): b1[q x k], b2[p x k] column-major, mu, h2, ve, vb1, vb2, cnv [k], its[k].  A panel switched to
 * implicit centring gives bit-identical results.  BWGR_EINVAL: a null required pointer, q < 1 or q > 2147483392 (the column ids are int32; the per-column
 * values live in global memory, so there is no other limit on q), ldz < n, k < 1, maxit < 0, an entry of Z that
 * is not finite, an fp32 panel, a trait with exactly one observed row.
 * Not here: solver2xF (:1649-1706) -- its shuffles run from RGSvec1.begin() to RGSvec2.end() (:1671-1672), iterators of two different
 * vectors, so its order is undefined and cannot be restated; no driver of the reference calls it.  A dense X2; fp32 panels; R's SEM(), which
 * needs MRR3F options this library refuses.  MEGA and GSEM themselves are compositions made by the host layers (bwgr_amd.MEGA, GSEM;
 * rshim/bwgr_hip.R): the thin SVD of an n x k matrix stays with the caller. */
int bwgr_uvbeta2(bwgr_panel *P, const double *Z, int64_t q, int64_t ldz, const double *Y, int64_t k, int maxit, double tol, double df0,
                 double *b1 /* q x k */, double *b2 /* p x k */, double *mu, double *h2, double *ve, double *vb1, double *vb2, int *its,
                 double *cnv);
/* ---- PEGS / PEGSZ: multi-trait fits over several designs --------------------------------------------------
 * Replaces SEXP PEGS(Y,X,maxit,logtol,covbend,covMinEv,XFA,NNC) src/RcppEigenX20251203.cpp:10-194 and PEGSZ(Y,X_list,...) :576-808: the
 * pseudo-expectation Gauss-Seidel solver for k correlated traits (1 <= k <= BWGR_MRR_MAXK), one residual variance per trait and one k x k
 * genetic covariance per random effect.  In every sweep the neff effects are walked in list order against one n x k residual.  An effect is
 *   a panel effect  (panel != NULL): the resident int8 genotypes, NOT centred (PEGS never centres X) -- bwgr_mrr's launch train in its
 *                   uncentred mode; or
 *   a dense effect  (panel == NULL): Z, n x q fp64 column-major with column stride ldz >= n, host -- one workgroup walks its q columns.
 * All effects have n rows; all panels live on one device and share the row padding ld (panels made with the same block / nwg arguments do);
 * `device` is used only where no effect is a panel.  Y: n x k column-major, NaN = missing; the caller rounds Y to float where it mirrors the
 * reference's float inputs -- the engine is fp64 throughout, and the reference's float constants (1e-12f, 10e-4) are taken as doubles.
 * After every sweep (host, double): ve_t = e_t'y_t / (n_t - 1); per effect vb from TildeHat = b'tilde and TrXSX with no prior, the XFA
 * structure (XFA < 0: k; 0: independent traits; else the leading XFA eigen-terms of the correlation matrix), NNC clamps at 0, MinDVb = the
 * smallest eigenvalue, inflate carried as a running maximum of |MinDVb covbend| over the sweeps with MinDVb < covMinEv and added to the
 * diagonal when k >= 5 or MinDVb < covMinEv, iG = pinv(vb); the intercept step with 1 / (n_t - 1) as the reference writes it; cnv = log10 of
 * sum over effects and traits of (delta b)^2, and the fit stops once cnv < logtol (logtol = -inf: every sweep runs).
 * own_text = 1 follows PEGS's own text where it differs from PEGSZ's: the XFA branch is taken whenever XFA > 0 (:139; PEGSZ: 0 < XFA < k,
 * :734) and a zero TrXSX is not guarded (:130; PEGSZ :722-724).  On ordinary data the two agree to rounding.
 * Departure: the reference seeds std::mt19937 from std::random_device, so its marker order cannot be reproduced and any permutation is
 * faithful; here sweep s (0-based) walks an effect of m columns in bwgr_em_order(m, s), the cumulative std::shuffle(order, std::mt19937(s)).
 * Outputs (host; b and numit are required): mu, h2 [k]; b[e]: p_e x k column-major; hat: n x k column-major, a row for every individual;
 * GC[e]: k x k (the max(sd, 1e-12) floor of :180-183); bend [neff]: every effect's inflate; cnv [max(maxit, 1)]: the value after every sweep
 * run (10 where none ran).  BWGR_EINVAL, the panels stay usable: a null required pointer, neff < 1, k outside 1..16, XFA > k (the
 * reference would index out of range), maxit < 0, covbend / covMinEv not finite or logtol NaN / +inf, a trait with fewer than 2 records,
 * an fp32 panel, effects with different n or ld, panels on different devices, q < 1 or q > 2147483392, ldz < n, a non-finite entry of Z, an
 * effect whose TrXSX is 0 for a trait (the start value ve / MSx is infinite there).
 * Not here: k > 16 (PEGSX is bwgr_pegsx below; sparse effects, PEGS_sparse and PEGSZ_sparse are bwgr_pegs_ex below). */
typedef struct bwgr_pegs_effect { bwgr_panel *panel; const double *Z; int64_t q, ldz; } bwgr_pegs_effect;
int bwgr_pegs(int device, const bwgr_pegs_effect *eff, int neff, const double *Y, int64_t n, int k, int maxit, double logtol, double covbend,
              double covMinEv, int XFA, int NNC, int own_text, double *mu, double *const *b, double *hat, double *h2, double *const *GC,
              double *bend, int *numit, double *cnv);
/* ---- sparse effects; PEGS_sparse / PEGSZ_sparse -------------------------------------------------------------
 * bwgr_pegs_ex is bwgr_pegs with a wider effect struct and `text` in place of own_text; bwgr_pegsx_ex (below) is bwgr_pegsx with the wider
 * effects.  bwgr_pegs and bwgr_pegsx forward to them (text = own_text != 0).  An effect is, in this order,
 *   a panel effect   (panel != NULL), as above;
 *   a sparse effect  (colptr != NULL): n x q column-compressed (CSC), host: colptr int64[q + 1], rowidx int32[nnz], val double[nnz], nnz =
 *                    colptr[q] -- the incidence matrix of environments, locations, blocks or genotype-by-environment cells.  On the device
 *                    it takes nnz + q k^2 values, never n q.  Where no row occurs in two columns (the columns of one factor; tested on the
 *                    host, O(nnz)) Gauss-Seidel over its columns does not depend on their order, and a grid of waves updates all columns at
 *                    once (k_pegs_sparse_leg_disjoint); any other sparse effect, or one with bit 0 of `flags` set (BWGR_PEGS_SERIAL, for
 *                    tests and the probe), is walked by one wave in the sweep's order (k_pegs_sparse_leg).  Both legs run one per-column
 *                    routine, so on a row-disjoint effect they give the same bits.  Empty columns (b stays 0) and stored zeros are allowed;
 *   a dense effect   (else), Z as above.
 * Any mix of kinds is allowed in one list, e.g. [panel, sparse, sparse, dense].
 * text: 0 PEGSZ's text; 1 PEGS's own text (own_text above) -- PEGS_sparse (:811-1007) is text 1 on one sparse effect; 2 PEGSZ_sparse's text
 * (:1010-1250).  What the sparse functions' texts change against PEGS / PEGSZ, line by line:
 *   - PEGSZ_sparse's intercept step divides the residual sums by n_t (iN_mu, :1202), PEGSZ's by n_t - 1 (iN_var, :760).  This is all text 2
 *     changes here.  PEGS_sparse keeps PEGS's 1 / (n_t - 1) (:865, :977).
 *   - PEGSZ_sparse takes vy and ve with 1 / (max(n_t, 1) - 1) (:1076), PEGSZ with 1 / (n_t - 1) (:639): they differ only for n_t < 1, and a
 *     trait with fewer than 2 records is refused here under every text.
 *   - the designs arrive as double sparse matrices and are cast to float once (:821, :1028): the caller rounds val, as it rounds Y.
 *   - XX, XSX, tilde, the dots and the residual update run over the stored entries (:846-860, :875, :924, :933-936, and the same in
 *     :1057-1092, :1138-1148): the same numbers as on the dense copy, summed over fewer terms.
 *   - PEGS_sparse keeps PEGS's XFA branch for every XFA > 0 and its unguarded division by TrXSX (:955, :947); PEGSZ_sparse keeps PEGSZ's
 *     0 < XFA < k and its guards (:1176, :1164-1166).  The bending, the stop rule, h2, GC and the outputs are the same text.
 * BWGR_EINVAL, the panels stay usable: what bwgr_pegs refuses; text outside 0..2; a sparse effect with Z set as well, with a null rowidx
 * or val, q < 1 or q > 2147483392, colptr[0] != 0, a decreasing colptr, colptr[q] > 2^31 - 1, a row index outside [0, n) or not strictly
 * increasing within its column (unsorted or duplicated), a non-finite value -- the message names the effect, the column and the entry. */
#define BWGR_PEGS_SERIAL 1
typedef struct bwgr_pegs_effect_ex {
  bwgr_panel *panel; const double *Z; int64_t q, ldz;
  const int64_t *colptr; const int32_t *rowidx; const double *val; int64_t flags;
} bwgr_pegs_effect_ex;
int bwgr_pegs_ex(int device, const bwgr_pegs_effect_ex *eff, int neff, const double *Y, int64_t n, int k, int maxit, double logtol, double covbend,
                 double covMinEv, int XFA, int NNC, int text, double *mu, double *const *b, double *hat, double *h2, double *const *GC,
                 double *bend, int *numit, double *cnv);
/* host arithmetic of the sparse legs (needs no GPU) for a sparse effect of n rows, q columns, nnz stored entries of which at most
 * max_col_nnz in one column, k traits, row-disjoint or not (n, q >= 1, 0 <= max_col_nnz <= nnz <= 2^31 - 1, 1 <= k <= 16, else BWGR_EINVAL):
 * out[0..1] the threads per workgroup and the workgroups of k_pegs_sparse_setup (one column per wave, at most 8192 workgroups); out[2..3] the
 * same of the serial leg (one wave); out[4..5] the same of the disjoint leg (one column per wave, at most 1024 workgroups); out[6] the columns
 * one trip of the disjoint grid covers; out[7] the leg a sweep takes (0 serial, 1 disjoint: exactly when `disjoint` is not 0); out[8] the
 * bytes of the effect's device workspace: both copies of the matrix, XX, XSX, tilde, b, (delta b)^2, the q k x k inverses, the order, the sums --
 * proportional to nnz + q k^2 (and n + q for the pointers), never to n q. */
#define BWGR_PEGS_SPARSE_PLAN_NOUT 9
int bwgr_debug_pegs_sparse_plan(int64_t n, int64_t q, int64_t nnz, int64_t max_col_nnz, int k, int disjoint, int64_t out[BWGR_PEGS_SPARSE_PLAN_NOUT]);
/* host arithmetic of bwgr_pegs's dense leg (needs no GPU), in the style of the other plan hooks, for a dense effect of n rows and q columns
 * and k traits (n, q >= 1, 1 <= k <= 16, else BWGR_EINVAL): out[0] the threads of the one workgroup of k_pegs_dense_leg (one row per thread
 * up to 1024, whole waves), out[1] its dynamic LDS bytes, out[2] the bytes of the effect's device workspace (Z, XX, XSX, tilde, b, the q
 * k x k inverses, the order, the sums). */
#define BWGR_PEGS_PLAN_NOUT 3
int bwgr_debug_pegs_plan(int64_t n, int64_t q, int k, int64_t out[BWGR_PEGS_PLAN_NOUT]);
/* ---- PEGSX: fixed effects beside the random effects of the multi-trait fit ------------------------------------
 * Replaces SEXP PEGSX(Y,X,Z_list,maxit,logtol,covbend,covMinEv,cores,verbose,df0,NNC,InnerGS,NoInv,XFA,NumXFA) src/RcppEigenX20251203.cpp:197-573,
 * "MLM with fixed effect and multiple random effects": Y = X b + sum_r Z_r u_r + E for k traits with missing records.  The effects are
 * bwgr_pegs's (a resident int8 panel, not centred, or a dense n x q matrix; one n, one device, one ld) and every sweep walks them as bwgr_pegs
 * does.  X: n x f fp64 column-major with column stride ldx >= n, host, 1 <= f <= BWGR_PEGSX_MAXF, finite; there is no intercept and no
 * centring -- an intercept is a column of X.  With W the mask of observed records and M_t = w_t o X:
 *   set-up     b_t = (M_t'M_t)^+ M_t'Y_t, y_t = (Y_t - M_t b_t) o w_t, e = y; per effect ZZ_jt = sum w_t z_j^2, tilde = Z'y and
 *              TrZSZ_t = sum_j [ZZ_jt - (M_t'z_j)'(M_t'M_t)^+(M_t'z_j)]; iN_t = 1 / max(n_t - f, 1), ve = max(ssy iN / 2, 1e-8),
 *              vb = diag(ve_t / max(Tr_t iN_t, 1e-8)), the priors Sb = df0 vb and Se = df0 ve, iNp_t = 1 / max(n_t + df0 - f, 1)
 *   per sweep  every effect's columns in the sweep's order (the k x k block solve); the fixed step d = (M_t'M_t)^+ M_t'e_t, b_t += d,
 *              e_t = (e_t - M_t d) o w_t on the device; per effect vb_ii = (TildeHat_ii + Sb_ii) / (max(Tr_i, 1e-8) + df0), vb_ij =
 *              (TH_ij + TH_ji) / max(Tr_i + Tr_j, 1e-8), NNC clamps at 0, then with XFA and NumXFA > 0 the correlation matrix is rebuilt
 *              from its top min(NumXFA, k) eigenpairs with a unit diagonal, then bending as in PEGSZ (inflate carried as a running maximum,
 *              added when k >= 5 or the smallest eigenvalue is below covMinEv), iG = pinv(vb); ve = max((e'y + Se) iNp, 1e-8);
 *              cnv = log10(max(max over the effects of sum (delta u)^2, 1e-20)); the fit stops once numit >= 5 and cnv < logtol, or cnv is NaN
 * Departures: the marker order of sweep s is bwgr_em_order(m, s) per effect (the reference seeds its generator from the machine).  Both
 * pseudo-inverses of M'M (the reference: a float COD for b, a float LLT with a COD fall-back for the trace) are one symmetric
 * pseudo-inverse per missingness pattern that drops eigenvalues with |lambda| <= f 2^-23 max |lambda|, the reference's float rank
 * decision; on a full-rank X it is the inverse.  The caller rounds Y, X, dense Z and the real options to float where it mirrors the
 * reference's float inputs; the engine is fp64 and the reference's float floors are taken as doubles.
 * Refused options: InnerGS != 0 and NoInv != 0 (the block solve has neither, as in bwgr_mrr).  cores and verbose have no counterpart.
 * Outputs (host; u and numit are required, the others may be null): TrZSZ [neff x k, effect e at e * k]; b: f x k column-major; u[e]: p_e x k
 * column-major; vb[e], GC[e]: k x k (GC with the max(sd, 1e-12) floor); ve [k]; hat: n x k column-major, X b + sum Z_r u_r for every row;
 * cnv [max(maxit, 1)]: the value after every sweep run (10 where none ran); bend [neff].
 * BWGR_EINVAL, the panels stay usable: what bwgr_pegs refuses of its effects and of maxit / logtol / covbend / covMinEv, df0 not finite or
 * negative, f < 1 or f > BWGR_PEGSX_MAXF, ldx < n, a non-finite entry of X, a trait with fewer than 2 records, InnerGS, NoInv.
 * MLM, which reaches the same model by projecting Z off X, is bwgr_mlm (above, on the dense block train).
 * bwgr_pegsx_ex is bwgr_pegsx with bwgr_pegs_ex's wider effects: a sparse effect is swept as there, and its share of TrZSZ is taken over the
 * column's stored entries (k_pegsx_trace_sparse).  bwgr_pegsx forwards to it. */
#define BWGR_PEGSX_MAXF 256
int bwgr_pegsx(int device, const bwgr_pegs_effect *eff, int neff, const double *X, int64_t ldx, int f, const double *Y, int64_t n, int k, int maxit,
               double logtol, double covbend, double covMinEv, double df0, int NNC, int XFA, int NumXFA, int InnerGS, int NoInv, double *TrZSZ,
               double *b, double *const *u, double *const *vb, double *const *GC, double *ve, double *hat, int *numit, double *cnv, double *bend);
int bwgr_pegsx_ex(int device, const bwgr_pegs_effect_ex *eff, int neff, const double *X, int64_t ldx, int f, const double *Y, int64_t n, int k, int maxit,
                  double logtol, double covbend, double covMinEv, double df0, int NNC, int XFA, int NumXFA, int InnerGS, int NoInv, double *TrZSZ,
                  double *b, double *const *u, double *const *vb, double *const *GC, double *ve, double *hat, int *numit, double *cnv, double *bend);
/* host arithmetic of bwgr_pegsx (needs no GPU) for n rows, f columns of X and k traits (n >= 1, 1 <= f <= BWGR_PEGSX_MAXF, 1 <= k <= 16, else
 * BWGR_EINVAL): out[0] the threads of each of the k workgroups of the fixed step (one row per thread up to 1024, whole waves), out[1] its
 * dynamic LDS bytes (two f-vectors), out[2] the bytes of X, the pseudo-inverses of up to k patterns and b on the device; the trace kernels'
 * tiling: out[3] the columns of an effect a wave carries at once, out[4] the columns of X per register tile, out[5] their dynamic LDS bytes
 * (four waves' v plus the per-wave totals). */
#define BWGR_PEGSX_PLAN_NOUT 6
int bwgr_debug_pegsx_plan(int64_t n, int f, int k, int64_t out[BWGR_PEGSX_PLAN_NOUT]);
/* host arithmetic of the launch shapes of bwgr_pegs and bwgr_pegsx (needs no GPU), in the style of bwgr_debug_launch_plan, for n rows and an
 * effect of m columns (each at least 1, else BWGR_EINVAL).  out[0..1], k_pegsx_trace_panel / k_pegsx_trace_dense: their workgroups (= partials
 * per pattern, at most 1024; four waves each, a wave four columns at once) and the columns one trip of that grid covers.  out[2..3],
 * k_pegs_dense_setup: its workgroups (at most 8192, one column per wave) and the columns per trip.  out[4]: the threads of the one workgroup
 * of k_pegs_dense_leg; out[5]: the threads of each workgroup of k_pegsx_fixed (both one row per thread up to 1024, whole waves). */
#define BWGR_PEGS_LAUNCH_PLAN_NOUT 6
int bwgr_debug_pegs_launch_plan(int64_t n, int64_t m, int64_t out[BWGR_PEGS_LAUNCH_PLAN_NOUT]);
/* timing of bwgr_pegsx for tools/pegsx_probe.py (process-wide, not thread-safe; off by default): sets the mode of the calls that follow --
 * 0: off; 1: the set-up kernels are bracketed with events (outside the sweeps) and every sweep is timed with the host clock, which adds no
 * synchronisation to a sweep; 2: k_pegsx_fixed is bracketed with events as well -- and copies out what the last timed call left, in ms:
 * out[0] the trace kernels, out[1] the effects' own set-up kernels (k_mrr_setup_cols / k_pegs_dense_setup), out[2] the sweeps timed,
 * out[3..5] mean / min / max of a sweep, out[6..8] mean / min / max of the fixed step alone (mode 2).  out may be null. */
#define BWGR_PEGSX_TIMING_NOUT 9
int bwgr_debug_pegsx_timing(int mode, double out[BWGR_PEGSX_TIMING_NOUT]);
/* out (n x k, host, column-major) = X B on the raw int8 genotypes for every row; B: p x k, host, column-major.  fp64 sums; the markers are
 * split over workgroups and the partial sums added in a fixed order, so two calls give the same bits, and so does a panel switched to implicit
 * centring.  BWGR_EINVAL: a null pointer, k < 1, an fp32 panel.  (bwgr_uvbeta's own xb output is a different summation order.) */
int bwgr_panel_xb(bwgr_panel *P, const double *B, int64_t k, double *out /* n x k */);
/* host arithmetic of a panel's plan (needs no GPU): what bwgr_panel_create would decide for an int8 (is_f32 = 0) or float panel of n x p
 * with these block / nwg arguments under the BWGR_* switches of the environment; kind 0: a main panel, 1: the row-subset scratch panel of
 * KMUP2 and wgr's bagging, 2: bwgr_em's scratch panel.  A shape bwgr_panel_create refuses returns its code and leaves its message in
 * bwgr_last_error.  out[0..17]: m, K, R, ld, nblocks, pstride, nfeed, lag-4 streamer fits, LDS bytes of k_sweep / k_sweep2 / k_sweep2w,
 * x_bytes, bytes per Gram array, pipelined engine (0: the first-generation k_sweep), farthest distance of the cross Gram arrays, 16-bit
 * copies carried, farthest distance the affine engine's byte planes may reach, k_sweep3 attempted.  out[18..24], k_sweep3's share for an
 * assumed largest |x| (xmax >= 0; xmax < 0: left at their defaults) and 16-bit verdict gram16: fits, R3, streamers per slab, K3, D, LDS
 * bytes, solo streamer height allowed. */
#define BWGR_PANEL_PLAN_NOUT 25
int bwgr_debug_panel_plan(int is_f32, int64_t n, int64_t p, int block, int nwg, int kind, int xmax, int gram16, int64_t out[BWGR_PANEL_PLAN_NOUT]);
/* host arithmetic of a sweep's plan (needs no GPU): what the library would decide for a sweep over a panel planned as bwgr_debug_panel_plan
 * plans it (its first eight arguments; xmax < 0: no k_sweep3), taken to be one whose far Gram blocks fit -- k_sweep3 is there exactly when its
 * plan fits, the distance-1 / 2 records exactly when gram16 holds as well, the affine engine's byte planes reach as far as the panel plan
 * allows.  flags: the sweep's SWF_* flags (csrc/sweep.hip.h); blocks [blk_begin, blk_end), blk_end <= 0: the whole panel; mode 0: a sweep
 * alone, 1: the fp64 redo of one, 2: a pair's (bwgr_chain_run_pair); state: bit 0 clones are alive, bit 1 the handle is a clone, bit 2 the
 * panel is a shard among three or more on its device, bit 3 bwgr_debug_withhold is on.  BWGR_EINVAL for what the library never plans: a shape
 * bwgr_panel_create refuses, a bad block range, clones or shards of a scratch panel, implicitly centred columns (SWF_CENTRE) but for a
 * selection sweep on a panel with k_sweep3, the redo of a sweep that has none, a pair but of whole selection sweeps, columns as stored, on a
 * panel with k_sweep3.  out[0..24]: engine (1 k_sweep, 2 k_sweep2, 3 k_sweep3, 4 k_sweep2w), the gate (0 none, 1 finite, 2 every sweep is
 * k_sweep3's) and its float bits, then for the engine behind the gate lag, feeders, 16-bit staging; k_sweep3's R3, K3, streamers per slab, the
 * two prefetch workgroups (-1: none), dbg3, qsplit, skip_vb, k_sweep3f; k_sweep2w's fx, nd, npf, ahead, nq, sub, K3; guarded, draws ahead,
 * spin launches.  out[25..39]: the spin launches in launch order, five each: kernel (the instantiation's number in tests/sweep_plan_cases.py:
 * KERNELS; -1 and zeros: none), grid, resident workgroups, threads, LDS bytes.  out[40..50]: the redo of a guarded sweep (zeros: none):
 * engine, lag, feeders, 16-bit staging, fx, nd, npf, ahead, nq, sub, K3.  out[51..66], the helper kernels: spin launch of the engine behind
 * the gate and of the redo (-1: none); k_escale_reset; k_escale on the gate and k_spec3; k_cen_tot / k_cen_scan / k_cen_begin / k_cen_end
 * mode 0; k_escale at infinity; k_affine_inv; k_cen_tot / k_cen_scan mode 1; k_spec (1 int32, 2 fp64) and its sel argument; the mode of
 * k_cen_begin / k_cen_end around the engine behind the gate and around the redo (-1: none); k_spec and k_cen_tot / k_cen_scan mode 2 in front
 * of the redo; k_vb_fill; SWF_DEBUG_WITHHOLD.  (The snapshot trio goes with guarded.) */
#define BWGR_SWEEP_PLAN_NOUT 67
int bwgr_debug_sweep_plan(int is_f32, int64_t n, int64_t p, int block, int nwg, int kind, int xmax, int gram16, int flags, int blk_begin, int blk_end,
                          int mode, int state, int64_t out[BWGR_SWEEP_PLAN_NOUT]);
/* host arithmetic of the two launch rules around the sweep (needs no GPU), in the style of bwgr_debug_panel_plan, for an int8 (is_f32 = 0) or
 * float panel of p markers and ld padded rows (a positive multiple of 128, else BWGR_EINVAL).  out[0..2], the two-stage product X * coef behind
 * every hat and wgr's residual: column chunks, columns per chunk (the last chunk takes what is left), row workgroups.  out[3..4], the row
 * gather of KMUP2 and wgr's bagging: its path (0: element-wise; else the columns an int8 workgroup stages in LDS) and that workgroup's LDS
 * bytes. */
#define BWGR_AUX_PLAN_NOUT 5
int bwgr_debug_aux_plan(int is_f32, int64_t p, int64_t ld, int64_t out[BWGR_AUX_PLAN_NOUT]);

/* ---- relationship kernels on the resident panel --------------------------------------------------------------
 * Replaces the functions with which bWGR's users make the K of wgr(eigK = eigen(K)): SEXP GAU(X) src/Rcpp20260726ai.cpp:1338-1360,
 * GRM(X, Code012) :1363-1383 (R/RcppExports.R:100-106), EigenARC(X, centralizeX, cores) src/RcppEigen20230423.cpp:8-26, EigenGAU(X, phi,
 * cores) :29-38, EigenGRM(X, centralizeZ, cores) :41-51 (R/RcppExports.R:140-150).  All five are one X X' over the panel's n rows -- exact in
 * integers on the int8 matrix cores, int32 sums over chunks of at most floor((2^31 - 1) / max|x|^2) markers added in int64 -- and an
 * element-wise finish in fp64 from the exact integers (the reference computes in float; the library returns the fp64 value of the
 * reference's formulas, its literals 3.1416 and 1.001 and the `m_j^2 / 2` of GRM's Code012 included).  int8 panels only, root or clone, any
 * geometry; a panel switched to implicit centring gives the same results as before the switch (all five are defined on the raw genotypes).
 * Both entry points run on the panel's stream, return when the result is complete, and return BWGR_EINVAL without enqueuing anything while
 * sweeps of other handles are in flight on the device (occupancy guard, above).  Also BWGR_EINVAL: fp32 panels, an unknown kind, a leading
 * dimension below n, max|x|^2 * p >= 2^53 or max|x|^2 * n * p >= 2^63.  BWGR_KCHUNK (read when the root panel is made) forces a shorter chunk.
 * Not here: fp32 panels, EigenEVD / mkr2X (the eigendecomposition stays with the caller; K2X and mkr decompose in the host layers and fit by bwgr_mrr_dense), CNT / IMP / SPC / SPM, and a product
 * sharded over GPUs. */
enum { BWGR_K_GRM = 0, BWGR_K_GAU = 1, BWGR_K_EIGEN_GRM = 2, BWGR_K_EIGEN_GAU = 3, BWGR_K_EIGEN_ARC = 4 };
/* exact X X' over the panel's n rows (the Eigen product of src/RcppEigen20230423.cpp:17, :32, :48, in integers): G is n x n int64, ldg >= n,
 * host or device per memloc */
int bwgr_panel_crossprod(bwgr_panel *P, int64_t *G, int64_t ldg, int memloc);
/* K (n x n doubles, column-major = row-major: exactly symmetric, ldk >= n, host or device per memloc; entries beyond column n of a row are
 * not touched).  par: phi for EIGEN_GAU (reference default 1.0), ignored otherwise.  flag: Code012 for GRM (default 0); centralizeZ /
 * centralizeX for EIGEN_GRM / EIGEN_ARC (default 1); ignored otherwise.  A device K serves as the call's own n x n workspace. */
int bwgr_panel_kernel(bwgr_panel *P, int kind, double par, int flag, double *K, int64_t ldk, int memloc);
/* host arithmetic of the product's plan (needs no GPU), in the style of bwgr_debug_panel_plan: for n, p, the panel's largest |x| and a
 * forced chunk (0 = the rule above; a forced chunk beyond the rule is cut to it) out[0..7] = markers per chunk, chunks, output tiles
 * computed (upper triangle of 128-row tiles), workgroups launched, workspace bytes of a kernel call with a host output, row tiles, pieces
 * a chunk is split into, markers per piece.  Refused shapes return their code with the message in bwgr_last_error. */
#define BWGR_XXT_PLAN_NOUT 8
int bwgr_debug_xxt_plan(int64_t n, int64_t p, int xmax, int64_t kchunk, int64_t out[BWGR_XXT_PLAN_NOUT]);

/* ---- founder-by-sample kernels on two resident panels -----------------------------------------------------------
 * Replaces the products and finishes inside EigenArcZ(Zfndr, Zsamp, cores) src/RcppEigen20230423.cpp:1877-1907 and EigenGauZ(Zfndr, Zsamp,
 * phi, cores) :1910-1939 (R/RcppExports.R:248-254): K_ff between the founders and K_fs between founders and samples, from which the caller
 * makes the samples' coordinates K_fs' V L^(-1/2) with the eigendecomposition K_ff = V L V' (which stays with the caller).  Pf and Ps are
 * int8 panels over the same p markers on the same device, roots or clones, of any geometry each; Pf == Ps is allowed; a panel switched to
 * implicit centring gives the same results.  The product X_f X_s' is exact in integers: int32 sums over chunks of at most
 * floor((2^31 - 1) / (max|x_f| max|x_s|)) markers added in int64, every 128 x 128 tile of the n_f x n_s result computed.  The finishes are
 * the fp64 values of the reference's float formulas from the exact integers, its literals 3.14159 and 1.001 included.  ARC: both matrices
 * centred by the FOUNDERS' column means (through the centring identity), K = N (sin t + (3.14159 - t) cos t) / 3.14159 with N = sqrt(d_a d_b
 * 1.001), t = acos(A / N), both outputs times Kscalar = 1 / mean(diag K_ff).  GAU: raw genotypes, D = the Euclidean distance, K = exp(D t),
 * t = par * (-n_f (n_f - 1)) / sum_{i != i'} D_ff; n_f (n_f - 1) is formed in double (the reference's int product overflows beyond 46 340
 * founders).  Degenerate inputs follow that arithmetic and are not refused: a row of zero centred norm gives NaN under ARC, duplicate
 * founders a singular K_ff.  Two calls give the same bits.
 * Both entry points enqueue on Pf's stream after everything pending on Ps's stream, return when the result is complete, and return
 * BWGR_EINVAL without enqueuing anything (both panels stay usable) while sweeps of other handles are in flight on the device (occupancy guard,
 * above) and for: a null pointer, a bad memloc, an fp32 panel on either side, different p, different devices, a leading dimension below its
 * row length, an unknown kind, max|x_f| max|x_s| p >= 2^53, max|x_f|^2 n_f p >= 2^63 or max|x_f| max|x_s| n_f p >= 2^63 (the int64 bounds of
 * X_f s_f and X_s s_f), a grid beyond the launch limits.  BWGR_KCHUNK forces a shorter chunk; it is read when the founders' root panel is
 * made. */
/* G (n_f x n_s int64, G[i * ldg + j] = x_f,i . x_s,j, ldg >= n_s, host or device per memloc); entries beyond column n_s of a row are not
 * touched.  bwgr_panel_crossprod2(P, P, ...) equals bwgr_panel_crossprod(P, ...) bit for bit. */
int bwgr_panel_crossprod2(bwgr_panel *Pf, bwgr_panel *Ps, int64_t *G, int64_t ldg, int memloc);
enum { BWGR_KZ_ARC = 0, BWGR_KZ_GAU = 1 };
/* Kff: n_f x n_f doubles, exactly symmetric, ldff >= n_f; Kfs: n_f x n_s doubles, row i = founder i, ldfs >= n_s; both required, host or
 * device per memloc; par: phi for GAU (reference default 1.0; ignored for ARC).  Entries beyond the last column of a row are not touched.
 * Device outputs serve as the call's own workspaces; host outputs need one n_f x n_s and one n_f x n_f 8-byte device array. */
int bwgr_panel_kernel2(bwgr_panel *Pf, bwgr_panel *Ps, int kind, double par, double *Kff, int64_t ldff, double *Kfs, int64_t ldfs, int memloc);
/* host arithmetic of the rectangular product's plan (needs no GPU), in the style of bwgr_debug_xxt_plan: for n_f, n_s, p, the two panels'
 * largest |x| and a forced chunk (0 = the rule above; a forced chunk beyond the rule is cut to it) out[0..8] = markers per chunk, chunks,
 * output tiles (T_f * T_s), workgroups launched (more than the tiles exactly when the workgroups of a tile add into it), workspace bytes of
 * a kernel2 call with host outputs, T_f, T_s, pieces a chunk is split into, markers per piece.  Refused shapes return their code with the
 * message in bwgr_last_error. */
#define BWGR_XYT_PLAN_NOUT 9
int bwgr_debug_xyt_plan(int64_t nf, int64_t ns, int64_t p, int xmaxf, int xmaxs, int64_t kchunk, int64_t out[BWGR_XYT_PLAN_NOUT]);

/* ---- synthetic panels ----------------------------------------------------------
 * X_ij ~ Binomial(2, f_j), f_j ~ U(0.05,0.5), int8 column-major written to device memory Xdev
 * (ldx >= n); freq (p floats, device, may be NULL) receives f_j.  The p columns written are columns
 * col0 .. col0+p-1 of the (conceptually unbounded) panel of this seed, so marker shards of one panel can be
 * generated independently on different GPUs. */
int bwgr_synth_genotypes(void *Xdev, int64_t n, int64_t p, int64_t ldx, int64_t col0, uint64_t seed, float *freq_dev,
                         int device, void *hip_stream);

/* ---- multi-GPU inside the library ----------------------------------------------------------------
 * (new; the reference is single-process, single-threaded R: R/wgr.R:2.)  One marker shard per device of THIS process, the
 * residual replicated, RCCL all-reduces of the residual delta (n fp64) at the exchange rounds, one host thread: what an R
 * .Call needs to use several GPUs.  G = 1 is the exact chain.  G > 1 is the partitioned sampler of DESIGN.md section 8: NOT the
 * reference's chain, and statistically SOUND ONLY ON CENTRED COLUMNS (x_j - mean(x_j); measured: 2 / 4 / 8 shards then follow the exact
 * chain's ve, mean(d) and hat; on uncentred genotypes -- what bWGR sweeps -- every shard corrects the same stale residual mean and the
 * sampler diverges: ve 15 against 1.45 with four shards).  bwgr_group_create therefore REFUSES G > 1 on uncentred columns (BWGR_EINVAL)
 * unless BWGR_GROUP_ALLOW_UNCENTRED=1 is set; bwgr_group_sound says which case a group is in.  Centring is a change
 * of the model's parametrisation under the flat intercept prior (src/Rcpp20260726ai.cpp:683-684; the intercept absorbs sum_j mean_j b_j), which an
 * exact Gibbs sampler would not notice; bWGR's own chain does, a little (its xx_j carry the squared means: DESIGN.md section 8 -- ve 1.47 uncentred
 * against 1.56 centred on the probe panel), so "sound" here means: follows the exact chain on the SAME centred panel.  X is a HOST matrix (column-major n x p, ldx >= n), y n host floats; device g
 * of `devices` takes the block-aligned column shard g.  markers_per_sync: markers swept per device between two all-reduces
 * (0: 131072 / ndev; 131072 when the shards share one device, where an exchange costs a launch boundary, not a ring).  bwgr_group_result returns the Bayes* return list over the whole panel (b, d, pval: p floats; vb: p
 * floats for BayesA/B/L/Dpi, else 1; hat: n floats).  info: {devices, exchange rounds per sweep, markers per round, RCCL in use}. */
typedef struct bwgr_group bwgr_group;
int bwgr_group_create(bwgr_group **out, int ndev, const int *devices, const void *X, int xtype, int64_t n, int64_t p, int64_t ldx,
                      int block, const float *y, int model, float it, float bi, float pi, float df, float R2, uint64_t seed,
                      int rng_mode, int64_t markers_per_sync);
/* the same on the IMPLICITLY centred columns of an int8 matrix (bwgr_panel_set_centred on every shard: the genotypes stay int8, k_sweep3 sweeps them):
 * sound with several devices; selection models only; the intercept returned is that of the centred parametrisation (mu_c = mu + sum_j mean_j b_j).
 * memloc: where X lives (BWGR_DEVICE: only when every shard sits on that device).
 * SHARDS SIDE BY SIDE ON ONE GPU: `devices` may name the same device ndev times (both create calls).  One exact chain is a latency-bound pipeline
 * that occupies a third of the chip; the shards of the partitioned sampler then run their sweeps concurrently on streams of their own, each on its own
 * compute units, and an exchange round is a sum kernel between events (no RCCL).  Same sampler, same soundness rule (centred columns) as across GPUs. */
int bwgr_group_create_centred(bwgr_group **out, int ndev, const int *devices, const void *X, int xtype, int64_t n, int64_t p, int64_t ldx,
                              int block, const float *y, int model, float it, float bi, float pi, float df, float R2, uint64_t seed,
                              int rng_mode, int64_t markers_per_sync, int memloc);
int bwgr_group_run(bwgr_group *G, int iters);
int bwgr_group_sync(bwgr_group *G);
int bwgr_group_info(const bwgr_group *G, int64_t info[4]);
int bwgr_group_sound(const bwgr_group *G, int *sound);      /* 1: one device (exact chain) or centred columns; 0: G > 1 on uncentred columns */
int bwgr_panel_centred(bwgr_panel *P, int *centred);        /* 1 when every column's |mean| <= 1e-3 sd (from the panel's own statistics), or after
                                                               bwgr_panel_set_centred(P, 1) */
/* Implicit centring of an int8 panel (no reference counterpart: bWGR sweeps whatever columns it is given, src/Rcpp20260726ai.cpp:668-682; centring
 * is the caller's preprocessing there).  on != 0: from now on the fused chains on this panel and its clones (bwgr_chain_*, bwgr_bayes, the chains
 * bwgr_group_* builds) sweep the columns x_j - mean(x_j) -- the same chain as on an explicitly centred float copy of the panel, to the float
 * rounding of that copy's entries -- while the genotypes stay int8 in HBM and every kernel keeps reading the raw columns: with s_j = sum_i x_ij and
 * the residual carried as e_stored = e - shift * 1,  (x_j - s_j/n 1)'e = x_j'e_stored - (s_j/n) sum(e_stored), and sum(e_stored) moves by -s_k delta_k
 * per marker: scalars on the sequencer, nothing on the streamers.  bwgr_panel_stats then returns xx_j = |x_j - mean_j|^2 (vx, MSx do not change),
 * hat = X_c B + mu, bwgr_panel_centred answers 1, and the group entry points accept several devices.  Selection models (BayesB / C /
 * Cpi / Dpi) on int8 panels that have k_sweep3, at every inclusion rate (both of their engines carry the terms, and so does the fp64 redo of a sweep
 * that leaves the fixed-point range); the affine models and the non-chain entry points (KMUP, wgr, EM, two-effect samplers, pairs) return BWGR_EINVAL
 * on a centred panel.  Refused while chains are alive on the panel; on == 0 switches back. */
int bwgr_panel_set_centred(bwgr_panel *P, int on);
int bwgr_group_result(bwgr_group *G, float *mu, float *b, float *d, float *hat, float *vb, float *ve, float *h2, float *MSx,
                      float *pi_out, float *pval);
int bwgr_group_destroy(bwgr_group *G);

/* ---- test hooks -----------------------------------------------------------------------------------
 * variates of the RNG contract computed on the device: kind 0 normal, 1 uniform, 2 chisq(nu);
 * out[i] for marker = marker0 + i. */
int bwgr_debug_variates(int device, uint64_t seed, int kind, double nu, uint32_t marker0, uint32_t iter,
                        uint32_t purpose, int count, double *out_host);
/* abort-path hook: while on != 0, sweeps launched on this panel run with slab workgroup 0 absent; every workgroup that waits
 * for it reaches its wall-clock bound (4 s), the shared abort word ends the launch and the call reports BWGR_ETIMEOUT.  The
 * panel stays usable: switch the hook off and launch again. */
int bwgr_debug_withhold(bwgr_panel *P, int on);
/* the sweeps that the calling thread's last bwgr_kmup / bwgr_kmup2 / bwgr_wgr / bwgr_wgr_ex call redid on the fp64 residual because they left
 * the fixed-point range of their engine: what bwgr_chain_redo_count is for a chain, for the entry points that have none. */
int bwgr_debug_last_redo(int *count);
/* host arithmetic of the launch grids of the fp64 families' tail, product and finish kernels (needs no GPU), in the style of
 * bwgr_debug_panel_plan, for a panel of n rows padded to ld (a multiple of 128, ld >= n), p markers and k columns of B (each at least 1, else
 * BWGR_EINVAL).  Every such kernel runs 256 threads per workgroup and strides over its rows, markers or entries by its grid.  out[0..2], mrr:
 * workgroups of the tail reductions k_mrr_ey (256 rows per trip) and k_mrr_tilde (256 markers per trip); of k_mrr_setup_cols (4 markers per
 * trip); of k_mrr_pass (one 64-row tile per trip).  out[3..6], uvbeta: workgroups of the tail reductions k_uvb_rows (256 rows per trip) and
 * k_uvb_cols; of k_uvb_pass (one 64-row tile per trip); of k_uvb_mu_shift per trait (256 rows per trip); of k_uvb_xb along the rows.
 * out[7..12], bwgr_panel_xb: rows per workgroup of k_pxb, then its row tiles, 16-column slices, marker chunks and markers per chunk (the last
 * chunk takes what is left), and the workgroups of k_pxb_finish (256 entries per trip).  out[13..14], the relationship kernels: workgroups
 * of k_xxt_zero and of k_kfin_apply (256 of the n x n entries per trip).  out[15]: the threads per workgroup of all of these.  out[16..17],
 * the constants of bwgr_panel_xb's chunk rule: the most chunks it asks for before it rounds the chunk up to whole staged tiles of B, and the
 * markers of such a tile. */
#define BWGR_LAUNCH_PLAN_NOUT 18
int bwgr_debug_launch_plan(int64_t n, int64_t ld, int64_t p, int64_t k, int64_t out[BWGR_LAUNCH_PLAN_NOUT]);
/* the device arrays, streams and events that the library's holders (csrc/devbufs.h) own in this process right now -- every handle's and every
 * running call's: out[0..2].  What a destroyed handle or a finished call took is gone from the counts. */
int bwgr_debug_live(int64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
