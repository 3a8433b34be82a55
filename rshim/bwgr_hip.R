# rshim/bwgr_hip.R -- R front-end over rshim/bwgr_shim.c: same names, argument order, defaults and return lists as
# R/RcppExports.R:4-6,48-74 and R/wgr.R:2-8, so that sourcing this file after library(bWGR) switches the Gibbs hot path to
# the MI355X engine.  SOURCE ONLY (no R in the build image; see INTEGRATION.md).
# dyn.load("bwgrhip.so")

.bwgr_panel <- function(X, device = 0L) if (inherits(X, "externalptr")) X else .Call("bwgrhip_panel", X, as.integer(device))
.bwgr_iter <- local({ i <- -1L; function() { i <<- i + 1L; i } })   # iteration word of the RNG counter for bare KMUP calls

KMUP <- function(X, b, d, xx, e, L, Ve, pi) .Call("bwgrhip_KMUP", .bwgr_panel(X), as.double(b), as.double(d), as.double(xx), as.double(e), as.double(L), as.double(Ve), as.double(pi), .bwgr_iter())
KMUP2 <- function(X, Use, b, d, xx, E, L, Ve, pi) .Call("bwgrhip_KMUP2", .bwgr_panel(X), as.double(Use), as.double(b), as.double(d), as.double(xx), as.double(E), as.double(L), as.double(Ve), as.double(pi), .bwgr_iter())

.bwgr_fused <- function(model, y, X, it, bi, pi, df, R2) .Call("bwgrhip_Bayes", as.integer(model), as.double(y), .bwgr_panel(X), as.double(it), as.double(bi), as.double(pi), as.double(df), as.double(R2))
BayesA   <- function(y, X, it = 1500, bi = 500, df = 5, R2 = 0.5) .bwgr_fused(0L, y, X, it, bi, 0, df, R2)
BayesB   <- function(y, X, it = 1500, bi = 500, pi = 0.95, df = 5, R2 = 0.5) .bwgr_fused(1L, y, X, it, bi, pi, df, R2)
BayesC   <- function(y, X, it = 1500, bi = 500, pi = 0.95, df = 5, R2 = 0.5) .bwgr_fused(2L, y, X, it, bi, pi, df, R2)
BayesL   <- function(y, X, it = 1500, bi = 500, df = 5, R2 = 0.5) .bwgr_fused(3L, y, X, it, bi, 0, df, R2)
BayesRR  <- function(y, X, it = 1500, bi = 500, df = 5, R2 = 0.5) .bwgr_fused(4L, y, X, it, bi, 0, df, R2)
BayesCpi <- function(y, X, it = 1500, bi = 500, df = 5, R2 = 0.5) .bwgr_fused(5L, y, X, it, bi, 0, df, R2)
BayesDpi <- function(y, X, it = 1500, bi = 500, df = 5, R2 = 0.5) .bwgr_fused(6L, y, X, it, bi, 0, df, R2)
# two-effect samplers, R/RcppExports.R (BayesA2, BayesB2, BayesRR2): the two panels must share the slab geometry, so the
# second is staged with the first one's workgroup count
.bwgr_fused2 <- function(model, y, X1, X2, it, bi, pi, df, R2) .Call("bwgrhip_Bayes2", as.integer(model), as.double(y), .bwgr_panel(X1), .bwgr_panel(X2), as.double(it), as.double(bi), as.double(pi), as.double(df), as.double(R2))
BayesA2  <- function(y, X1, X2, it = 1500, bi = 500, df = 5, R2 = 0.5) .bwgr_fused2(0L, y, X1, X2, it, bi, 0, df, R2)
BayesB2  <- function(y, X1, X2, it = 1500, bi = 500, pi = 0.95, df = 5, R2 = 0.5) .bwgr_fused2(1L, y, X1, X2, it, bi, pi, df, R2)
BayesRR2 <- function(y, X1, X2, it = 1500, bi = 500, df = 5, R2 = 0.5) .bwgr_fused2(4L, y, X1, X2, it, bi, 0, df, R2)

wgr <- function(y, X, it = 1500, bi = 500, th = 1, bag = 1, rp = FALSE, iv = FALSE, de = FALSE, pi = 0, df = 5, R2 = 0.5,
                eigK = NULL, VarK = 0.95, verb = FALSE) {
  if (bag != 1 && !is.null(eigK)) stop("bag != 1 with eigK is undefined in bWGR (R/wgr.R:73-79); not supported")
  if (bag != 1) df <- df   # df/(bag^2) (R/wgr.R:20) is applied inside the engine
  if (anyNA(X)) {                       # R/wgr.R:12-18
    imp <- function(x) { x[is.na(x)] <- mean(x, na.rm = TRUE); x[is.nan(x)] <- 0; x }
    X <- apply(X, 2, imp)
  }
  gen0 <- X; mis <- integer(0)           # R/wgr.R:10: predictions are returned for every row of gen0
  if (anyNA(y)) { mis <- which(is.na(y)); y <- y[-mis]; X <- X[-mis, , drop = FALSE] }   # R/wgr.R:34-39
  U <- U0 <- V <- NULL
  if (!is.null(eigK)) {                  # R/wgr.R:23-27; the rows of missing y are dropped from U for the sweeps (:37)
    V <- eigK$values; pk <- which.max((cumsum(V) / length(V)) > VarK)
    U0 <- eigK$vectors[, 1:pk, drop = FALSE]; V <- V[1:pk]
    U <- if (length(mis)) U0[-mis, , drop = FALSE] else U0
  }
  fit <- .Call("bwgrhip_wgr", as.double(y), .bwgr_panel(X), as.integer(it), as.integer(bi), as.integer(th), as.logical(iv), as.logical(de),
               as.double(pi), as.double(df), as.double(R2), U, V, as.double(bag), as.logical(rp))
  if (length(mis)) {                     # R/wgr.R:146-153: HAT = B0 + gen0 %*% B (+ U0 %*% H) over ALL rows, missing-y rows included
    hat <- matrix(0, nrow(gen0), 1); hat[-mis, 1] <- fit$hat
    hat[mis, 1] <- fit$mu + gen0[mis, , drop = FALSE] %*% fit$b
    if (!is.null(U0)) {
      H <- qr.solve(U, fit$u)            # u = U %*% H on the swept rows; H recovered for the rows that were left out
      poly <- U0 %*% H; hat[mis, 1] <- hat[mis, 1] + poly[mis]; fit$u <- poly
    }
    fit$hat <- hat
  }
  fit
}

# EM / Gauss-Seidel family, R/RcppExports.R (emRR, emBA, emBB, emBC, emBCpi, emDE, emBL, emEN, emML): same names, argument
# order and defaults; the marker order of every sweep is the reference's std::shuffle(order, std::mt19937(i))
.bwgr_em <- function(model, y, gen, df, R2, par, D = NULL) .Call("bwgrhip_em", as.integer(model), as.double(y), .bwgr_panel(gen), as.double(df), as.double(R2), as.double(par), D)
emRR   <- function(y, gen, df = 10, R2 = 0.5) .bwgr_em(0L, y, gen, df, R2, 0)
emBA   <- function(y, gen, df = 10, R2 = 0.5) .bwgr_em(1L, y, gen, df, R2, 0)
emDE   <- function(y, gen, R2 = 0.5) .bwgr_em(2L, y, gen, 0, R2, 0)
emML   <- function(y, gen, D = NULL) .bwgr_em(3L, y, gen, 0, 0.5, 0, D)
emBB   <- function(y, gen, df = 10, R2 = 0.5, Pi = 0.75) .bwgr_em(4L, y, gen, df, R2, Pi)
emBC   <- function(y, gen, df = 10, R2 = 0.5, Pi = 0.75) .bwgr_em(5L, y, gen, df, R2, Pi)
emBCpi <- function(y, gen, df = 10, R2 = 0.5, Pi = 0.75) .bwgr_em(6L, y, gen, df, R2, Pi)
emBL   <- function(y, gen, R2 = 0.5, alpha = 0.02) .bwgr_em(7L, y, gen, 0, R2, alpha)
emEN   <- function(y, gen, R2 = 0.5, alpha = 0.02) .bwgr_em(8L, y, gen, 0, R2, alpha)
lasso  <- function(y, gen) .bwgr_em(9L, y, gen, 0, 0.5, 0)
# multi-trait ridge regression, R/RcppExports.R:180-186 (MRR3, MRR3F) and R/mix.R:1271-1273 (mrr, mrr_float): same names, argument
# order, defaults and return list.  `cores` is ignored; InnerGS, NoInv, NLfactor / NonLinearFactor, PenCor, MinCor, uncorH2below,
# round*, bucket* and DeflateBy are refused away from their defaults (include/bwgr.h).  Y: NA = missing.
.bwgr_mrr_opts <- function(maxit, tol, TH, NLfactor, InnerGS, NoInv, HCS, XFA, ACS, NumXFA, R2, gc0, df0, updateMu, weight_prior_h2, weight_prior_gc, PenCor, MinCor, uncorH2below, roundGCupFrom, roundGCupTo, roundGCdownFrom, roundGCdownTo, bucketGCfrom, bucketGCto, DeflateMax, DeflateBy, OneVarB, OneVarE, verbose)
  as.double(c(maxit, tol, TH, NLfactor, InnerGS, NoInv, HCS, XFA, ACS, NumXFA, R2, gc0, df0, updateMu, weight_prior_h2, weight_prior_gc, PenCor, MinCor, uncorH2below, roundGCupFrom, roundGCupTo, roundGCdownFrom, roundGCdownTo, bucketGCfrom, bucketGCto, DeflateMax, DeflateBy, OneVarB, OneVarE, verbose))
.bwgr_f32 <- function(x) { storage.mode(x) <- "double"; x[] <- as.double(sprintf("%.9g", x)); x }   # float-rounded, as MRR3F receives its inputs
MRR3 <- function(Y, X, maxit = 500L, tol = 10e-9, cores = 1L, TH = FALSE, NLfactor = 0.0, InnerGS = FALSE, NoInv = FALSE, HCS = FALSE, XFA = FALSE, ACS = FALSE, NumXFA = 3L, R2 = 0.5, gc0 = 0.5, df0 = 1.0, updateMu = FALSE, weight_prior_h2 = 0.01, weight_prior_gc = 0.01, PenCor = 0.0, MinCor = 1.0, uncorH2below = 0.0, roundGCupFrom = 1.0, roundGCupTo = 1.0, roundGCdownFrom = 1.0, roundGCdownTo = 0.0, bucketGCfrom = 1.0, bucketGCto = 1.0, DeflateMax = 0.9, DeflateBy = 0.0, OneVarB = FALSE, OneVarE = FALSE, verbose = FALSE)
  .Call("bwgrhip_MRR3", as.matrix(Y) * 1.0, .bwgr_panel(X), .bwgr_mrr_opts(maxit, tol, TH, NLfactor, InnerGS, NoInv, HCS, XFA, ACS, NumXFA, R2, gc0, df0, updateMu, weight_prior_h2, weight_prior_gc, PenCor, MinCor, uncorH2below, roundGCupFrom, roundGCupTo, roundGCdownFrom, roundGCdownTo, bucketGCfrom, bucketGCto, DeflateMax, DeflateBy, OneVarB, OneVarE, verbose))
MRR3F <- function(Y, X, maxit = 500L, tol = 10e-9, cores = 1L, TH = FALSE, NonLinearFactor = 0.0, InnerGS = FALSE, NoInv = FALSE, HCS = FALSE, XFA = FALSE, ACS = FALSE, NumXFA = 3L, R2 = 0.5, gc0 = 0.5, df0 = 1.0, updateMu = FALSE, weight_prior_h2 = 0.01, weight_prior_gc = 0.01, PenCor = 0.0, MinCor = 1.0, uncorH2below = 0.0, roundGCupFrom = 1.0, roundGCupTo = 1.0, roundGCdownFrom = 1.0, roundGCdownTo = 0.0, bucketGCfrom = 1.0, bucketGCto = 1.0, DeflateMax = 0.9, DeflateBy = 0.0, OneVarB = FALSE, OneVarE = FALSE, verbose = FALSE)
  .Call("bwgrhip_MRR3F", .bwgr_f32(as.matrix(Y)), .bwgr_panel(X), .bwgr_mrr_opts(maxit, tol, TH, NonLinearFactor, InnerGS, NoInv, HCS, XFA, ACS, NumXFA, R2, gc0, df0, updateMu, weight_prior_h2, weight_prior_gc, PenCor, MinCor, uncorH2below, roundGCupFrom, roundGCupTo, roundGCdownFrom, roundGCdownTo, bucketGCfrom, bucketGCto, DeflateMax, DeflateBy, OneVarB, OneVarE, verbose))
mrr <- function(Y, X, ...) MRR3(Y, X, ...)
mrr_float <- function(Y, X, ...) MRR3F(Y, X, ...)
# K2X(K, MinEV, cores), R/RcppExports.R:256, and mkr(Y, K, ...) = MRR3(Y, K2X(K), ...), R/mix.R:1275.  K2X: the eigenvectors of the symmetric K
# times |eigenvalue| (U D of the reference's SVD, not U sqrt(D): X X' = K K), by decreasing |eigenvalue|, those above MinEV, float-rounded.
# The count is made on base eigen()'s fp64 spectrum (the reference counts on a float SVD and keeps a rank-deficient K's null directions).
# mkr takes MRR3's arguments after K; its `b` are the effects of K2X's columns.  `cores` is ignored.
K2X <- function(K, MinEV = 1e-8, cores = 1L) {
  K <- as.matrix(K) * 1.0
  if (nrow(K) != ncol(K)) stop("K2X: K must be square")
  if (max(abs(K - t(K))) > 1e-6 * max(abs(K))) stop("K2X: K is not symmetric")
  es <- eigen((K + t(K)) / 2, symmetric = TRUE)
  o <- order(-abs(es$values))
  o <- o[abs(es$values[o]) > MinEV]
  .bwgr_f32(es$vectors[, o, drop = FALSE] %*% diag(abs(es$values[o]), length(o)))
}
.bwgr_mrr_dense <- function(Y, X, maxit = 500L, tol = 10e-9, cores = 1L, TH = FALSE, NLfactor = 0.0, InnerGS = FALSE, NoInv = FALSE, HCS = FALSE, XFA = FALSE, ACS = FALSE, NumXFA = 3L, R2 = 0.5, gc0 = 0.5, df0 = 1.0, updateMu = FALSE, weight_prior_h2 = 0.01, weight_prior_gc = 0.01, PenCor = 0.0, MinCor = 1.0, uncorH2below = 0.0, roundGCupFrom = 1.0, roundGCupTo = 1.0, roundGCdownFrom = 1.0, roundGCdownTo = 0.0, bucketGCfrom = 1.0, bucketGCto = 1.0, DeflateMax = 0.9, DeflateBy = 0.0, OneVarB = FALSE, OneVarE = FALSE, verbose = FALSE)
  .Call("bwgrhip_mrr_dense", as.matrix(Y) * 1.0, as.matrix(X) * 1.0, .bwgr_mrr_opts(maxit, tol, TH, NLfactor, InnerGS, NoInv, HCS, XFA, ACS, NumXFA, R2, gc0, df0, updateMu, weight_prior_h2, weight_prior_gc, PenCor, MinCor, uncorH2below, roundGCupFrom, roundGCupTo, roundGCdownFrom, roundGCdownTo, bucketGCfrom, bucketGCto, DeflateMax, DeflateBy, OneVarB, OneVarE, verbose))
mkr <- function(Y, K, ...) .bwgr_mrr_dense(Y, K2X(K), ...)
# per-trait ridge fits, R/RcppExports.R:196-238 (solver1x, UVBETA, solver1xF, FUVBETA, XFUVBETA, ZFUVBETA): same names, argument order,
# defaults and return shapes.  Integer genotypes only (an int8 panel).  Y: NA = missing; every trait is fitted on its own observed rows.
# A trait without observed rows gives a zero column (XFUVBETA too).  The float solvers receive float-rounded Y, tol and df0.
solver1x <- function(Y, X, maxit = 100L, tol = 10e-7, df0 = 20.0)
  .Call("bwgrhip_solver1x", as.double(Y), .bwgr_ipanel(X), 0L, as.integer(maxit), as.double(tol), as.double(df0))
solver1xF <- function(Y, X, maxit = 100L, tol = 10e-7, df0 = 20.0)
  .Call("bwgrhip_solver1x", .bwgr_f32(as.double(Y)), .bwgr_ipanel(X), 1L, as.integer(maxit), .bwgr_f32(tol), .bwgr_f32(df0))
UVBETA <- function(Y, X) .Call("bwgrhip_UVBETA", as.matrix(Y) * 1.0, .bwgr_ipanel(X), 0L)
FUVBETA <- function(Y, X) .Call("bwgrhip_UVBETA", .bwgr_f32(as.matrix(Y)), .bwgr_ipanel(X), 1L)
XFUVBETA <- function(Y, X) .Call("bwgrhip_UVBETA", .bwgr_f32(as.matrix(Y)), .bwgr_ipanel(X), 2L)
ZFUVBETA <- function(Y, X) .Call("bwgrhip_UVBETA", .bwgr_f32(as.matrix(Y)), .bwgr_ipanel(X), 3L)
# latent-space fits, R/RcppExports.R:232, 240, 244 (XSEMF, ZSEMF, YSEMF; src/RcppEigen20230423.cpp:1756-1769, :1819-1874): same names, argument
# order, defaults and return lists.  Composed from the per-trait fits on the panel, X %*% B on the panel, base R's svd() of the n x k matrix
# G and the per-trait fits on the dense latent design.  Y is rounded to float once; everything after runs on unrounded doubles (the reference
# computes in float throughout).  The results do not depend on the signs svd() gives the singular pairs.
.bwgr_uvb <- function(Y, P, variant) {      # list(b, mu, h2) of the panel fit
  r <- .Call("bwgrhip_UVBETA", Y, P, variant)
  if (variant == 3L) list(b = r[-(1:2), , drop = FALSE], mu = r[2, ], h2 = r[1, ]) else list(b = r)
}
.bwgr_uvbd <- function(Y, Z, variant) .Call("bwgrhip_uvbeta_dense", Y, Z, variant, 100L, .bwgr_f32(10e-7), .bwgr_f32(20.0))
.bwgr_xb <- function(P, B) .Call("bwgrhip_panel_xb", P, B * 1.0)
.bwgr_latent <- function(G, npc) {          # Z = (U diag(s)).leftCols(npc), V.leftCols(npc), :1759-1762
  s <- svd(G); m <- length(s$d)
  if (npc < 0) npc <- floor(2 * sqrt(m) + 0.5)
  if (npc == 0) npc <- m
  if (npc > m) stop("npc exceeds min(nrow(Y), ncol(Y))")
  i <- seq_len(npc)
  list(Z = s$u[, i, drop = FALSE] %*% diag(s$d[i], npc), V = s$v[, i, drop = FALSE])
}
.bwgr_gc <- function(G) {                   # :1765-1768: list(hat = standardised columns, GC)
  G <- sweep(G, 2, colMeans(G)); G <- sweep(G, 2, sqrt(colSums(G^2) / nrow(G)), "/")
  list(hat = G, GC = crossprod(G) / nrow(G))
}
.bwgr_sem <- function(Y, X, npc, variant) {
  P <- .bwgr_ipanel(X); Y <- .bwgr_f32(as.matrix(Y))
  s1 <- .bwgr_uvb(Y, P, variant)
  L <- .bwgr_latent(.bwgr_xb(P, s1$b), npc)
  s2 <- .bwgr_uvbd(Y, L$Z, variant)
  list(P = P, Y = Y, s2 = s2, b = s1$b %*% (L$V %*% s2$b))
}
XSEMF <- function(Y, X, npc = 0L) {
  f <- .bwgr_sem(Y, X, npc, 2L); g <- .bwgr_gc(.bwgr_xb(f$P, f$b))
  list(b = f$b, GC = g$GC, hat = g$hat)
}
ZSEMF <- function(Y, X, npc = 0L) {
  f <- .bwgr_sem(Y, X, npc, 3L); G <- .bwgr_xb(f$P, f$b)
  list(mu = f$s2$mu, b = f$b, hat = sweep(G, 2, f$s2$mu, "+"), h2 = f$s2$h2, GC = .bwgr_gc(G)$GC)
}
YSEMF <- function(Y, X, npc = -1L) {
  f <- .bwgr_sem(Y, X, npc, 3L)
  s3 <- .bwgr_uvb(f$Y - .bwgr_xb(f$P, f$b), f$P, 3L)
  b <- f$b + s3$b; G <- .bwgr_xb(f$P, b)
  list(mu = s3$mu, b = b, hat = sweep(G, 2, s3$mu, "+"), h2 = f$s2$h2 + s3$h2, GC = .bwgr_gc(G)$GC)
}
# multi-trait fits over several designs, R/RcppExports.R:280, 288 (PEGS, PEGSZ; src/RcppEigenX20251203.cpp:10-194, :576-808): same names,
# argument order, defaults and return lists.  An effect is a panel effect -- a panel handle, an integer matrix or an integer-valued numeric
# matrix within int8 range, staged as int8 genotypes and NOT centred -- or a dense effect: a numeric matrix with a non-integer value, or any
# matrix passed as dense(Z).  Y and the real options are float-rounded, as the reference receives them.  The marker order of a sweep is the
# library's own (the reference seeds it from the machine).
# A third kind is a sparse effect: a sparse matrix of the Matrix package (a dgCMatrix as it is, any other sparseMatrix converted to one) or
# any matrix passed as sparse(S), whose nonzeros are taken -- the incidence matrix of environments, blocks or genotype-by-environment cells,
# held column-compressed on the device.  Its @i, @p, @x and @Dim travel to C as plain vectors; the values are float-rounded, as the
# reference casts them.  PEGS_sparse and PEGSZ_sparse (R/RcppExports.R:292, 296; src/RcppEigenX20251203.cpp:811-1007, :1010-1250) are the
# same fit under their own texts: text 1 (PEGS's) and text 2 (PEGSZ_sparse's, whose intercept step divides by n where PEGSZ divides by n - 1).
dense <- function(Z) structure(as.matrix(Z) * 1.0, class = c("bwgr_dense", "matrix"))
sparse <- function(S) {
  if (inherits(S, "bwgr_sparse")) return(S)
  if (inherits(S, "sparseMatrix")) {
    if (!inherits(S, "dgCMatrix")) S <- methods::as(methods::as(methods::as(S, "dMatrix"), "generalMatrix"), "CsparseMatrix")
    return(structure(list(i = as.integer(S@i), p = as.integer(S@p), x = .bwgr_f32(as.double(S@x)), Dim = as.integer(S@Dim)), class = "bwgr_sparse"))
  }
  S <- as.matrix(S) * 1.0
  nz <- which(S != 0, arr.ind = TRUE)                      # by column, rows ascending within one
  structure(list(i = as.integer(nz[, 1] - 1L), p = as.integer(c(0L, cumsum(tabulate(nz[, 2], ncol(S))))), x = .bwgr_f32(as.double(S[nz])),
                 Dim = as.integer(dim(S))), class = "bwgr_sparse")
}
.bwgr_pegs_effect <- function(X) {
  if (inherits(X, "externalptr")) return(X)
  if (inherits(X, "bwgr_dense")) return(unclass(X))
  if (inherits(X, "bwgr_sparse") || inherits(X, "sparseMatrix")) return(sparse(X))
  X <- as.matrix(X)
  if (is.integer(X) || (!anyNA(X) && all(X == round(X)) && all(abs(X) <= 127))) .bwgr_ipanel(X) else X * 1.0
}
# the effects into a set, one by one; round: dense effects are float-rounded first.  Returns the effects as they were put (the caller keeps them alive).
.bwgr_pegs_fill <- function(set, eff, round) {
  for (i in seq_along(eff)) {
    if (inherits(eff[[i]], "bwgr_sparse")) {
      .Call("bwgrhip_pegs_put_sparse", set, i - 1L, eff[[i]]$i, eff[[i]]$p, eff[[i]]$x, eff[[i]]$Dim)
      next
    }
    isz <- is.matrix(eff[[i]])
    if (isz && round) eff[[i]] <- .bwgr_f32(eff[[i]])
    pan <- if (isz) NULL else eff[[i]]
    Z <- if (isz) eff[[i]] else NULL
    .Call("bwgrhip_pegs_put", set, i - 1L, pan, Z)
  }
  eff
}
.bwgr_pegs <- function(Y, X_list, maxit, logtol, covbend, covMinEv, XFA, NNC, text) {
  eff <- lapply(X_list, .bwgr_pegs_effect)
  set <- .Call("bwgrhip_pegs_set", length(eff))
  eff <- .bwgr_pegs_fill(set, eff, FALSE)
  r <- .Call("bwgrhip_pegs", set, .bwgr_f32(as.matrix(Y)), as.integer(maxit), .bwgr_f32(logtol), .bwgr_f32(covbend), .bwgr_f32(covMinEv), as.integer(XFA), as.logical(NNC), as.integer(text))
  rm(eff)
  r
}
PEGS <- function(Y, X, maxit = 100L, logtol = -4.0, covbend = 1.1, covMinEv = 10e-4, XFA = -1L, NNC = TRUE) {
  r <- .bwgr_pegs(Y, list(X), maxit, logtol, covbend, covMinEv, XFA, NNC, 1L)
  r$b <- r$b[[1]]; r$GC <- r$GC[[1]]
  r
}
PEGSZ <- function(Y, X_list, maxit = 100L, logtol = -4.0, covbend = 1.1, covMinEv = 10e-4, XFA = -1L, NNC = TRUE)
  .bwgr_pegs(Y, X_list, maxit, logtol, covbend, covMinEv, XFA, NNC, 0L)
PEGS_sparse <- function(Y, S, maxit = 100L, logtol = -4.0, covbend = 1.1, covMinEv = 10e-4, XFA = -1L, NNC = TRUE) {
  r <- .bwgr_pegs(Y, list(sparse(S)), maxit, logtol, covbend, covMinEv, XFA, NNC, 1L)
  r$b <- r$b[[1]]; r$GC <- r$GC[[1]]
  r
}
PEGSZ_sparse <- function(Y, X_list, maxit = 100L, logtol = -4.0, covbend = 1.1, covMinEv = 10e-4, XFA = -1L, NNC = TRUE)
  .bwgr_pegs(Y, lapply(X_list, function(X) if (inherits(X, "externalptr") || inherits(X, "bwgr_dense")) X else sparse(X)), maxit, logtol, covbend, covMinEv, XFA, NNC, 2L)
# fixed effects beside the random effects, R/RcppExports.R:284 (PEGSX; src/RcppEigenX20251203.cpp:197-573): same name, argument order, defaults
# and return list.  X is the fixed design (an intercept is a column of it; nothing is centred); every element of Z_list is an effect as for
# PEGSZ, sparse ones included.  Y, X, the dense effects and the real options are float-rounded.  InnerGS = TRUE and NoInv = TRUE are refused by the library; cores
# and verbose are accepted and ignored.  MLM is not here: it projects Z off X, which makes the int8 panel dense.
PEGSX <- function(Y, X, Z_list, maxit = 500L, logtol = -8.0, covbend = 1.1, covMinEv = 10e-4, cores = 1L, verbose = FALSE, df0 = 1.1, NNC = FALSE,
                  InnerGS = FALSE, NoInv = FALSE, XFA = FALSE, NumXFA = 3L) {
  eff <- lapply(Z_list, .bwgr_pegs_effect)
  set <- .Call("bwgrhip_pegs_set", length(eff))
  eff <- .bwgr_pegs_fill(set, eff, TRUE)
  opts <- c(as.integer(maxit), .bwgr_f32(logtol), .bwgr_f32(covbend), .bwgr_f32(covMinEv), .bwgr_f32(df0), as.logical(NNC), as.logical(InnerGS),
            as.logical(NoInv), as.logical(XFA), as.integer(NumXFA)) * 1.0
  r <- .Call("bwgrhip_pegsx", set, .bwgr_f32(as.matrix(Y)), .bwgr_f32(as.matrix(X) * 1.0), opts)
  rm(eff)
  r
}
# two designs in one sweep, R/RcppExports.R:200, 208, 212 (solver2x, MEGA, GSEM; src/RcppEigen20230423.cpp:1446-1493, :1542-1610): same names,
# argument order, defaults and return lists; doubles throughout.  solver2x's X1 is the dense design and X2 the integer genotypes (an int8
# panel), as MEGA and GSEM call it; a dense X2 is not taken.  MEGA refuses a trait without records (the reference's imputed column is NaN);
# GSEM's b uses V.leftCols(npc) (:1609 multiplies by the whole V, conformable only for npc = min(n, k), where the two agree).  The results
# do not depend on the signs svd() gives the singular pairs; LS, LS_BETA and BETA1 are defined up to them.
.bwgr_uvb2 <- function(Y, Z, P, maxit = 100L, tol = 10e-7, df0 = 20.0)
  .Call("bwgrhip_uvbeta2", Y, Z * 1.0, P, as.integer(maxit), as.double(tol), as.double(df0))
solver2x <- function(Y, X1, X2, maxit = 100L, tol = 10e-7, df0 = 20.0) {
  r <- .bwgr_uvb2(as.matrix(as.double(Y)), as.matrix(X1), .bwgr_ipanel(X2), maxit, tol, df0)
  c(r$mu, r$b1[, 1], r$b2[, 1])
}
MEGA <- function(Y, X, npc = -1L) {
  P <- .bwgr_ipanel(X); Y <- as.matrix(Y) * 1.0; n <- nrow(Y)
  if (any(colSums(!is.na(Y)) == 0)) stop("MEGA: a trait has no record")
  BETA <- .bwgr_uvb(Y, P, 0L)$b
  Y2 <- sweep(Y, 2, colMeans(Y, na.rm = TRUE)); G <- .bwgr_xb(P, BETA)          # GetImputedY, :1517-1528
  Y2[is.na(Y)] <- G[is.na(Y)]
  Y2 <- sweep(Y2, 2, sqrt(colSums(Y2^2) / (n - 1)), "/")                         # :1533-1534
  LS <- .bwgr_latent(Y2, npc)$Z
  LS_BETA <- .bwgr_uvb(LS, P, 0L)$b
  f <- .bwgr_uvb2(Y, LS, P)
  b <- LS_BETA %*% f$b1 + f$b2
  XB <- .bwgr_xb(P, cbind(f$b2, b)); k <- ncol(Y)
  hat <- sweep(LS %*% f$b1 + XB[, seq_len(k), drop = FALSE], 2, f$mu, "+")
  gebv <- sweep(XB[, k + seq_len(k), drop = FALSE], 2, f$mu, "+")
  list(mu = f$mu, b = b, hat = hat, LS = LS, LS_BETA = LS_BETA, BETA1 = f$b1, BETA2 = f$b2, gebv = gebv)
}
GSEM <- function(Y, X, npc = -1L) {
  P <- .bwgr_ipanel(X); Y <- as.matrix(Y) * 1.0
  BETA <- .bwgr_uvb(Y, P, 0L)$b
  L <- .bwgr_latent(.bwgr_xb(P, BETA), npc)
  f <- .bwgr_uvb2(Y, L$Z, P)
  list(mu = f$mu, b = BETA %*% (L$V %*% f$b1) + f$b2, hat = sweep(L$Z %*% f$b1 + .bwgr_xb(P, f$b2), 2, f$mu, "+"))
}
# relationship kernels, R/RcppExports.R:100-106 (GAU, GRM) and :140-150 (EigenARC, EigenGAU, EigenGRM): same names, argument order and defaults;
# integer genotypes only (an int8 panel); `cores` is ignored.  Their result feeds wgr(eigK = eigen(K)).
# (a numeric matrix of whole numbers is staged as integers, so that it becomes an int8 panel)
.bwgr_ipanel <- function(X) { if (is.matrix(X) && is.double(X) && !anyNA(X) && all(X == round(X))) storage.mode(X) <- "integer"; .bwgr_panel(X) }
.bwgr_kernel <- function(kind, X, par = 1.0, flag = FALSE) .Call("bwgrhip_kernel", .bwgr_ipanel(X), as.integer(kind), as.double(par), as.integer(flag))
GRM      <- function(X, Code012 = FALSE) .bwgr_kernel(0L, X, 1.0, Code012)
GAU      <- function(X) .bwgr_kernel(1L, X)
EigenGRM <- function(X, centralizeZ = TRUE, cores = 1L) .bwgr_kernel(2L, X, 1.0, centralizeZ)
EigenGAU <- function(X, phi = 1.0, cores = 1L) .bwgr_kernel(3L, X, phi)
EigenARC <- function(X, centralizeX = TRUE, cores = 1L) .bwgr_kernel(4L, X, 1.0, centralizeX)
.bwgr_crossprod <- function(X) .Call("bwgrhip_crossprod", .bwgr_ipanel(X))   # the exact X X' (tcrossprod) of integer genotypes
# founder-by-sample kernels, R/RcppExports.R:248-254 (EigenArcZ, EigenGauZ; src/RcppEigen20230423.cpp:1877-1939): same names, argument order
# and defaults; integer genotypes only; `cores` is ignored.  The library makes K_ff and K_fs, eigen() here the founders' rotation; the result
# is the samples' coordinates t(K_fs) V L^(-1/2), nrow(Zsamp) x nrow(Zfndr).  Its columns are defined up to sign, and up to rotation inside
# close eigenvalues; Z Z' is not affected.  (eigen() returns descending eigenvalues, Eigen's solver ascending: the columns come reversed.)
.bwgr_kernel2 <- function(kind, Zfndr, Zsamp, par = 1.0) {
  if (ncol(Zfndr) != ncol(Zsamp)) stop("Zfndr and Zsamp must have the same columns (markers)")
  k <- .Call("bwgrhip_kernel2", .bwgr_ipanel(Zfndr), .bwgr_ipanel(Zsamp), as.integer(kind), as.double(par))
  e <- eigen(k$Kff, symmetric = TRUE); o <- rev(seq_along(e$values))
  k$Ksf %*% sweep(e$vectors[, o, drop = FALSE], 2, sqrt(e$values[o]), "/")
}
EigenArcZ <- function(Zfndr, Zsamp, cores = 1L) .bwgr_kernel2(0L, Zfndr, Zsamp)
EigenGauZ <- function(Zfndr, Zsamp, phi = 1.0, cores = 1L) .bwgr_kernel2(1L, Zfndr, Zsamp, phi)
.bwgr_crossprod2 <- function(Xf, Xs) .Call("bwgrhip_crossprod2", .bwgr_ipanel(Xf), .bwgr_ipanel(Xs))   # the exact Xs Xf' (tcrossprod(Xs, Xf))
