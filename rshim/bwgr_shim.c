/*
 * rshim/bwgr_shim.c -- the reference-side binding a bWGR maintainer would add: a thin .Call shim over the C ABI of
 * libbwgr_hip.so (include/bwgr.h).  SOURCE ONLY: R, Rinternals.h and libR do not exist in the build image, so this file
 * is not compiled or tested there.  Build where R exists with
 *     R CMD SHLIB bwgr_shim.c -I../include -L../bwgr_amd -lbwgr_hip -o bwgrhip.so
 *
 * It replaces the Rcpp-generated glue for the hot path:
 *     _bWGR_KMUP      src/RcppExports.cpp:16-31      -> bwgrhip_KMUP     (8 args)
 *     _bWGR_KMUP2     src/RcppExports.cpp:34-50      -> bwgrhip_KMUP2    (9 args)
 *     _bWGR_BayesA..  src/RcppExports.cpp:177-290    -> bwgrhip_Bayes    (model + 7 args)
 *     _bWGR_GRM, _bWGR_GAU, _bWGR_EigenGRM / GAU / ARC      -> bwgrhip_kernel   (kind + 2 args)
 *     _bWGR_EigenArcZ, _bWGR_EigenGauZ                      -> bwgrhip_kernel2  (kind + phi; eigen() stays in R)
 * and adds bwgrhip_wgr (R/wgr.R:2-169 as one device-resident call) plus panel handles so that X is staged in HBM
 * once instead of being converted SEXP -> Eigen::MatrixXf on every call (src/RcppExports.cpp:20).
 *
 * Conventions kept from the reference: inputs are never written (Rcpp passes by value, :20-27); outputs are fresh
 * vectors under PROTECT; errors become R conditions (BEGIN_RCPP/END_RCPP, :17,30) via Rf_error with
 * bwgr_last_error(); the seed is drawn from R's stream between GetRNGstate/PutRNGstate (Rcpp::RNGScope, :19) so
 * set.seed() governs repeatability.
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include <R_ext/Random.h>
#include <stdint.h>
#include <string.h>
#include "bwgr.h"

static void chk(int rc) { if (rc != BWGR_OK) Rf_error("bwgr: %s", bwgr_last_error()); }

static uint64_t seed_from_R(void) {
  GetRNGstate();
  uint64_t hi = (uint64_t)(unif_rand() * 4294967296.0), lo = (uint64_t)(unif_rand() * 4294967296.0);
  PutRNGstate();
  return (hi << 32) | lo;
}

static void panel_finalizer(SEXP ext) {
  bwgr_panel *P = (bwgr_panel *)R_ExternalPtrAddr(ext);
  if (P) { bwgr_panel_destroy(P); R_ClearExternalPtr(ext); }
}

/* X: numeric (double) or integer matrix, column-major as R stores it.  Integer matrices within int8 range are
 * staged as int8 genotypes, everything else as float (the narrowing Rcpp performs on every call). */
SEXP bwgrhip_panel(SEXP X, SEXP device) {
  SEXP dim = Rf_getAttrib(X, R_DimSymbol);
  if (Rf_length(dim) != 2) Rf_error("X must be a matrix");
  const int64_t n = INTEGER(dim)[0], p = INTEGER(dim)[1];
  bwgr_panel *P = NULL;
  if (TYPEOF(X) == INTSXP) {
    const int *xi = INTEGER(X);
    int8_t *x8 = (int8_t *)R_alloc((size_t)n * p, 1);
    int ok = 1;
    for (int64_t k = 0; k < n * p; k++) { if (xi[k] < -128 || xi[k] > 127) { ok = 0; break; } x8[k] = (int8_t)xi[k]; }
    if (ok) chk(bwgr_panel_create(&P, x8, BWGR_X_I8, BWGR_HOST, n, p, n, Rf_asInteger(device), 0, 0));
    else X = Rf_coerceVector(X, REALSXP);
  }
  if (!P) chk(bwgr_panel_create(&P, REAL(X), BWGR_X_F64, BWGR_HOST, n, p, n, Rf_asInteger(device), 0, 0));
  SEXP ext = PROTECT(R_MakeExternalPtr(P, R_NilValue, R_NilValue));
  R_RegisterCFinalizerEx(ext, panel_finalizer, TRUE);
  UNPROTECT(1);
  return ext;
}

static bwgr_panel *panel_of(SEXP ext) {
  bwgr_panel *P = (bwgr_panel *)R_ExternalPtrAddr(ext);
  if (!P) Rf_error("bwgr: panel was freed");
  return P;
}
static float *to_float(SEXP v, R_xlen_t n) {
  float *f = (float *)R_alloc((size_t)n, sizeof(float));
  const double *d = REAL(v);
  for (R_xlen_t k = 0; k < n; k++) f[k] = (float)d[k];
  return f;
}
static SEXP from_float(const float *f, R_xlen_t n) {
  SEXP v = PROTECT(Rf_allocVector(REALSXP, n));
  for (R_xlen_t k = 0; k < n; k++) REAL(v)[k] = (double)f[k];
  UNPROTECT(1);
  return v;
}
static SEXP named_list(int n, const char **names) {
  SEXP l = PROTECT(Rf_allocVector(VECSXP, n)), nm = PROTECT(Rf_allocVector(STRSXP, n));
  for (int k = 0; k < n; k++) SET_STRING_ELT(nm, k, Rf_mkChar(names[k]));
  Rf_setAttrib(l, R_NamesSymbol, nm);
  UNPROTECT(2);
  return l;
}

/* KMUP(X,b,d,xx,e,L,Ve,pi) -> list(b=,d=,e=)            src/Rcpp20260726ai.cpp:12-38 */
SEXP bwgrhip_KMUP(SEXP panel, SEXP b, SEXP d, SEXP xx, SEXP e, SEXP L, SEXP Ve, SEXP pi, SEXP iter) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  if (XLENGTH(b) != p || XLENGTH(d) != p || XLENGTH(xx) != p || XLENGTH(L) != p || XLENGTH(e) != n) Rf_error("KMUP: length mismatch");
  float *fb = to_float(b, p), *fd = to_float(d, p), *fxx = to_float(xx, p), *fe = to_float(e, n), *fL = to_float(L, p);
  chk(bwgr_kmup(P, fb, fd, fxx, fe, fL, (float)Rf_asReal(Ve), (float)Rf_asReal(pi), seed_from_R(), (uint32_t)Rf_asInteger(iter), BWGR_RNG_PHILOX));
  const char *nm[] = {"b", "d", "e"};
  SEXP out = PROTECT(named_list(3, nm));
  SET_VECTOR_ELT(out, 0, from_float(fb, p)); SET_VECTOR_ELT(out, 1, from_float(fd, p)); SET_VECTOR_ELT(out, 2, from_float(fe, n));
  UNPROTECT(1);
  return out;
}

/* BayesA/B/C/L/RR/Cpi/Dpi(y,X,it,bi,[pi,]df,R2)          src/Rcpp20260726ai.cpp:589-987; return lists :631-634,
 * :694-698, :916-920 (names and order kept) */
SEXP bwgrhip_Bayes(SEXP model, SEXP y, SEXP panel, SEXP it, SEXP bi, SEXP pi, SEXP df, SEXP R2) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  const int m = Rf_asInteger(model);
  if (XLENGTH(y) != n) Rf_error("length(y) must equal nrow(X)");
  const int per = (m == BWGR_BAYESA || m == BWGR_BAYESB || m == BWGR_BAYESL || m == BWGR_BAYESDPI);
  float *fy = to_float(y, n);
  float *B = (float *)R_alloc(p, 4), *D = (float *)R_alloc(p, 4), *hat = (float *)R_alloc(n, 4), *VB = (float *)R_alloc(per ? p : 1, 4), *PV = (float *)R_alloc(p, 4);
  float mu, ve, h2, MSx, Pi;
  chk(bwgr_bayes(P, m, fy, (float)Rf_asReal(it), (float)Rf_asReal(bi), (float)Rf_asReal(pi), (float)Rf_asReal(df), (float)Rf_asReal(R2),
                 seed_from_R(), BWGR_RNG_PHILOX, &mu, B, D, hat, VB, &ve, &h2, &MSx, &Pi, PV));
  SEXP out;
  if (m == BWGR_BAYESA || m == BWGR_BAYESL || m == BWGR_BAYESRR) {
    const char *nm[] = {"mu", "b", "hat", "vb", "ve", "h2", "MSx"};
    out = PROTECT(named_list(7, nm));
    SET_VECTOR_ELT(out, 0, Rf_ScalarReal(mu)); SET_VECTOR_ELT(out, 1, from_float(B, p)); SET_VECTOR_ELT(out, 2, from_float(hat, n));
    SET_VECTOR_ELT(out, 3, from_float(VB, per ? p : 1)); SET_VECTOR_ELT(out, 4, Rf_ScalarReal(ve)); SET_VECTOR_ELT(out, 5, Rf_ScalarReal(h2));
    SET_VECTOR_ELT(out, 6, Rf_ScalarReal(MSx));
  } else if (m == BWGR_BAYESB || m == BWGR_BAYESC) {
    const char *nm[] = {"mu", "b", "d", "hat", "vb", "ve", "h2", "MSx"};
    out = PROTECT(named_list(8, nm));
    SET_VECTOR_ELT(out, 0, Rf_ScalarReal(mu)); SET_VECTOR_ELT(out, 1, from_float(B, p)); SET_VECTOR_ELT(out, 2, from_float(D, p));
    SET_VECTOR_ELT(out, 3, from_float(hat, n)); SET_VECTOR_ELT(out, 4, from_float(VB, per ? p : 1)); SET_VECTOR_ELT(out, 5, Rf_ScalarReal(ve));
    SET_VECTOR_ELT(out, 6, Rf_ScalarReal(h2)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(MSx));
  } else {
    const char *nm[] = {"mu", "b", "d", "pi", "hat", "h2", "vb", "ve", "PVAL"};
    out = PROTECT(named_list(9, nm));
    SET_VECTOR_ELT(out, 0, Rf_ScalarReal(mu)); SET_VECTOR_ELT(out, 1, from_float(B, p)); SET_VECTOR_ELT(out, 2, from_float(D, p));
    SET_VECTOR_ELT(out, 3, Rf_ScalarReal(Pi)); SET_VECTOR_ELT(out, 4, from_float(hat, n)); SET_VECTOR_ELT(out, 5, Rf_ScalarReal(h2));
    SET_VECTOR_ELT(out, 6, from_float(VB, per ? p : 1)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(ve)); SET_VECTOR_ELT(out, 8, from_float(PV, p));
  }
  UNPROTECT(1);
  return out;
}

/* BayesA2 / BayesB2 / BayesRR2(y,X1,X2,it,bi,[pi,]df,R2)  src/Rcpp20260726ai.cpp:990-1218; return lists :1054-1057,
 * :1146-1149, :1216-1219 (names and order kept) */
SEXP bwgrhip_Bayes2(SEXP model, SEXP y, SEXP panel1, SEXP panel2, SEXP it, SEXP bi, SEXP pi, SEXP df, SEXP R2) {
  bwgr_panel *P1 = panel_of(panel1), *P2 = panel_of(panel2);
  int64_t i1[8], i2[8]; chk(bwgr_panel_info(P1, i1)); chk(bwgr_panel_info(P2, i2));
  const R_xlen_t n = i1[0], p1 = i1[1], p2 = i2[1];
  const int m = Rf_asInteger(model);
  if (XLENGTH(y) != n || i2[0] != i1[0]) Rf_error("length(y), nrow(X1) and nrow(X2) must agree");
  const int per = (m != BWGR_BAYESRR);
  float *fy = to_float(y, n);
  float *B1 = (float *)R_alloc(p1, 4), *D1 = (float *)R_alloc(p1, 4), *V1 = (float *)R_alloc(per ? p1 : 1, 4);
  float *B2 = (float *)R_alloc(p2, 4), *D2 = (float *)R_alloc(p2, 4), *V2 = (float *)R_alloc(per ? p2 : 1, 4), *hat = (float *)R_alloc(n, 4);
  float mu, ve, h2;
  chk(bwgr_bayes2(P1, P2, m, fy, (float)Rf_asReal(it), (float)Rf_asReal(bi), (float)Rf_asReal(pi), (float)Rf_asReal(df), (float)Rf_asReal(R2),
                  seed_from_R(), BWGR_RNG_PHILOX, &mu, B1, D1, V1, B2, D2, V2, &ve, hat, &h2));
  SEXP out;
  if (m == BWGR_BAYESB) {
    const char *nm[] = {"mu", "b1", "d1", "vb1", "b2", "d2", "vb2", "ve", "hat", "h2"};
    out = PROTECT(named_list(10, nm));
    SET_VECTOR_ELT(out, 0, Rf_ScalarReal(mu)); SET_VECTOR_ELT(out, 1, from_float(B1, p1)); SET_VECTOR_ELT(out, 2, from_float(D1, p1));
    SET_VECTOR_ELT(out, 3, from_float(V1, p1)); SET_VECTOR_ELT(out, 4, from_float(B2, p2)); SET_VECTOR_ELT(out, 5, from_float(D2, p2));
    SET_VECTOR_ELT(out, 6, from_float(V2, p2)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(ve)); SET_VECTOR_ELT(out, 8, from_float(hat, n));
    SET_VECTOR_ELT(out, 9, Rf_ScalarReal(h2));
  } else {
    const char *nm[] = {"hat", "mu", "b1", "b2", "vb1", "vb2", "ve", "h2"};
    out = PROTECT(named_list(8, nm));
    SET_VECTOR_ELT(out, 0, from_float(hat, n)); SET_VECTOR_ELT(out, 1, Rf_ScalarReal(mu)); SET_VECTOR_ELT(out, 2, from_float(B1, p1));
    SET_VECTOR_ELT(out, 3, from_float(B2, p2)); SET_VECTOR_ELT(out, 4, from_float(V1, per ? p1 : 1)); SET_VECTOR_ELT(out, 5, from_float(V2, per ? p2 : 1));
    SET_VECTOR_ELT(out, 6, Rf_ScalarReal(ve)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(h2));
  }
  UNPROTECT(1);
  return out;
}

/* EM / Gauss-Seidel family: emRR, emBA, emBB, emBC, emBCpi, emDE, emBL, emEN, emML  src/Rcpp20260726ai.cpp:80-521, :1502-1550;
 * return lists :122-127, :181-187, :240-247, :298-304, :347-353, :394, :453-459, :514-520, :1545-1549 (names and order kept).
 * model = BWGR_EM_*; par = Pi or alpha; D = emML's weights or NULL */
SEXP bwgrhip_em(SEXP model, SEXP y, SEXP panel, SEXP df, SEXP R2, SEXP par, SEXP D) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  const int m = Rf_asInteger(model);
  if (XLENGTH(y) != n) Rf_error("length(y) must equal nrow(gen)");
  float *fy = to_float(y, n), *fD = Rf_isNull(D) ? NULL : to_float(D, p);
  float *B = (float *)R_alloc(p, 4), *Dv = (float *)R_alloc(p, 4), *V = (float *)R_alloc(p, 4), *hat = (float *)R_alloc(n, 4);
  float mu, s[6]; int iters;
  chk(bwgr_em(P, m, fy, (float)Rf_asReal(df), (float)Rf_asReal(R2), (float)Rf_asReal(par), fD, 0, &mu, B, Dv, hat, V, s, &iters));
  SEXP out;
#define EM_SET(k_, v_) SET_VECTOR_ELT(out, k_, v_)
  if (m == BWGR_EM_RR) {
    const char *nm[] = {"mu", "b", "hat", "Va", "Ve", "h2"}; out = PROTECT(named_list(6, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, from_float(hat, n)); EM_SET(3, Rf_ScalarReal(s[0])); EM_SET(4, Rf_ScalarReal(s[1])); EM_SET(5, Rf_ScalarReal(s[2]));
  } else if (m == BWGR_EM_BA || m == BWGR_EM_DE) {
    const char *nm[] = {"mu", "b", "hat", "Vb", "Ve", "h2"}; out = PROTECT(named_list(6, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, from_float(hat, n)); EM_SET(3, from_float(V, p)); EM_SET(4, Rf_ScalarReal(s[1])); EM_SET(5, Rf_ScalarReal(s[2]));
  } else if (m == BWGR_EM_BB) {
    const char *nm[] = {"mu", "b", "d", "hat", "Vb", "Ve", "h2"}; out = PROTECT(named_list(7, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, from_float(Dv, p)); EM_SET(3, from_float(hat, n)); EM_SET(4, from_float(V, p)); EM_SET(5, Rf_ScalarReal(s[1])); EM_SET(6, Rf_ScalarReal(s[2]));
  } else if (m == BWGR_EM_BC) {
    const char *nm[] = {"mu", "b", "d", "hat", "Vg", "Va", "Ve", "h2"}; out = PROTECT(named_list(8, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, from_float(Dv, p)); EM_SET(3, from_float(hat, n)); EM_SET(4, Rf_ScalarReal(s[3])); EM_SET(5, Rf_ScalarReal(s[0])); EM_SET(6, Rf_ScalarReal(s[1])); EM_SET(7, Rf_ScalarReal(s[2]));
  } else if (m == BWGR_EM_BCPI) {
    const char *nm[] = {"mu", "b", "d", "pi", "hat", "Vg", "Va", "Ve", "h2"}; out = PROTECT(named_list(9, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, from_float(Dv, p)); EM_SET(3, Rf_ScalarReal(s[4])); EM_SET(4, from_float(hat, n)); EM_SET(5, Rf_ScalarReal(s[3])); EM_SET(6, Rf_ScalarReal(s[0])); EM_SET(7, Rf_ScalarReal(s[1])); EM_SET(8, Rf_ScalarReal(s[2]));
  } else if (m == BWGR_EM_BL) {
    const char *nm[] = {"mu", "b", "hat", "h2"}; out = PROTECT(named_list(4, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, from_float(hat, n)); EM_SET(3, Rf_ScalarReal(s[2]));
  } else if (m == BWGR_EM_LASSO) {
    const char *nm[] = {"mu", "b", "h2", "hat", "Lmb"}; out = PROTECT(named_list(5, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, Rf_ScalarReal(s[2])); EM_SET(3, from_float(hat, n)); EM_SET(4, Rf_ScalarReal(s[0]));
  } else if (m == BWGR_EM_EN) {
    const char *nm[] = {"mu", "b", "hat", "Va", "Ve", "h2"}; out = PROTECT(named_list(6, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, from_float(hat, n)); EM_SET(3, Rf_ScalarReal(s[0])); EM_SET(4, Rf_ScalarReal(s[1])); EM_SET(5, Rf_ScalarReal(s[2]));
  } else {
    const char *nm[] = {"mu", "b", "hat", "h2", "Vb", "Va", "Ve"}; out = PROTECT(named_list(7, nm));
    EM_SET(0, Rf_ScalarReal(mu)); EM_SET(1, from_float(B, p)); EM_SET(2, from_float(hat, n)); EM_SET(3, Rf_ScalarReal(s[2])); EM_SET(4, Rf_ScalarReal(s[0])); EM_SET(5, Rf_ScalarReal(s[3])); EM_SET(6, Rf_ScalarReal(s[1]));
  }
#undef EM_SET
  UNPROTECT(1);
  return out;
}

/* wgr(y,X,it,bi,th,bag=1,rp=FALSE,iv,de,pi,df,R2,eigK=NULL)    R/wgr.R:2-169 -> list(mu,b,Vb,d,Ve,hat,cxx), :155-168 */
SEXP bwgrhip_wgr(SEXP y, SEXP panel, SEXP it, SEXP bi, SEXP th, SEXP iv, SEXP de, SEXP pi, SEXP df, SEXP R2, SEXP U, SEXP V, SEXP bag, SEXP rp) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  if (XLENGTH(y) != n) Rf_error("length(y) must equal nrow(X)");
  const int per = Rf_asLogical(iv) || Rf_asLogical(de);
  SEXP b = PROTECT(Rf_allocVector(REALSXP, p)), d = PROTECT(Rf_allocVector(REALSXP, p)), Vb = PROTECT(Rf_allocVector(REALSXP, per ? p : 1));
  SEXP hat = PROTECT(Rf_allocMatrix(REALSXP, (int)n, 1));
  double mu, Ve, cxx, Vk = 0;
  const int has_k = !Rf_isNull(U);
  const int64_t pk = has_k ? INTEGER(Rf_getAttrib(U, R_DimSymbol))[1] : 0;
  SEXP u = PROTECT(Rf_allocMatrix(REALSXP, (int)n, 1));
  chk(bwgr_wgr_ex(P, REAL(y), Rf_asInteger(it), Rf_asInteger(bi), Rf_asInteger(th), Rf_asLogical(iv), Rf_asLogical(de), Rf_asReal(pi),
                  Rf_asReal(df), Rf_asReal(R2), seed_from_R(), BWGR_RNG_PHILOX, has_k ? REAL(U) : NULL, has_k ? REAL(V) : NULL, pk,
                  Rf_asReal(bag), Rf_asLogical(rp), &mu, REAL(b), REAL(Vb), REAL(d), &Ve, REAL(hat), &cxx, REAL(u), &Vk));
  SEXP out;
  if (has_k) {   /* list(mu,b,Vb,d,Ve,hat,u,Vk,cxx), R/wgr.R:157-160 */
    const char *nm[] = {"mu", "b", "Vb", "d", "Ve", "hat", "u", "Vk", "cxx"};
    out = PROTECT(named_list(9, nm));
    SET_VECTOR_ELT(out, 6, u); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(Vk)); SET_VECTOR_ELT(out, 8, Rf_ScalarReal(cxx));
  } else {
    const char *nm[] = {"mu", "b", "Vb", "d", "Ve", "hat", "cxx"};
    out = PROTECT(named_list(7, nm));
    SET_VECTOR_ELT(out, 6, Rf_ScalarReal(cxx));
  }
  SET_VECTOR_ELT(out, 0, Rf_ScalarReal(mu)); SET_VECTOR_ELT(out, 1, b); SET_VECTOR_ELT(out, 2, Vb); SET_VECTOR_ELT(out, 3, d);
  SET_VECTOR_ELT(out, 4, Rf_ScalarReal(Ve)); SET_VECTOR_ELT(out, 5, hat);
  UNPROTECT(6);
  return out;
}

/* KMUP2(X,Use,b,d,xx,E,L,Ve,pi) -> list(b=,d=,e=)     src/Rcpp20260726ai.cpp:41-77; Use holds 0-based row ids (R/wgr.R:68) */
SEXP bwgrhip_KMUP2(SEXP panel, SEXP Use, SEXP b, SEXP d, SEXP xx, SEXP E, SEXP L, SEXP Ve, SEXP pi, SEXP iter) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n0 = info[0], p = info[1], n = XLENGTH(Use);
  if (XLENGTH(b) != p || XLENGTH(d) != p || XLENGTH(xx) != p || XLENGTH(L) != p || XLENGTH(E) != n0) Rf_error("KMUP2: length mismatch");
  int *use = (int *)R_alloc((size_t)n, sizeof(int));
  const double *ud = REAL(Use);                            /* the reference takes Use as a float vector and truncates, :50 */
  for (R_xlen_t k = 0; k < n; k++) use[k] = (int)ud[k];
  float *fb = to_float(b, p), *fd = to_float(d, p), *fxx = to_float(xx, p), *fE = to_float(E, n0), *fL = to_float(L, p);
  float *fe = (float *)R_alloc((size_t)n, sizeof(float));
  chk(bwgr_kmup2(P, use, (int64_t)n, fb, fd, fxx, fE, fe, fL, (float)Rf_asReal(Ve), (float)Rf_asReal(pi), seed_from_R(), (uint32_t)Rf_asInteger(iter), BWGR_RNG_PHILOX));
  const char *nm[] = {"b", "d", "e"};
  SEXP out = PROTECT(named_list(3, nm));
  SET_VECTOR_ELT(out, 0, from_float(fb, p)); SET_VECTOR_ELT(out, 1, from_float(fd, p)); SET_VECTOR_ELT(out, 2, from_float(fe, n));
  UNPROTECT(1);
  return out;
}

/* multi-trait ridge regression: MRR3 / MRR3F(Y, X, maxit, tol, ...)  src/RcppEigen20230423.cpp:318-700, :704-1080 (R/mix.R:1271-1273:
 * mrr, mrr_float) -> list(mu, b, hat, h2, GC, vb, ve, MSx, cnvB, cnvH2, cnvV, b_Weights, Its), :1066-1078.  Y: numeric n x k matrix, NA =
 * missing; opts: the BWGR_MRR_* values in order (bwgr_hip.R builds them from the reference's arguments).  MRR3F's float inputs are
 * rounded by the R front-end; the engine is the same. */
static SEXP mrr_call(SEXP Y, SEXP panel, SEXP opts) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  SEXP dim = Rf_getAttrib(Y, R_DimSymbol);
  if (Rf_length(dim) != 2 || INTEGER(dim)[0] != n) Rf_error("Y must be a matrix with nrow(X) rows");
  const int k = INTEGER(dim)[1], nopts = (int)XLENGTH(opts), maxit = (int)REAL(opts)[BWGR_MRR_MAXIT];
  SEXP mu = PROTECT(Rf_allocVector(REALSXP, k)), b = PROTECT(Rf_allocMatrix(REALSXP, (int)p, k)), hat = PROTECT(Rf_allocMatrix(REALSXP, (int)n, k));
  SEXP h2 = PROTECT(Rf_allocVector(REALSXP, k)), GC = PROTECT(Rf_allocMatrix(REALSXP, k, k)), vb = PROTECT(Rf_allocMatrix(REALSXP, k, k));
  SEXP ve = PROTECT(Rf_allocVector(REALSXP, k)), MSx = PROTECT(Rf_allocVector(REALSXP, k)), W = PROTECT(Rf_allocMatrix(REALSXP, (int)p, k));
  double *c1 = (double *)R_alloc(maxit > 0 ? maxit : 1, sizeof(double)), *c2 = (double *)R_alloc(maxit > 0 ? maxit : 1, sizeof(double));
  double *c3 = (double *)R_alloc(maxit > 0 ? maxit : 1, sizeof(double));
  int its = 0;
  chk(bwgr_mrr(P, REAL(Y), k,   /* R's NA is a NaN: both mark a missing value */
                REAL(opts), nopts, REAL(mu), REAL(b), REAL(hat), REAL(h2), REAL(GC), REAL(vb), REAL(ve), REAL(MSx), c1, c2, c3, &its));
  SEXP cB = PROTECT(Rf_allocVector(REALSXP, its)), cH = PROTECT(Rf_allocVector(REALSXP, its)), cV = PROTECT(Rf_allocVector(REALSXP, its));
  for (int i = 0; i < its; i++) { REAL(cB)[i] = c1[i]; REAL(cH)[i] = c2[i]; REAL(cV)[i] = c3[i]; }
  for (R_xlen_t i = 0; i < p * k; i++) REAL(W)[i] = 1.0;                                /* b_Weights: no non-linear factor */
  const char *nm[] = {"mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV", "b_Weights", "Its"};
  SEXP out = PROTECT(named_list(13, nm));
  SEXP v[] = {mu, b, hat, h2, GC, vb, ve, MSx, cB, cH, cV, W};
  for (int i = 0; i < 12; i++) SET_VECTOR_ELT(out, i, v[i]);
  SET_VECTOR_ELT(out, 12, Rf_ScalarReal((double)its));
  UNPROTECT(13);
  return out;
}
SEXP bwgrhip_MRR3(SEXP Y, SEXP panel, SEXP opts) { return mrr_call(Y, panel, opts); }
SEXP bwgrhip_MRR3F(SEXP Y, SEXP panel, SEXP opts) { return mrr_call(Y, panel, opts); }

/* mkr(Y, K, ...) = MRR3(Y, K2X(K), ...)  R/mix.R:1275: MRR3's list on a dense design.  X: the numeric n x r matrix K2X (bwgr_hip.R) made of K,
 * or any real-valued design; Y and opts as for MRR3.  One call of bwgr_mrr_dense on device 0. */
SEXP bwgrhip_mrr_dense(SEXP Y, SEXP X, SEXP opts) {
  SEXP dx = Rf_getAttrib(X, R_DimSymbol), dim = Rf_getAttrib(Y, R_DimSymbol);
  if (Rf_length(dx) != 2 || Rf_length(dim) != 2 || INTEGER(dim)[0] != INTEGER(dx)[0]) Rf_error("Y and X must be matrices with the same number of rows");
  const int n = INTEGER(dx)[0], r = INTEGER(dx)[1], k = INTEGER(dim)[1], nopts = (int)XLENGTH(opts), maxit = (int)REAL(opts)[BWGR_MRR_MAXIT];
  const int rr = r > 0 ? r : 1;
  SEXP mu = PROTECT(Rf_allocVector(REALSXP, k)), b = PROTECT(Rf_allocMatrix(REALSXP, rr, k)), hat = PROTECT(Rf_allocMatrix(REALSXP, n, k));
  SEXP h2 = PROTECT(Rf_allocVector(REALSXP, k)), GC = PROTECT(Rf_allocMatrix(REALSXP, k, k)), vb = PROTECT(Rf_allocMatrix(REALSXP, k, k));
  SEXP ve = PROTECT(Rf_allocVector(REALSXP, k)), MSx = PROTECT(Rf_allocVector(REALSXP, k)), W = PROTECT(Rf_allocMatrix(REALSXP, rr, k));
  double *c1 = (double *)R_alloc(maxit > 0 ? maxit : 1, sizeof(double)), *c2 = (double *)R_alloc(maxit > 0 ? maxit : 1, sizeof(double));
  double *c3 = (double *)R_alloc(maxit > 0 ? maxit : 1, sizeof(double));
  int its = 0;
  chk(bwgr_mrr_dense(0, REAL(X), BWGR_HOST, (int64_t)n, (int64_t)r, (int64_t)n, REAL(Y), k, REAL(opts), nopts, REAL(mu), REAL(b), REAL(hat), REAL(h2),
                     REAL(GC), REAL(vb), REAL(ve), REAL(MSx), c1, c2, c3, &its));
  SEXP cB = PROTECT(Rf_allocVector(REALSXP, its)), cH = PROTECT(Rf_allocVector(REALSXP, its)), cV = PROTECT(Rf_allocVector(REALSXP, its));
  for (int i = 0; i < its; i++) { REAL(cB)[i] = c1[i]; REAL(cH)[i] = c2[i]; REAL(cV)[i] = c3[i]; }
  for (R_xlen_t i = 0; i < (R_xlen_t)rr * k; i++) REAL(W)[i] = 1.0;                     /* b_Weights: no non-linear factor */
  const char *nm[] = {"mu", "b", "hat", "h2", "GC", "vb", "ve", "MSx", "cnvB", "cnvH2", "cnvV", "b_Weights", "Its"};
  SEXP out = PROTECT(named_list(13, nm));
  SEXP v[] = {mu, b, hat, h2, GC, vb, ve, MSx, cB, cH, cV, W};
  for (int i = 0; i < 12; i++) SET_VECTOR_ELT(out, i, v[i]);
  SET_VECTOR_ELT(out, 12, Rf_ScalarReal((double)its));
  UNPROTECT(13);
  return out;
}

/* per-trait ridge fits: solver1x / solver1xF(Y, X, maxit, tol, df0) src/RcppEigen20230423.cpp:1410-1443, :1613-1646 -> the p effects;
 * UVBETA / FUVBETA / XFUVBETA(Y, X) :1506-1515, :1709-1753 -> p x k; ZFUVBETA(Y, X) :1807-1816 -> (p + 2) x k, rows 1 - ve / vy, mu, b.
 * variant: BWGR_UVB_*.  Y: NA = missing (solver1x: those rows are left out).  The float variants' inputs are rounded by the R front-end. */
SEXP bwgrhip_solver1x(SEXP Y, SEXP panel, SEXP variant, SEXP maxit, SEXP tol, SEXP df0) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  if (XLENGTH(Y) != n) Rf_error("Y must have nrow(X) entries");
  SEXP b = PROTECT(Rf_allocVector(REALSXP, p));
  int its = 0;
  chk(bwgr_uvbeta(P, REAL(Y), 1, Rf_asInteger(variant), Rf_asInteger(maxit), Rf_asReal(tol), Rf_asReal(df0), REAL(b), NULL, NULL, NULL, NULL, &its, NULL, NULL));
  UNPROTECT(1);
  return b;
}
SEXP bwgrhip_UVBETA(SEXP Y, SEXP panel, SEXP variant) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  SEXP dim = Rf_getAttrib(Y, R_DimSymbol);
  if (Rf_length(dim) != 2 || INTEGER(dim)[0] != n) Rf_error("Y must be a matrix with nrow(X) rows");
  const int k = INTEGER(dim)[1], v = Rf_asInteger(variant);
  const float tol = 10e-7f, df0 = 20.0f;                      /* the float solvers' arguments, as they receive them (:1614, :1723, :1772) */
  double *b = (double *)R_alloc((size_t)p * (k > 0 ? k : 1), sizeof(double)), *mu = (double *)R_alloc(k > 0 ? k : 1, sizeof(double));
  double *h2 = (double *)R_alloc(k > 0 ? k : 1, sizeof(double));
  int *its = (int *)R_alloc(k > 0 ? k : 1, sizeof(int));
  chk(bwgr_uvbeta(P, REAL(Y), k, v, 100, v == BWGR_UVB_D ? 10e-7 : (double)tol, (double)df0, b, mu, h2, NULL, NULL, its, NULL, NULL));
  const int head = v == BWGR_UVB_Z ? 2 : 0;
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)p + head, k));
  for (int t = 0; t < k; t++) {
    double *o = REAL(out) + (size_t)t * (p + head);
    if (head) { o[0] = h2[t]; o[1] = mu[t]; }
    for (R_xlen_t j = 0; j < p; j++) o[head + j] = b[(size_t)t * p + j];
  }
  UNPROTECT(1);
  return out;
}

/* the pieces of XSEMF / ZSEMF / YSEMF(Y, X, npc) src/RcppEigen20230423.cpp:1756-1769, :1819-1874, which bwgr_hip.R composes with base R's svd():
 * the per-trait fits on a dense latent design Z (n x q numeric) -> list(b = q x k, mu, h2), and X %*% B on the panel's integer genotypes.
 * variant: BWGR_UVB_*; Y: NA = missing, already float-rounded by the R front-end (once: the later stages run on unrounded doubles). */
SEXP bwgrhip_uvbeta_dense(SEXP Y, SEXP Z, SEXP variant, SEXP maxit, SEXP tol, SEXP df0) {
  SEXP dz = Rf_getAttrib(Z, R_DimSymbol), dy = Rf_getAttrib(Y, R_DimSymbol);
  if (Rf_length(dz) != 2 || Rf_length(dy) != 2 || INTEGER(dy)[0] != INTEGER(dz)[0]) Rf_error("Y and Z must be matrices with the same number of rows");
  const int n = INTEGER(dz)[0], q = INTEGER(dz)[1], k = INTEGER(dy)[1];
  SEXP b = PROTECT(Rf_allocMatrix(REALSXP, q, k)), mu = PROTECT(Rf_allocVector(REALSXP, k)), h2 = PROTECT(Rf_allocVector(REALSXP, k));
  int *its = (int *)R_alloc(k > 0 ? k : 1, sizeof(int));
  chk(bwgr_uvbeta_dense(0, REAL(Z), (int64_t)n, (int64_t)q, (int64_t)n, REAL(Y), (int64_t)k, Rf_asInteger(variant), Rf_asInteger(maxit), Rf_asReal(tol),
                        Rf_asReal(df0), REAL(b), REAL(mu), REAL(h2), NULL, NULL, its, NULL));
  const char *nm[] = {"b", "mu", "h2"};
  SEXP out = PROTECT(named_list(3, nm));
  SET_VECTOR_ELT(out, 0, b); SET_VECTOR_ELT(out, 1, mu); SET_VECTOR_ELT(out, 2, h2);
  UNPROTECT(4);
  return out;
}
SEXP bwgrhip_panel_xb(SEXP panel, SEXP B) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  SEXP dim = Rf_getAttrib(B, R_DimSymbol);
  if (Rf_length(dim) != 2 || INTEGER(dim)[0] != p) Rf_error("B must be a matrix with ncol(X) rows");
  const int k = INTEGER(dim)[1];
  SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)n, k));
  chk(bwgr_panel_xb(P, REAL(B), (int64_t)k, REAL(out)));
  UNPROTECT(1);
  return out;
}

/* solver2x(Y, X1, X2, maxit, tol, df0) src/RcppEigen20230423.cpp:1446-1493 for every column of Y, as MEGA (:1542-1579) and GSEM (:1582-1610) call it:
 * X1 = Z, a dense n x q numeric design, X2 = the panel; doubles throughout.  Y: NA = missing -> list(b1 = q x k, b2 = p x k, mu). */
SEXP bwgrhip_uvbeta2(SEXP Y, SEXP Z, SEXP panel, SEXP maxit, SEXP tol, SEXP df0) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const R_xlen_t n = info[0], p = info[1];
  SEXP dz = Rf_getAttrib(Z, R_DimSymbol), dy = Rf_getAttrib(Y, R_DimSymbol);
  if (Rf_length(dz) != 2 || Rf_length(dy) != 2 || INTEGER(dy)[0] != n || INTEGER(dz)[0] != n) Rf_error("Y and Z must be matrices with nrow(X) rows");
  const int q = INTEGER(dz)[1], k = INTEGER(dy)[1];
  SEXP b1 = PROTECT(Rf_allocMatrix(REALSXP, q, k)), b2 = PROTECT(Rf_allocMatrix(REALSXP, (int)p, k)), mu = PROTECT(Rf_allocVector(REALSXP, k));
  int *its = (int *)R_alloc(k > 0 ? k : 1, sizeof(int));
  chk(bwgr_uvbeta2(P, REAL(Z), (int64_t)q, (int64_t)n, REAL(Y), (int64_t)k, Rf_asInteger(maxit), Rf_asReal(tol), Rf_asReal(df0), REAL(b1), REAL(b2), REAL(mu),
                   NULL, NULL, NULL, NULL, its, NULL));
  const char *nm[] = {"b1", "b2", "mu"};
  SEXP out = PROTECT(named_list(3, nm));
  SET_VECTOR_ELT(out, 0, b1); SET_VECTOR_ELT(out, 1, b2); SET_VECTOR_ELT(out, 2, mu);
  UNPROTECT(4);
  return out;
}

/* PEGS(Y, X, ...) / PEGSZ(Y, X_list, maxit, logtol, covbend, covMinEv, XFA, NNC) src/RcppEigenX20251203.cpp:10-194, :576-808 ->
 * list(mu, b, hat, h2, GC, bend, numit, cnv); for PEGSZ b and GC are lists with one entry per effect and bend a vector (bwgr_hip.R unwraps
 * them for PEGS).  The effects are put into a set one by one -- a panel (the int8 genotypes, not centred), a dense numeric n x q matrix or a
 * sparse one (a dgCMatrix's @i, @p, @x and @Dim as plain vectors: no S4 accessor is needed here) -- and the set is fitted in one call;
 * bwgr_hip.R keeps the panels, matrices and vectors alive meanwhile.  Y: float-rounded by the R front-end, NA = missing.  text: 0 PEGSZ's,
 * 1 PEGS's own (PEGS_sparse is text 1 on a sparse effect), 2 PEGSZ_sparse's (:811-1007, :1010-1250; include/bwgr.h). */
#include <stdlib.h>
typedef struct { int neff; bwgr_pegs_effect_ex *e; int *cols, *rows; int64_t **ptr; } pegs_set;   /* ptr[i]: a sparse effect's @p as int64, owned */
static void pegs_set_free(pegs_set *S) {
  if (!S) return;
  if (S->ptr) for (int i = 0; i < S->neff; i++) free(S->ptr[i]);
  free(S->e); free(S->cols); free(S->rows); free(S->ptr); free(S);
}
static void pegs_set_finalizer(SEXP ext) {
  pegs_set *S = (pegs_set *)R_ExternalPtrAddr(ext);
  if (S) { pegs_set_free(S); R_ClearExternalPtr(ext); }
}
SEXP bwgrhip_pegs_set(SEXP neff) {
  const int m = Rf_asInteger(neff);
  if (m < 1) Rf_error("X_list holds no effects");
  pegs_set *S = (pegs_set *)calloc(1, sizeof(pegs_set));
  if (S) {
    S->neff = m; S->e = (bwgr_pegs_effect_ex *)calloc((size_t)m, sizeof(bwgr_pegs_effect_ex)); S->cols = (int *)calloc((size_t)m, sizeof(int));
    S->rows = (int *)calloc((size_t)m, sizeof(int)); S->ptr = (int64_t **)calloc((size_t)m, sizeof(int64_t *));
  }
  if (!S || !S->e || !S->cols || !S->rows || !S->ptr) { pegs_set_free(S); Rf_error("out of memory"); }
  SEXP ext = PROTECT(R_MakeExternalPtr(S, R_NilValue, R_NilValue));
  R_RegisterCFinalizerEx(ext, pegs_set_finalizer, TRUE);
  UNPROTECT(1);
  return ext;
}
SEXP bwgrhip_pegs_put(SEXP set, SEXP index, SEXP panel, SEXP Z) {
  pegs_set *S = (pegs_set *)R_ExternalPtrAddr(set);
  const int i = Rf_asInteger(index);
  if (!S || i < 0 || i >= S->neff) Rf_error("bad effect set or index");
  free(S->ptr[i]); S->ptr[i] = NULL;
  S->e[i].colptr = NULL; S->e[i].rowidx = NULL; S->e[i].val = NULL; S->e[i].flags = 0;
  if (!Rf_isNull(panel)) {
    bwgr_panel *P = panel_of(panel);
    int64_t info[8]; chk(bwgr_panel_info(P, info));
    S->e[i].panel = P; S->e[i].Z = NULL; S->e[i].q = 0; S->e[i].ldz = 0; S->cols[i] = (int)info[1]; S->rows[i] = (int)info[0];
  } else {
    SEXP dz = Rf_getAttrib(Z, R_DimSymbol);
    if (TYPEOF(Z) != REALSXP || Rf_length(dz) != 2) Rf_error("a dense effect must be a numeric matrix");
    S->e[i].panel = NULL; S->e[i].Z = REAL(Z); S->e[i].q = INTEGER(dz)[1]; S->e[i].ldz = INTEGER(dz)[0]; S->cols[i] = INTEGER(dz)[1]; S->rows[i] = INTEGER(dz)[0];
  }
  return R_NilValue;
}
/* a sparse effect: the slots of a dgCMatrix -- ri = @i (0-based rows, integer), cp = @p (integer, ncol + 1), x = @x (double, float-rounded by
 * the R front-end), dim = @Dim.  @i and @x are read where they are; @p is widened to the library's int64 and kept with the set. */
SEXP bwgrhip_pegs_put_sparse(SEXP set, SEXP index, SEXP ri, SEXP cp, SEXP x, SEXP dim) {
  pegs_set *S = (pegs_set *)R_ExternalPtrAddr(set);
  const int i = Rf_asInteger(index);
  if (!S || i < 0 || i >= S->neff) Rf_error("bad effect set or index");
  if (TYPEOF(ri) != INTSXP || TYPEOF(cp) != INTSXP || TYPEOF(x) != REALSXP || TYPEOF(dim) != INTSXP || Rf_length(dim) != 2)
    Rf_error("a sparse effect needs integer @i, @p and @Dim and double @x");
  const int n = INTEGER(dim)[0], q = INTEGER(dim)[1];
  if (q < 1 || Rf_length(cp) != q + 1 || Rf_length(ri) != Rf_length(x) || INTEGER(cp)[q] > Rf_length(x)) Rf_error("a sparse effect's @p, @i and @x do not describe its @Dim");
  int64_t *p64 = (int64_t *)malloc(((size_t)q + 1) * sizeof(int64_t));
  if (!p64) Rf_error("out of memory");
  for (int j = 0; j <= q; j++) p64[j] = INTEGER(cp)[j];
  free(S->ptr[i]); S->ptr[i] = p64;
  S->e[i].panel = NULL; S->e[i].Z = NULL; S->e[i].q = q; S->e[i].ldz = 0;
  S->e[i].colptr = p64; S->e[i].rowidx = (const int32_t *)INTEGER(ri); S->e[i].val = REAL(x); S->e[i].flags = 0;
  S->cols[i] = q; S->rows[i] = n;
  return R_NilValue;
}
SEXP bwgrhip_pegs(SEXP set, SEXP Y, SEXP maxit, SEXP logtol, SEXP covbend, SEXP covMinEv, SEXP XFA, SEXP NNC, SEXP text) {
  pegs_set *S = (pegs_set *)R_ExternalPtrAddr(set);
  if (!S) Rf_error("bad effect set");
  SEXP dy = Rf_getAttrib(Y, R_DimSymbol);
  if (Rf_length(dy) != 2) Rf_error("Y must be a matrix");
  const int n = INTEGER(dy)[0], k = INTEGER(dy)[1], m = S->neff, mit = Rf_asInteger(maxit);
  for (int i = 0; i < m; i++)
    if ((!S->e[i].panel && !S->e[i].Z && !S->e[i].colptr) || S->rows[i] != n) Rf_error("every effect must be set and have nrow(Y) rows");
  SEXP mu = PROTECT(Rf_allocVector(REALSXP, k)), hat = PROTECT(Rf_allocMatrix(REALSXP, n, k)), h2 = PROTECT(Rf_allocVector(REALSXP, k));
  SEXP bend = PROTECT(Rf_allocVector(REALSXP, m)), bl = PROTECT(Rf_allocVector(VECSXP, m)), gl = PROTECT(Rf_allocVector(VECSXP, m));
  double **bp = (double **)R_alloc((size_t)m, sizeof(double *)), **gp = (double **)R_alloc((size_t)m, sizeof(double *));
  for (int i = 0; i < m; i++) {
    SEXP b = PROTECT(Rf_allocMatrix(REALSXP, S->cols[i], k)), g = PROTECT(Rf_allocMatrix(REALSXP, k, k));
    SET_VECTOR_ELT(bl, i, b); SET_VECTOR_ELT(gl, i, g);
    bp[i] = REAL(b); gp[i] = REAL(g);
    UNPROTECT(2);
  }
  double *cnv = (double *)R_alloc(mit > 0 ? mit : 1, sizeof(double));
  int numit = 0;
  chk(bwgr_pegs_ex(0, S->e, m, REAL(Y), (int64_t)n, k, mit, Rf_asReal(logtol), Rf_asReal(covbend), Rf_asReal(covMinEv), Rf_asInteger(XFA),
                   Rf_asLogical(NNC), Rf_asInteger(text), REAL(mu), bp, REAL(hat), REAL(h2), gp, REAL(bend), &numit, cnv));
  const char *nm[] = {"mu", "b", "hat", "h2", "GC", "bend", "numit", "cnv"};
  SEXP out = PROTECT(named_list(8, nm));
  SET_VECTOR_ELT(out, 0, mu); SET_VECTOR_ELT(out, 1, bl); SET_VECTOR_ELT(out, 2, hat); SET_VECTOR_ELT(out, 3, h2); SET_VECTOR_ELT(out, 4, gl);
  SET_VECTOR_ELT(out, 5, bend); SET_VECTOR_ELT(out, 6, Rf_ScalarReal((double)numit)); SET_VECTOR_ELT(out, 7, Rf_ScalarReal(cnv[numit > 0 ? numit - 1 : 0]));
  UNPROTECT(7);
  return out;
}

/* PEGSX(Y, X, Z_list, maxit, logtol, covbend, covMinEv, cores, verbose, df0, NNC, InnerGS, NoInv, XFA, NumXFA) src/RcppEigenX20251203.cpp:197-573
 * -> list(TrZSZ, b, u, vb_list, GC_list, ve, hat, its, cnv, bend); TrZSZ, u, vb_list and GC_list are lists with one entry per effect.  The
 * effects are a set made as for PEGSZ.  Y, X and the dense effects: float-rounded by the R front-end, NA in Y = missing.  opts: the numeric
 * vector c(maxit, logtol, covbend, covMinEv, df0, NNC, InnerGS, NoInv, XFA, NumXFA); the library refuses InnerGS and NoInv. */
SEXP bwgrhip_pegsx(SEXP set, SEXP Y, SEXP X, SEXP opts) {
  pegs_set *S = (pegs_set *)R_ExternalPtrAddr(set);
  if (!S) Rf_error("bad effect set");
  SEXP dy = Rf_getAttrib(Y, R_DimSymbol), dx = Rf_getAttrib(X, R_DimSymbol);
  if (Rf_length(dy) != 2 || Rf_length(dx) != 2 || TYPEOF(X) != REALSXP) Rf_error("Y and X must be numeric matrices");
  if (TYPEOF(opts) != REALSXP || Rf_length(opts) != 10) Rf_error("opts must hold 10 numbers");
  const double *o = REAL(opts);
  const int n = INTEGER(dy)[0], k = INTEGER(dy)[1], f = INTEGER(dx)[1], m = S->neff, mit = (int)o[0];
  if (INTEGER(dx)[0] != n) Rf_error("nrow(X) must equal nrow(Y)");
  for (int i = 0; i < m; i++)
    if ((!S->e[i].panel && !S->e[i].Z && !S->e[i].colptr) || S->rows[i] != n) Rf_error("every effect must be set and have nrow(Y) rows");
  SEXP b = PROTECT(Rf_allocMatrix(REALSXP, f, k)), ve = PROTECT(Rf_allocVector(REALSXP, k)), hat = PROTECT(Rf_allocMatrix(REALSXP, n, k));
  SEXP bend = PROTECT(Rf_allocVector(REALSXP, m)), tl = PROTECT(Rf_allocVector(VECSXP, m)), ul = PROTECT(Rf_allocVector(VECSXP, m));
  SEXP vl = PROTECT(Rf_allocVector(VECSXP, m)), gl = PROTECT(Rf_allocVector(VECSXP, m));
  double **up = (double **)R_alloc((size_t)m, sizeof(double *)), **vp = (double **)R_alloc((size_t)m, sizeof(double *));
  double **gp = (double **)R_alloc((size_t)m, sizeof(double *)), *tr = (double *)R_alloc((size_t)m * (size_t)(k > 0 ? k : 1), sizeof(double));
  for (int i = 0; i < m; i++) {
    SEXP u = PROTECT(Rf_allocMatrix(REALSXP, S->cols[i], k)), v = PROTECT(Rf_allocMatrix(REALSXP, k, k)), g = PROTECT(Rf_allocMatrix(REALSXP, k, k));
    SET_VECTOR_ELT(ul, i, u); SET_VECTOR_ELT(vl, i, v); SET_VECTOR_ELT(gl, i, g);
    up[i] = REAL(u); vp[i] = REAL(v); gp[i] = REAL(g);
    UNPROTECT(3);
  }
  double *cnv = (double *)R_alloc(mit > 0 ? mit : 1, sizeof(double));
  int its = 0;
  chk(bwgr_pegsx_ex(0, S->e, m, REAL(X), (int64_t)n, f, REAL(Y), (int64_t)n, k, mit, o[1], o[2], o[3], o[4], o[5] != 0, o[8] != 0, (int)o[9], o[6] != 0, o[7] != 0,
                 tr, REAL(b), up, vp, gp, REAL(ve), REAL(hat), &its, cnv, REAL(bend)));
  for (int i = 0; i < m; i++) {
    SEXP t = PROTECT(Rf_allocVector(REALSXP, k));
    for (int j = 0; j < k; j++) REAL(t)[j] = tr[(size_t)i * k + j];
    SET_VECTOR_ELT(tl, i, t);
    UNPROTECT(1);
  }
  const char *nm[] = {"TrZSZ", "b", "u", "vb_list", "GC_list", "ve", "hat", "its", "cnv", "bend"};
  SEXP out = PROTECT(named_list(10, nm));
  SET_VECTOR_ELT(out, 0, tl); SET_VECTOR_ELT(out, 1, b); SET_VECTOR_ELT(out, 2, ul); SET_VECTOR_ELT(out, 3, vl); SET_VECTOR_ELT(out, 4, gl);
  SET_VECTOR_ELT(out, 5, ve); SET_VECTOR_ELT(out, 6, hat); SET_VECTOR_ELT(out, 7, Rf_ScalarReal((double)its)); SET_VECTOR_ELT(out, 8, Rf_ScalarReal(cnv[its > 0 ? its - 1 : 0]));
  SET_VECTOR_ELT(out, 9, bend);
  UNPROTECT(9);
  return out;
}

/* relationship kernels: GRM(X, Code012) / GAU(X) src/Rcpp20260726ai.cpp:1338-1383, EigenARC / EigenGAU / EigenGRM(X, ., cores)
 * src/RcppEigen20230423.cpp:8-51 -> an n x n numeric matrix.  kind: BWGR_K_*; par: phi; flag: Code012 / centralizeZ / centralizeX. */
SEXP bwgrhip_kernel(SEXP panel, SEXP kind, SEXP par, SEXP flag) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const int n = (int)info[0];
  SEXP K = PROTECT(Rf_allocMatrix(REALSXP, n, n));
  chk(bwgr_panel_kernel(P, Rf_asInteger(kind), Rf_asReal(par), Rf_asInteger(flag), REAL(K), (int64_t)n, BWGR_HOST));
  UNPROTECT(1);
  return K;
}
/* the exact X X' (tcrossprod(X) on integer genotypes) as a numeric matrix: every entry is an integer below 2^53 */
SEXP bwgrhip_crossprod(SEXP panel) {
  bwgr_panel *P = panel_of(panel);
  int64_t info[8]; chk(bwgr_panel_info(P, info));
  const int n = (int)info[0];
  int64_t *g = (int64_t *)R_alloc((size_t)n * n, sizeof(int64_t));
  chk(bwgr_panel_crossprod(P, g, (int64_t)n, BWGR_HOST));
  SEXP G = PROTECT(Rf_allocMatrix(REALSXP, n, n));
  for (R_xlen_t k = 0; k < (R_xlen_t)n * n; k++) REAL(G)[k] = (double)g[k];
  UNPROTECT(1);
  return G;
}

/* founder-by-sample kernels: the K_ff and K_fs of EigenArcZ / EigenGauZ(Zfndr, Zsamp, ., cores) src/RcppEigen20230423.cpp:1877-1939 ->
 * list(Kff = n_f x n_f, Ksf = n_s x n_f): the library's row-major n_f x n_s K_fs is R's column-major t(K_fs).  kind: BWGR_KZ_*; par: phi. */
SEXP bwgrhip_kernel2(SEXP fndr, SEXP samp, SEXP kind, SEXP par) {
  bwgr_panel *Pf = panel_of(fndr), *Ps = panel_of(samp);
  int64_t info[8]; chk(bwgr_panel_info(Pf, info));
  const int nf = (int)info[0];
  chk(bwgr_panel_info(Ps, info));
  const int ns = (int)info[0];
  SEXP Kff = PROTECT(Rf_allocMatrix(REALSXP, nf, nf)), Ksf = PROTECT(Rf_allocMatrix(REALSXP, ns, nf));
  chk(bwgr_panel_kernel2(Pf, Ps, Rf_asInteger(kind), Rf_asReal(par), REAL(Kff), (int64_t)nf, REAL(Ksf), (int64_t)ns, BWGR_HOST));
  SEXP out = PROTECT(Rf_allocVector(VECSXP, 2)), nm = PROTECT(Rf_allocVector(STRSXP, 2));
  SET_VECTOR_ELT(out, 0, Kff); SET_VECTOR_ELT(out, 1, Ksf);
  SET_STRING_ELT(nm, 0, Rf_mkChar("Kff")); SET_STRING_ELT(nm, 1, Rf_mkChar("Ksf"));
  Rf_setAttrib(out, R_NamesSymbol, nm);
  UNPROTECT(4);
  return out;
}
/* the exact X_s X_f' (tcrossprod(Xs, Xf) on integer genotypes) as an n_s x n_f numeric matrix: every entry is an integer below 2^53 */
SEXP bwgrhip_crossprod2(SEXP fndr, SEXP samp) {
  bwgr_panel *Pf = panel_of(fndr), *Ps = panel_of(samp);
  int64_t info[8]; chk(bwgr_panel_info(Pf, info));
  const int nf = (int)info[0];
  chk(bwgr_panel_info(Ps, info));
  const int ns = (int)info[0];
  int64_t *g = (int64_t *)R_alloc((size_t)nf * ns, sizeof(int64_t));
  chk(bwgr_panel_crossprod2(Pf, Ps, g, (int64_t)ns, BWGR_HOST));
  SEXP G = PROTECT(Rf_allocMatrix(REALSXP, ns, nf));
  for (R_xlen_t k = 0; k < (R_xlen_t)nf * ns; k++) REAL(G)[k] = (double)g[k];
  UNPROTECT(1);
  return G;
}

static const R_CallMethodDef CallEntries[] = {   /* as src/RcppExports.cpp:1152-1228 registers _bWGR_* */
  {"bwgrhip_panel", (DL_FUNC)&bwgrhip_panel, 2}, {"bwgrhip_KMUP", (DL_FUNC)&bwgrhip_KMUP, 9}, {"bwgrhip_KMUP2", (DL_FUNC)&bwgrhip_KMUP2, 10},
  {"bwgrhip_Bayes", (DL_FUNC)&bwgrhip_Bayes, 8}, {"bwgrhip_Bayes2", (DL_FUNC)&bwgrhip_Bayes2, 9},
  {"bwgrhip_wgr", (DL_FUNC)&bwgrhip_wgr, 14}, {"bwgrhip_em", (DL_FUNC)&bwgrhip_em, 7},
  {"bwgrhip_MRR3", (DL_FUNC)&bwgrhip_MRR3, 3}, {"bwgrhip_MRR3F", (DL_FUNC)&bwgrhip_MRR3F, 3}, {"bwgrhip_mrr_dense", (DL_FUNC)&bwgrhip_mrr_dense, 3},
  {"bwgrhip_solver1x", (DL_FUNC)&bwgrhip_solver1x, 6}, {"bwgrhip_UVBETA", (DL_FUNC)&bwgrhip_UVBETA, 3},
  {"bwgrhip_uvbeta_dense", (DL_FUNC)&bwgrhip_uvbeta_dense, 6}, {"bwgrhip_panel_xb", (DL_FUNC)&bwgrhip_panel_xb, 2},
  {"bwgrhip_uvbeta2", (DL_FUNC)&bwgrhip_uvbeta2, 6},
  {"bwgrhip_pegs_set", (DL_FUNC)&bwgrhip_pegs_set, 1}, {"bwgrhip_pegs_put", (DL_FUNC)&bwgrhip_pegs_put, 4}, {"bwgrhip_pegs_put_sparse", (DL_FUNC)&bwgrhip_pegs_put_sparse, 6},
  {"bwgrhip_pegs", (DL_FUNC)&bwgrhip_pegs, 9},
  {"bwgrhip_pegsx", (DL_FUNC)&bwgrhip_pegsx, 4},
  {"bwgrhip_kernel", (DL_FUNC)&bwgrhip_kernel, 4}, {"bwgrhip_crossprod", (DL_FUNC)&bwgrhip_crossprod, 1},
  {"bwgrhip_kernel2", (DL_FUNC)&bwgrhip_kernel2, 4}, {"bwgrhip_crossprod2", (DL_FUNC)&bwgrhip_crossprod2, 2}, {NULL, NULL, 0}};

void R_init_bwgrhip(DllInfo *dll) {              /* as R_init_bWGR, src/RcppExports.cpp:1230-1233 */
  R_registerRoutines(dll, NULL, CallEntries, NULL, NULL);
  R_useDynamicSymbols(dll, FALSE);
}
