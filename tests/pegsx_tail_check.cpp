// The host work of PEGSX -- the trait set-up (bwgr_amd/csrc/pegsx_setup.h) and the new functions of bwgr_amd/csrc/pegs_tail.h -- as a program of
// its own: tests/test_pegsx_cpu.py builds it with -fsanitize=address,undefined and gives it a text file of fits dumped by
// tests/pegsx_restatement.py -- Y and X with what the set-up must make of them (n_t, the pseudo-inverse of every trait's M'M, b, the projected
// y and its sum of squares), TrZSZ and the start values, and per sweep the sums a sweep leaves (e'y, every effect's TildeHat and
// sum (delta u)^2) with what the restatement made of them.  Every value must agree to 1e-12 scaled error: vectors and matrices on the scale of
// their largest entry; eigenvalues and inflate on the scale of vb's largest eigenvalue; an inverse on the scale of its largest entry times
// the condition number of what was inverted (for M'M: over the kept eigenvalues).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../bwgr_amd/csrc/pegsx_setup.h"

using namespace bwgr;

static FILE *in;
static int fails = 0;
static double rd() {
  char tok[64];
  if (fscanf(in, "%63s", tok) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return strtod(tok, nullptr);   // (reads nan and inf too)
}
static void rdv(std::vector<double> &v, size_t m) { v.resize(m); for (size_t i = 0; i < m; ++i) v[i] = rd(); }
static double maxabs(const std::vector<double> &v) { double m = 0; for (double x : v) m = std::max(m, fabs(x)); return m; }
static void near(const char *what, int cs, int sw, const double *a, const std::vector<double> &b, double scale) {
  if (!(scale > 0)) scale = 1.0;
  for (size_t i = 0; i < b.size(); ++i)
    if (!(fabs(a[i] - b[i]) <= 1e-12 * scale)) { fprintf(stderr, "case %d sweep %d: %s[%zu] = %.17g, expected %.17g (scale %g)\n", cs, sw, what, i, a[i], b[i], scale); ++fails; return; }
}

int main(int argc, char **argv) {
  if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: pegsx_tail_check CASES\n"); return 2; }
  // the refusals, the pseudo-inverse's rank decision, the set-up's refusals
  {
    const PegsxOpts ok = {500, -8.0, 1.1, 1e-3, 1.1, false, false, 3};
    PegsxOpts o = ok;
    if (pegsx_refuses(o)) { fprintf(stderr, "defaults refused\n"); ++fails; }
    o = ok; o.maxit = -1; if (!pegsx_refuses(o)) { fprintf(stderr, "maxit < 0 accepted\n"); ++fails; }
    o = ok; o.covbend = NAN; if (!pegsx_refuses(o)) { fprintf(stderr, "covbend NaN accepted\n"); ++fails; }
    o = ok; o.covMinEv = INFINITY; if (!pegsx_refuses(o)) { fprintf(stderr, "covMinEv inf accepted\n"); ++fails; }
    o = ok; o.df0 = NAN; if (!pegsx_refuses(o)) { fprintf(stderr, "df0 NaN accepted\n"); ++fails; }
    o = ok; o.logtol = NAN; if (!pegsx_refuses(o)) { fprintf(stderr, "logtol NaN accepted\n"); ++fails; }
    o = ok; o.logtol = -INFINITY; if (pegsx_refuses(o)) { fprintf(stderr, "logtol -inf refused\n"); ++fails; }
    // [[2, 2], [2, 2 (1 + 1e-9)]]: the small eigenvalue is rounding-far from zero in fp64 and still below 2 * 2^-23 of the large one: rank 1
    const double A[4] = {2.0, 2.0, 2.0, 2.0 * (1.0 + 1e-9)};
    double P[4], rt[2];
    if (pegsx_pinv(2, A, P, rt) != 1 || !(rt[0] < 1e-9) || fabs(P[0] - 0.125) > 1e-9) { fprintf(stderr, "pegsx_pinv kept a direction below the float threshold\n"); ++fails; }
    const double I2[4] = {3.0, 0.0, 0.0, 5.0};
    if (pegsx_pinv(2, I2, P, nullptr) != 2 || fabs(P[0] - 1.0 / 3.0) > 1e-15 || fabs(P[3] - 0.2) > 1e-15) { fprintf(stderr, "pegsx_pinv of a full-rank matrix is not its inverse\n"); ++fails; }
    const double Y1[6] = {1.0, NAN, NAN, 1.0, 2.0, 3.0}, X1[3] = {1.0, 1.0, 1.0}, Xb[3] = {1.0, INFINITY, 1.0};
    if (read_fixed(Y1, X1, 3, 2, 1, 3, 128).S.bad != 0) { fprintf(stderr, "a trait with one record accepted\n"); ++fails; }
    const FixedSet Fb = read_fixed(Y1, Xb, 3, 2, 1, 3, 128);
    if (Fb.bad_row != 1 || Fb.bad_col != 0) { fprintf(stderr, "a non-finite X accepted\n"); ++fails; }
    PegsxState S; int fl = 0;
    const double nt[1] = {3}, ssy[1] = {0.0}, Tr[1] = {0.0};
    pegsx_init(S, 1, 1, 4, ok, nt, ssy, Tr, &fl);
    if (fl != (PEGSX_FL_DENOM | PEGSX_FL_VE | PEGSX_FL_TR) || S.ve[0] != 1e-8 || S.eff[0].vb[0] != 1.0) { fprintf(stderr, "the start values' floors: %d\n", fl); ++fails; }
  }
  const int ncases = (int)rd();
  for (int cs = 0; cs < ncases; ++cs) {
    const int k = (int)rd(), neff = (int)rd(), nsw = (int)rd(), f = (int)rd(), n = (int)rd(), setup = (int)rd();
    PegsxOpts o;
    o.maxit = nsw; o.logtol = rd(); o.covbend = rd(); o.covMinEv = rd(); o.df0 = rd(); o.NNC = rd() != 0; o.XFA = rd() != 0; o.NumXFA = (int)rd();
    const size_t kk = (size_t)k * k, ff = (size_t)f * f;
    std::vector<double> nt, ssy, Tr, ve0, vb0;
    rdv(nt, k); rdv(ssy, k);
    if (setup) {
      std::vector<double> Y, X, iXX, b0, y, cond;
      rdv(Y, (size_t)n * k); rdv(X, (size_t)n * f); rdv(iXX, k * ff); rdv(cond, k); rdv(b0, (size_t)f * k); rdv(y, (size_t)n * k);
      // X with a padded column stride, to walk the ldx path
      const int ldx = n + 3, ld = (n + 127) / 128 * 128;
      std::vector<double> Xp((size_t)ldx * f, NAN);
      for (int c = 0; c < f; ++c) for (int r = 0; r < n; ++r) Xp[(size_t)c * ldx + r] = X[(size_t)c * n + r];
      const FixedSet F = read_fixed(Y.data(), Xp.data(), n, k, f, ldx, ld);
      if (F.bad_row >= 0 || F.S.bad >= 0 || (int)F.pat.id.size() != k) { fprintf(stderr, "case %d: set-up refused\n", cs); ++fails; break; }
      near("nt", cs, -1, F.S.nt.data(), nt, maxabs(nt));
      near("ssy", cs, -1, F.ssy.data(), ssy, maxabs(ssy));
      near("b0", cs, -1, F.b.data(), b0, maxabs(b0) * maxabs(cond));
      double ymax = maxabs(y);
      for (int t = 0; t < k; ++t) {
        std::vector<double> one(iXX.begin() + t * ff, iXX.begin() + (t + 1) * ff), yt(y.begin() + (size_t)t * n, y.begin() + (size_t)(t + 1) * n);
        near("iXX", cs, -1, F.iXX.data() + (size_t)F.pat.id[(size_t)t] * ff, one, maxabs(one) * cond[(size_t)t]);
        near("y", cs, -1, F.S.y.data() + (size_t)t * ld, yt, ymax * maxabs(cond));
        for (int r = n; r < ld; ++r) if (F.S.y[(size_t)t * ld + r] != 0.0) { fprintf(stderr, "case %d: the padding of y is not zero\n", cs); ++fails; break; }
      }
    }
    rdv(Tr, (size_t)neff * k); rdv(ve0, k); rdv(vb0, neff * kk);
    PegsxState S; int fl0 = -1;
    pegsx_init(S, k, neff, f, o, nt.data(), ssy.data(), Tr.data(), &fl0);
    const int fl0x = (int)rd();
    if (fl0 != fl0x) { fprintf(stderr, "case %d: start floors %d, expected %d\n", cs, fl0, fl0x); ++fails; }
    near("ve0", cs, -1, S.ve.data(), ve0, maxabs(ve0));
    for (int e = 0; e < neff; ++e) {
      std::vector<double> one(vb0.begin() + e * kk, vb0.begin() + (e + 1) * kk);
      near("vb0", cs, -1, S.eff[(size_t)e].vb.data(), one, maxabs(one));
    }
    for (int sw = 0; sw < nsw; ++sw) {
      std::vector<double> ey, TH, db2, ve, vbx, iGx, one;
      rdv(ey, k); rdv(TH, neff * kk); rdv(db2, neff);
      std::vector<PegsxTrace> tr((size_t)neff);
      const bool stop = pegsx_after_sweep(S, o, ey.data(), TH.data(), db2.data(), tr.data());
      rdv(ve, k);
      const double cnv = rd(); const bool stopx = rd() != 0;
      near("ve", cs, sw, S.ve.data(), ve, maxabs(ve));
      one.assign(1, cnv); near("cnv", cs, sw, &S.cnv, one, std::max(1.0, fabs(cnv)));
      if (stop != stopx || S.numit != sw + 1) { fprintf(stderr, "case %d sweep %d: stop %d, expected %d (numit %d)\n", cs, sw, (int)stop, (int)stopx, S.numit); ++fails; }
      for (int e = 0; e < neff; ++e) {
        rdv(vbx, kk); rdv(iGx, kk);
        const double infl = rd(), mindvb = rd(), maxev = rd(); const int inflated = (int)rd(); const double gap = rd(); const int floors = (int)rd();
        const PegsxEffect &E = S.eff[(size_t)e];
        near("vb", cs, sw, E.vb.data(), vbx, maxabs(vbx));
        one.assign(1, infl); near("inflate", cs, sw, &E.inflate, one, fabs(maxev));
        one.assign(1, mindvb); near("MinDVb", cs, sw, &tr[(size_t)e].MinDVb, one, fabs(maxev));
        one.assign(1, maxev); near("maxEv", cs, sw, &tr[(size_t)e].maxEv, one, fabs(maxev));
        one.assign(1, gap); near("gap", cs, sw, &tr[(size_t)e].gap, one, 1.0);
        if (tr[(size_t)e].inflated != inflated || tr[(size_t)e].floors != floors) {
          fprintf(stderr, "case %d sweep %d effect %d: inflated %d floors %d, expected %d %d\n", cs, sw, e, tr[(size_t)e].inflated, tr[(size_t)e].floors, inflated, floors); ++fails;
        }
        std::vector<double> w(k), V(kk);
        mrr_eigh(k, E.vb.data(), w.data(), V.data());
        double lo = INFINITY, hi = 0.0;
        for (int i = 0; i < k; ++i) { lo = std::min(lo, fabs(w[i])); hi = std::max(hi, fabs(w[i])); }
        near("iG", cs, sw, E.iG.data(), iGx, maxabs(iGx) * (hi / lo));
      }
    }
    std::vector<double> GCx, GC(neff * kk);
    rdv(GCx, neff * kk);
    pegsx_finish(S, GC.data());
    near("GC", cs, nsw, GC.data(), GCx, 1.0);
  }
  fclose(in);
  if (fails) return 1;
  printf("pegsx_tail_check ok\n");
  return 0;
}
