// The host tail of PEGS / PEGSZ (bwgr_amd/csrc/pegs_tail.h) as a program of its own: tests/test_pegs_cpu.py builds it with
// -fsanitize=address,undefined and gives it a text file of fits -- the start values and, per sweep, the sums a sweep leaves (e'y, sum e, every
// effect's TildeHat and sum (delta b)^2) with what tests/pegs_restatement.py made of them.  Every value must agree to 1e-12 scaled error:
// vectors and matrices on the scale of their largest entry; MinDVb, the largest eigenvalue and inflate on the scale of vb's largest eigenvalue
// (an eigenvalue of a symmetric matrix is determined to rounding on the scale of the matrix, not of itself); iG on the scale of its largest entry times
// vb's condition number (the inverse of a matrix is determined to rounding times its condition number, which reaches 1e7 for the bent matrices).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../bwgr_amd/csrc/pegs_tail.h"

using namespace bwgr;

static FILE *in;
static int fails = 0;
static double rd() { double v = 0; if (fscanf(in, "%lf", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static void rdv(std::vector<double> &v, size_t m) { v.resize(m); for (size_t i = 0; i < m; ++i) v[i] = rd(); }
static double maxabs(const std::vector<double> &v) { double m = 0; for (double x : v) m = std::max(m, fabs(x)); return m; }
static void near(const char *what, int cs, int sw, const double *a, const std::vector<double> &b, double scale) {
  if (!(scale > 0)) scale = 1.0;
  for (size_t i = 0; i < b.size(); ++i)
    if (!(fabs(a[i] - b[i]) <= 1e-12 * scale)) { fprintf(stderr, "case %d sweep %d: %s[%zu] = %.17g, expected %.17g (scale %g)\n", cs, sw, what, i, a[i], b[i], scale); ++fails; return; }
}

int main(int argc, char **argv) {
  if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: pegs_tail_check CASES\n"); return 2; }
  // the refusals
  {
    const PegsOpts ok = {100, -4.0, 1.1, 1e-3, -1, true, false};
    PegsOpts o = ok;
    if (pegs_refuses(3, o)) { fprintf(stderr, "defaults refused\n"); ++fails; }
    o = ok; o.maxit = -1; if (!pegs_refuses(3, o)) { fprintf(stderr, "maxit < 0 accepted\n"); ++fails; }
    o = ok; o.XFA = 4; if (!pegs_refuses(3, o)) { fprintf(stderr, "XFA > k accepted\n"); ++fails; }
    o = ok; o.XFA = 3; if (pegs_refuses(3, o)) { fprintf(stderr, "XFA = k refused\n"); ++fails; }
    o = ok; o.covbend = NAN; if (!pegs_refuses(3, o)) { fprintf(stderr, "covbend NaN accepted\n"); ++fails; }
    o = ok; o.covMinEv = INFINITY; if (!pegs_refuses(3, o)) { fprintf(stderr, "covMinEv inf accepted\n"); ++fails; }
    o = ok; o.logtol = NAN; if (!pegs_refuses(3, o)) { fprintf(stderr, "logtol NaN accepted\n"); ++fails; }
    o = ok; o.logtol = -INFINITY; if (pegs_refuses(3, o)) { fprintf(stderr, "logtol -inf refused\n"); ++fails; }
    PegsState S; int be = -1, bt = -1;
    const double nt[2] = {5, 6}, vy[2] = {1, 2}, mu[2] = {0, 0}, MSx[4] = {1, 2, 3, 0};
    if (pegs_init(S, 2, 2, nt, vy, mu, MSx, &be, &bt) || be != 1 || bt != 1) { fprintf(stderr, "TrXSX = 0 accepted\n"); ++fails; }
  }
  const int ncases = (int)rd();
  for (int cs = 0; cs < ncases; ++cs) {
    const int k = (int)rd(), neff = (int)rd(), nsw = (int)rd();
    PegsOpts o;
    o.maxit = nsw; o.logtol = rd(); o.covbend = rd(); o.covMinEv = rd(); o.XFA = (int)rd(); o.NNC = rd() != 0; o.own_text = rd() != 0;
    std::vector<double> nt, vy, mu, MSx;
    rdv(nt, k); rdv(vy, k); rdv(mu, k); rdv(MSx, (size_t)neff * k);
    PegsState S; int be = -1, bt = -1;
    if (pegs_refuses(k, o) || !pegs_init(S, k, neff, nt.data(), vy.data(), mu.data(), MSx.data(), &be, &bt)) { fprintf(stderr, "case %d refused\n", cs); ++fails; break; }
    const size_t kk = (size_t)k * k;
    for (int sw = 0; sw < nsw; ++sw) {
      std::vector<double> ey, TH, db2, ve, dx, mux, d(k), vbx, iGx, one;
      rdv(ey, 2 * (size_t)k); rdv(TH, neff * kk); rdv(db2, neff);
      std::vector<PegsTrace> tr((size_t)neff);
      const bool stop = pegs_after_sweep(S, o, ey.data(), TH.data(), db2.data(), d.data(), tr.data());
      rdv(ve, k); rdv(dx, k); rdv(mux, k);
      const double cnv = rd(); const bool stopx = rd() != 0;
      near("ve", cs, sw, S.ve.data(), ve, maxabs(ve));
      near("d", cs, sw, d.data(), dx, maxabs(dx));
      near("mu", cs, sw, S.mu.data(), mux, maxabs(mux));
      one.assign(1, cnv); near("cnv", cs, sw, &S.cnv, one, std::max(1.0, fabs(cnv)));
      if (stop != stopx || S.numit != sw + 1) { fprintf(stderr, "case %d sweep %d: stop %d, expected %d (numit %d)\n", cs, sw, (int)stop, (int)stopx, S.numit); ++fails; }
      for (int e = 0; e < neff; ++e) {
        rdv(vbx, kk); rdv(iGx, kk);
        const double infl = rd(), mindvb = rd(), maxev = rd(); const int inflated = (int)rd(); const double gap = rd();
        const PegsEffect &E = S.eff[(size_t)e];
        near("vb", cs, sw, E.vb.data(), vbx, maxabs(vbx));
        one.assign(1, infl); near("inflate", cs, sw, &E.inflate, one, fabs(maxev));
        one.assign(1, mindvb); near("MinDVb", cs, sw, &tr[(size_t)e].MinDVb, one, fabs(maxev));
        one.assign(1, maxev); near("maxEv", cs, sw, &tr[(size_t)e].maxEv, one, fabs(maxev));
        one.assign(1, gap); near("gap", cs, sw, &tr[(size_t)e].gap, one, 1.0);
        if (tr[(size_t)e].inflated != inflated) { fprintf(stderr, "case %d sweep %d effect %d: inflated %d, expected %d\n", cs, sw, e, tr[(size_t)e].inflated, inflated); ++fails; }
        // iG on the scale of its largest entry times vb's condition number
        std::vector<double> w(k), V(kk);
        mrr_eigh(k, E.vb.data(), w.data(), V.data());
        double lo = INFINITY, hi = 0.0;
        for (int i = 0; i < k; ++i) { lo = std::min(lo, fabs(w[i])); hi = std::max(hi, fabs(w[i])); }
        near("iG", cs, sw, E.iG.data(), iGx, maxabs(iGx) * (hi / lo));
      }
    }
    std::vector<double> h2x, GCx, h2(k), GC(neff * kk);
    rdv(h2x, k); rdv(GCx, neff * kk);
    pegs_finish(S, h2.data(), GC.data());
    near("h2", cs, nsw, h2.data(), h2x, maxabs(h2x));
    near("GC", cs, nsw, GC.data(), GCx, 1.0);
  }
  fclose(in);
  if (fails) return 1;
  printf("pegs_tail_check ok\n");
  return 0;
}
