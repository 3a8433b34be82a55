// The host tail of mrr_svd (bwgr_amd/csrc/mrr_svd_tail.h) as a program of its own: tests/test_mrr_svd_cpu.py builds it with
// -fsanitize=address,undefined and gives it a text file of cases -- the start values' inputs and, per sweep, TildeHat and TrDinvXSX with what
// tests/mrr_svd_restatement.py made of them; then a convergence triple and the correlations.  Every value must agree to 1e-12 scaled error:
// vectors and matrices on the scale of their largest entry, the smallest eigenvalue on the scale of vb's largest entry (an eigenvalue of a
// symmetric matrix is determined to rounding on the scale of the matrix), iG on the scale of its largest entry times vb's condition number.
#include <stdio.h>
#include <stdlib.h>
#include "../bwgr_amd/csrc/mrr_svd_tail.h"

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
  if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: mrr_svd_tail_check CASES\n"); return 2; }
  const int ncases = (int)rd();
  int bent_seen = 0;
  for (int cs = 0; cs < ncases; ++cs) {
    const int k = (int)rd(), nsw = (int)rd();
    const size_t K = (size_t)k, KK = K * K;
    std::vector<double> nt, vy, MSx, xve, xvb, xiG, xh2, xiN;
    rdv(nt, K); rdv(vy, K); rdv(MSx, K); rdv(xve, K); rdv(xvb, KK); rdv(xiG, KK); rdv(xh2, K); rdv(xiN, K);
    std::vector<double> ve(K), vb(KK), iG(KK), h2(K), iN(K), GC(KK);
    mrr_svd_start(k, nt.data(), vy.data(), MSx.data(), ve.data(), vb.data(), iG.data(), h2.data(), iN.data());
    near("start ve", cs, -1, ve.data(), xve, maxabs(xve)); near("start vb", cs, -1, vb.data(), xvb, maxabs(xvb));
    near("start iG", cs, -1, iG.data(), xiG, maxabs(xiG)); near("start h2", cs, -1, h2.data(), xh2, 1.0); near("start iN", cs, -1, iN.data(), xiN, maxabs(xiN));
    for (int sw = 0; sw < nsw; ++sw) {
      std::vector<double> TH, Tr, wvb, wiG;
      rdv(TH, KK); rdv(Tr, K); rdv(wvb, KK); rdv(wiG, KK);
      const int wbent = (int)rd();
      const double wlam = rd(), cond = rd();
      int bent = -1; double lam = 0;
      mrr_svd_tail_vb(k, TH.data(), Tr.data(), vb.data(), iG.data(), &bent, &lam);
      near("vb", cs, sw, vb.data(), wvb, maxabs(wvb));
      near("iG", cs, sw, iG.data(), wiG, maxabs(wiG) * std::max(1.0, cond));
      near("lam", cs, sw, &lam, std::vector<double>(1, wlam), maxabs(wvb));
      if (bent != wbent) { fprintf(stderr, "case %d sweep %d: bent = %d, expected %d\n", cs, sw, bent, wbent); ++fails; }
      bent_seen += bent;
    }
    std::vector<double> db2, h20, h2b, vb0, vb1, xc, xGC;
    rdv(db2, K); rdv(h20, K); rdv(h2b, K); rdv(vb0, KK); rdv(vb1, KK); rdv(xc, 3); rdv(xGC, KK);
    double c[3];
    mrr_svd_cnv(k, db2.data(), h20.data(), h2b.data(), vb0.data(), vb1.data(), &c[0], &c[1], &c[2]);
    near("cnv", cs, nsw, c, xc, maxabs(xc));
    mrr_svd_gc(k, vb1.data(), GC.data());
    near("GC", cs, nsw, GC.data(), xGC, 1.0);
  }
  fclose(in);
  if (!bent_seen) { fprintf(stderr, "no case bent\n"); ++fails; }
  if (fails) return 1;
  printf("mrr_svd_tail_check ok\n");
  return 0;
}
