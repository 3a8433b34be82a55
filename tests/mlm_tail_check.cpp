// The host tail of MLM (bwgr_amd/csrc/mlm_tail.h) as a program of its own: tests/test_mlm_cpu.py builds it with -fsanitize=address,undefined
// and gives it a text file of cases taken from the trace of tests/mlm_restatement.py -- the start values' inputs and results, then per sweep
// e'y, TildeHat and sum (delta b)^2 with the ve, vb, iG, inflate and cnv the restatement made of them, then h2 and GC.  Every value must agree to
// 1e-12 scaled error: vectors and matrices on the scale of their largest entry, inflate on the scale of vb's largest entry (an eigenvalue of a
// symmetric matrix is determined to rounding on the scale of the matrix), iG on the scale of its largest entry times vb's condition number.
#include <stdio.h>
#include <stdlib.h>
#include "../bwgr_amd/csrc/mlm_tail.h"

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
  if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: mlm_tail_check CASES\n"); return 2; }
  const int ncases = (int)rd();
  int raised_seen = 0;
  for (int cs = 0; cs < ncases; ++cs) {
    const int k = (int)rd(), f = (int)rd(), nsw = (int)rd();
    const double df0 = rd();
    const size_t K = (size_t)k, KK = K * K;
    std::vector<double> nt, ssy, Tr, xvy, xve, xvb, xSe, xiNp;
    rdv(nt, K); rdv(ssy, K); rdv(Tr, K); rdv(xvy, K); rdv(xve, K); rdv(xvb, KK); rdv(xSe, K); rdv(xiNp, K);
    MlmState S;
    mlm_start(S, k, f, df0, nt.data(), ssy.data(), Tr.data());
    near("start vy", cs, -1, S.vy.data(), xvy, maxabs(xvy)); near("start ve", cs, -1, S.ve.data(), xve, maxabs(xve));
    near("start vb", cs, -1, S.vb.data(), xvb, maxabs(xvb)); near("start Se", cs, -1, S.Se.data(), xSe, maxabs(xSe));
    near("start iNp", cs, -1, S.iNp.data(), xiNp, maxabs(xiNp));
    for (size_t t = 0; t < K; ++t)
      if (!(fabs(S.iG[t * K + t] * S.vb[t * K + t] - 1.0) <= 1e-12) || S.Sb[t] != S.vb[t * K + t] * df0) { fprintf(stderr, "case %d: start iG / Sb of trait %zu\n", cs, t); ++fails; }
    if (S.cnv != 10.0 || S.numit != 0 || S.inflate != 0.0) { fprintf(stderr, "case %d: start cnv / numit / inflate\n", cs); ++fails; }
    double before = 0.0;
    for (int sw = 0; sw < nsw; ++sw) {
      std::vector<double> ey, TH, wve, wvb, wiG;
      rdv(ey, K); rdv(TH, KK);
      const double db2 = rd();
      rdv(wve, K); rdv(wvb, KK); rdv(wiG, KK);
      const double winf = rd(), wcnv = rd(), cond = rd();
      const bool raised = mlm_after_sweep(S, ey.data(), TH.data(), db2);
      near("ve", cs, sw, S.ve.data(), wve, maxabs(wve));
      near("vb", cs, sw, S.vb.data(), wvb, maxabs(wvb));
      near("iG", cs, sw, S.iG.data(), wiG, maxabs(wiG) * std::max(1.0, cond));
      near("inflate", cs, sw, &S.inflate, std::vector<double>(1, winf), maxabs(wvb));
      near("cnv", cs, sw, &S.cnv, std::vector<double>(1, wcnv), std::max(1.0, fabs(wcnv)));
      if (S.inflate < before || raised != (S.inflate > before)) { fprintf(stderr, "case %d sweep %d: inflate went from %g to %g, raised = %d\n", cs, sw, before, S.inflate, (int)raised); ++fails; }
      if (S.numit != sw + 1) { fprintf(stderr, "case %d sweep %d: numit = %d\n", cs, sw, S.numit); ++fails; }
      before = S.inflate;
      raised_seen += raised;
    }
    std::vector<double> xh2, xGC, h2(K), GC(KK);
    rdv(xh2, K); rdv(xGC, KK);
    mlm_finish(S, h2.data(), GC.data());
    near("h2", cs, nsw, h2.data(), xh2, 1.0);
    near("GC", cs, nsw, GC.data(), xGC, 1.0);
  }
  fclose(in);
  if (!raised_seen) { fprintf(stderr, "no case bent\n"); ++fails; }
  if (fails) return 1;
  printf("mlm_tail_check ok\n");
  return 0;
}
