// The host algebra of the per-trait fits (bwgr_amd/csrc/uvb_tail.h) as a program of its own: tests/test_uvb_tail_cpu.py builds it with
// -fsanitize=address,undefined and gives it a text file of fits -- a trait's start values and, per sweep, the sums a sweep leaves (sum e, e'y,
// e'e, b'b, tilde'b, sum (delta b)^2 and the dense leg's three) with what tests/uvb_restatement.py and tests/sem2_restatement.py made of them.
// uvb_start and uvb_update are replayed on it: every value must agree to 1e-9 of the restatement's (NaN and infinity where it has them), the
// sweep count and the stop decision exactly.  uvb_result and uvb_slots are checked against values written out by hand.
#include <stdio.h>
#include <stdlib.h>
#include "../bwgr_amd/csrc/uvb_tail.h"

using namespace bwgr;

static FILE *in;
static int fails = 0;
static double rd() { double v = 0; if (fscanf(in, "%lf", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }
static bool same(double got, double want) {
  if (std::isnan(want) || std::isnan(got)) return std::isnan(want) && std::isnan(got);
  if (std::isinf(want) || std::isinf(got)) return got == want;
  return fabs(got - want) <= 1e-9 * (want != 0.0 ? fabs(want) : 1.0);
}
static void near(const char *what, int cs, int sw, double got, double want) {
  if (!same(got, want)) { fprintf(stderr, "case %d sweep %d: %s = %.17g, expected %.17g\n", cs, sw, what, got, want); ++fails; }
}
static void expect(bool ok, const char *what) { if (!ok) { fprintf(stderr, "%s\n", what); ++fails; } }

static void check_result() {
  double mu[3] = {-1, -1, -1}, h2[3] = {-1, -1, -1}, ve[3] = {-1, -1, -1}, vb[3] = {-1, -1, -1}, cnv[3] = {-1, -1, -1};
  int its[3] = {-1, -1, -1};
  const UvbOut o = {mu, h2, ve, vb, cnv, its};
  uvb_result(o, 0, false, BWGR_UVB_D, 3.0, 1.0, 2.0, 4.0, -6.5, 7);
  uvb_result(o, 1, true, BWGR_UVB_D, 3.0, NAN, NAN, 0.0, NAN, 0);      // a trait with no rows
  uvb_result(o, 2, false, BWGR_UVB_X, 3.0, NAN, NAN, 4.0, -6.5, 7);    // xsolver1xF estimates no variance
  expect(mu[0] == 3.0 && h2[0] == 0.75 && ve[0] == 1.0 && vb[0] == 2.0 && cnv[0] == -6.5 && its[0] == 7, "uvb_result: a trait that ran");
  expect(mu[1] == 0.0 && h2[1] == 0.0 && std::isnan(ve[1]) && std::isnan(vb[1]) && std::isnan(cnv[1]) && its[1] == 0, "uvb_result: a trait with no rows");
  expect(mu[2] == 3.0 && std::isnan(h2[2]) && std::isnan(ve[2]) && std::isnan(vb[2]) && cnv[2] == -6.5 && its[2] == 7, "uvb_result: variant X");
  const UvbOut only_its = {nullptr, nullptr, nullptr, nullptr, nullptr, its};
  uvb_result(only_its, 0, false, BWGR_UVB_Z, 3.0, 1.0, 2.0, 4.0, -6.5, 9);
  expect(its[0] == 9 && mu[0] == 3.0, "uvb_result: the optional outputs");
}

// two groups of 8 traits, solve workgroups of 4, two slots each.  Workgroup 0: patterns 0, 1, 2, 0 -- pattern 2 finds no slot, the second
// pattern 0 shares the first's.  Workgroup 1: an idle trait (it takes no slot), then patterns 2, 2, 1.  Group 1: idle throughout.
static void check_slots() {
  const struct { double nt; int pat; } t[8] = {{5, 0}, {5, 1}, {5, 2}, {5, 0}, {0, 0}, {7, 2}, {7, 2}, {7, 1}};
  const UvbTrait idle = {0.0, 0.0, 0, -1, 0, 0};
  std::vector<UvbTrait> tr(16, idle);
  for (int i = 0; i < 8; ++i) { tr[(size_t)i].nt = t[i].nt; tr[(size_t)i].pat = t[i].pat; }
  const std::vector<int> slotpat = uvb_slots(tr, {2, 2, 2, 8, 4});
  const int want_pat[8] = {0, 1, 2, 1, -1, -1, -1, -1}, want_slot[16] = {0, 1, -1, 0, -1, 0, 0, 1, -1, -1, -1, -1, -1, -1, -1, -1};
  expect(slotpat.size() == 8, "uvb_slots: groups x nsolve x ngl entries");
  for (size_t i = 0; i < 8 && i < slotpat.size(); ++i) if (slotpat[i] != want_pat[i]) { fprintf(stderr, "uvb_slots: slotpat[%zu] = %d, expected %d\n", i, slotpat[i], want_pat[i]); ++fails; }
  for (size_t i = 0; i < 16; ++i) if (tr[i].slot != want_slot[i]) { fprintf(stderr, "uvb_slots: trait %zu in slot %d, expected %d\n", i, tr[i].slot, want_slot[i]); ++fails; }
}

int main(int argc, char **argv) {
  if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: uvb_tail_check CASES\n"); return 2; }
  check_result();
  check_slots();
  const int ncases = (int)rd();
  for (int cs = 0; cs < ncases; ++cs) {
    const int variant = (int)rd(); const bool two = rd() != 0; const int maxit = (int)rd();
    const double logtol = rd(), df0 = rd(); const int64_t p = (int64_t)rd(), q1 = (int64_t)rd(); const int nsw = (int)rd();
    UvbState q;
    q.nt = rd(); q.mu = rd(); q.sumy = rd(); q.vy = rd();
    q.active = q.nt > 0 && maxit > 0;
    const double TrXSX = rd(), TrXSX1 = rd();
    uvb_start(q, variant, df0, p, TrXSX, two ? &TrXSX1 : nullptr);
    near("start ve", cs, -1, q.ve, rd()); near("start vb", cs, -1, q.vb, rd());
    const double lam = rd(); near("start vb1", cs, -1, q.vb1, rd()); const double lam1 = rd();
    const bool skip1 = rd() != 0, skip2 = rd() != 0;
    if (q.skip1 != skip1 || q.skip2 != skip2) { fprintf(stderr, "case %d: skips %d %d, expected %d %d\n", cs, (int)q.skip1, (int)q.skip2, (int)skip1, (int)skip2); ++fails; }
    if (!skip2) near("start lam", cs, -1, q.lam, lam);      // (a skipped design's lambda is never formed)
    if (two && !skip1) near("start lam1", cs, -1, q.lam1, lam1);
    for (int sw = 0; sw < nsw; ++sw) {
      if (!q.active) { fprintf(stderr, "case %d: stopped before sweep %d\n", cs, sw); ++fails; }
      double v[9], leg[3];
      for (double &x : v) x = rd();
      leg[0] = v[6]; leg[1] = v[7]; leg[2] = v[8];
      const UvbSums s = {v[0], v[1], v[2], v[3], v[4], v[5], two ? leg : nullptr};
      const double m0 = uvb_update(q, s, variant, maxit, logtol, df0, p, q1);
      near("mu0", cs, sw, m0, v[0] / q.nt);
      near("mu", cs, sw, q.mu, rd()); near("ve", cs, sw, q.ve, rd()); near("vb", cs, sw, q.vb, rd()); near("vb1", cs, sw, q.vb1, rd());
      const double l = rd(), l1 = rd();
      if (!skip2) near("lam", cs, sw, q.lam, l);
      if (two && !skip1) near("lam1", cs, sw, q.lam1, l1);
      near("cnv", cs, sw, q.cnv, rd());
      const int its = (int)rd(); const bool on = rd() != 0;
      if (q.its != its || q.active != on) { fprintf(stderr, "case %d sweep %d: its %d, goes on %d; expected %d, %d\n", cs, sw, q.its, (int)q.active, its, (int)on); ++fails; }
    }
  }
  fclose(in);
  if (fails) return 1;
  printf("uvb_tail_check ok\n");
  return 0;
}
