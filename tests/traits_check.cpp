// tests/traits_check.cpp -- the traits' host set-up of the fp64 fits (bwgr_amd/csrc/traits.h) against plain loops written here, and against a
// few values worked out by hand: doubles by their bits, masks byte for byte.  A program of its own: built with -fsanitize=address,undefined
// and run by tests/test_traits_cpu.py.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <limits>
#include <random>
#include <vector>
#include "../bwgr_amd/csrc/traits.h"

using namespace bwgr;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); ++g_failed; } } while (0)

static const double NA = std::numeric_limits<double>::quiet_NaN();
static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

// n = 7 rows; columns by the rows they miss
static const int64_t N = 7;
static std::vector<double> column(unsigned missing_bits, double scale) {
  std::vector<double> c((size_t)N);
  for (int64_t r = 0; r < N; ++r) c[(size_t)r] = ((missing_bits >> r) & 1u) ? NA : scale * (double)((r * 5 + 3) % 7) + 0.1 * (double)r;
  return c;
}
static std::vector<double> columns(const std::vector<std::vector<double>> &cols) {
  std::vector<double> Y;
  for (const auto &c : cols) Y.insert(Y.end(), c.begin(), c.end());
  return Y;
}

// the plain statement of everything read_traits returns for traits that keep the rule
static void check_against_loops(const std::vector<double> &Y, int64_t k, int64_t ld, int64_t ycols, const TraitSet &S) {
  CHECK(S.bad == -1 && S.n == N && S.k == k && S.ld == ld);
  CHECK((int64_t)S.y.size() == ycols * ld && (int64_t)S.obs.size() == k * N);
  for (int64_t t = 0; t < k; ++t) {
    double nt = 0.0, mu = 0.0;
    for (int64_t r = 0; r < N; ++r) if (Y[(size_t)(t * N + r)] == Y[(size_t)(t * N + r)]) { nt += 1.0; mu += Y[(size_t)(t * N + r)]; }
    if (nt > 0.0) mu /= nt;
    std::vector<double> c((size_t)ld, 0.0);
    for (int64_t r = 0; r < N; ++r) if (Y[(size_t)(t * N + r)] == Y[(size_t)(t * N + r)]) c[(size_t)r] = Y[(size_t)(t * N + r)] - mu;
    double sumy = 0.0, vy = 0.0;
    for (int64_t r = 0; r < ld; ++r) { sumy += c[(size_t)r]; vy += c[(size_t)r] * c[(size_t)r]; }   // over every row, the padding included
    if (nt > 0.0) vy /= (nt - 1.0);
    CHECK(same_bits(S.nt[(size_t)t], nt) && same_bits(S.mu[(size_t)t], mu) && same_bits(S.sumy[(size_t)t], sumy) && same_bits(S.vy[(size_t)t], vy));
    CHECK(memcmp(S.y.data() + (size_t)(t * ld), c.data(), sizeof(double) * (size_t)ld) == 0);
    for (int64_t r = 0; r < N; ++r) {
      CHECK(S.obs[(size_t)(t * N + r)] == (Y[(size_t)(t * N + r)] == Y[(size_t)(t * N + r)] ? 1 : 0));
      CHECK(S.observed(t, r) == (S.obs[(size_t)(t * N + r)] == 1));
    }
  }
  for (size_t i = (size_t)(k * ld); i < S.y.size(); ++i) CHECK(same_bits(S.y[i], 0.0));
}

// the packers, bit by bit and byte by byte
static void check_packers(const TraitSet &S, int64_t t0, int kg, const Patterns &P) {
  const int64_t ld = S.ld;
  std::vector<unsigned long long> w64((size_t)ld, ~0ull);
  pack_row_bits(S, t0, kg, w64.data());
  for (int64_t r = 0; r < ld; ++r)
    for (int j = 0; j < 64; ++j) CHECK(((w64[(size_t)r] >> j) & 1ull) == (unsigned long long)(j < kg && r < N && S.observed(t0 + j, r) ? 1 : 0));
  const int np = (int)P.rep.size();
  if (np <= 32) {
    std::vector<uint32_t> w32((size_t)ld, ~0u);
    pack_row_bits(S, P.rep.data(), np, w32.data());
    for (int64_t r = 0; r < ld; ++r)
      for (int j = 0; j < 32; ++j) CHECK(((w32[(size_t)r] >> j) & 1u) == (uint32_t)(j < np && r < N && S.observed(P.rep[(size_t)j], r) ? 1 : 0));
  }
  std::vector<uint8_t> zm(3, 0x5A);   // (appends: what is there stays)
  append_byte_masks(S, P.rep.data(), np, zm);
  CHECK((int64_t)zm.size() == 3 + np * ld && zm[0] == 0x5A && zm[2] == 0x5A);
  for (int j = 0; j < np; ++j)
    for (int64_t r = 0; r < ld; ++r) CHECK(zm[(size_t)(3 + j * ld + r)] == (r < N && S.observed(P.rep[(size_t)j], r) ? 0xFF : 0));
}

// the plain statement of the patterns: id by comparing every row with the earlier traits' rows
static void check_patterns(const TraitSet &S, int64_t t0, int64_t t1, const Patterns &P) {
  std::vector<int64_t> rep;
  CHECK((int64_t)P.id.size() == t1 - t0);
  for (int64_t t = t0; t < t1; ++t) {
    int want = -1;
    if (S.nt[(size_t)t] > 0.0) {
      for (size_t g = 0; g < rep.size() && want < 0; ++g) {
        bool same = true;
        for (int64_t r = 0; r < N; ++r) same = same && S.observed(t, r) == S.observed(rep[g], r);
        if (same) want = (int)g;
      }
      if (want < 0) { want = (int)rep.size(); rep.push_back(t); }
    }
    CHECK(P.id[(size_t)(t - t0)] == want);
  }
  CHECK(P.rep == rep);
}

static void one_trait_fully_observed() {
  for (int64_t ld : {(int64_t)8, (int64_t)128}) {
    const std::vector<double> Y = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0};
    for (RowRule rule : {RowRule::AtLeastTwo, RowRule::NotOne}) {
      const TraitSet S = read_traits(Y.data(), N, 1, ld, 1, rule);
      check_against_loops(Y, 1, ld, 1, S);
      // by hand: mean 4; centred -3 .. 3, sum 0, squares 28 over 6
      CHECK(S.nt[0] == 7.0 && S.mu[0] == 4.0 && same_bits(S.sumy[0], 0.0) && S.vy[0] == 28.0 / 6.0);
      CHECK(S.y[0] == -3.0 && S.y[6] == 3.0 && same_bits(S.y[7], 0.0) && same_bits(S.y[(size_t)ld - 1], 0.0));
      const Patterns P = find_patterns(S, 0, 1);
      CHECK(P.id == std::vector<int>{0} && P.rep == std::vector<int64_t>{0});
      check_packers(S, 0, 1, P);
    }
  }
}

static void three_traits_two_patterns() {
  const std::vector<double> Y = columns({column(0x12, 1.0), column(0x01, 2.0), column(0x12, -3.0)});
  const TraitSet S = read_traits(Y.data(), N, 3, 8, 64, RowRule::AtLeastTwo);   // (y padded to a group of 64 columns)
  check_against_loops(Y, 3, 8, 64, S);
  const Patterns P = find_patterns(S, 0, 3);
  CHECK((P.id == std::vector<int>{0, 1, 0}) && (P.rep == std::vector<int64_t>{0, 1}));
  check_patterns(S, 0, 3, P);
  check_packers(S, 0, 3, P);
  // by hand: mrr's word of row 0 (trait 1 misses it), row 1 (traits 0 and 2 miss it), row 2 (all there)
  std::vector<uint32_t> zt(8);
  pack_row_bits(S, (int64_t)0, 3, zt.data());
  CHECK(zt[0] == 0x5u && zt[1] == 0x2u && zt[2] == 0x7u && zt[4] == 0x2u && zt[7] == 0u);
  std::vector<uint32_t> zb(8);
  pack_row_bits(S, P.rep.data(), 2, zb.data());
  CHECK(zb[0] == 0x1u && zb[1] == 0x2u && zb[2] == 0x3u && zb[7] == 0u);
}

static void sixty_six_traits_two_groups() {
  // traits 1 .. 63 alternate between two patterns of their own; trait 64 has trait 0's rows, trait 65 rows nobody else has
  std::vector<std::vector<double>> cols;
  cols.push_back(column(0x03, 1.0));
  for (int t = 1; t < 64; ++t) cols.push_back(column(t % 2 ? 0x0C : 0x30, 1.0 + t));
  cols.push_back(column(0x03, -2.0));
  cols.push_back(column(0x41, 0.5));
  const std::vector<double> Y = columns(cols);
  const TraitSet S = read_traits(Y.data(), N, 66, 8, 128, RowRule::NotOne);
  check_against_loops(Y, 66, 8, 128, S);
  const Patterns P0 = find_patterns(S, 0, 64), P1 = find_patterns(S, 64, 66);
  check_patterns(S, 0, 64, P0);
  check_patterns(S, 64, 66, P1);
  CHECK(P0.rep == (std::vector<int64_t>{0, 1, 2}) && P0.id[0] == 0 && P0.id[1] == 1 && P0.id[2] == 2 && P0.id[63] == 1);
  // ids are a group's own: trait 64 is pattern 0 of group 1 and its own representative, although trait 0 has the same rows
  CHECK(P1.id == (std::vector<int>{0, 1}) && P1.rep == (std::vector<int64_t>{64, 65}));
  check_packers(S, 0, 64, P0);
  check_packers(S, 64, 2, P1);
  // across the whole set (as mrr would ask, were k this large) trait 64 does share trait 0's pattern
  const Patterns all = find_patterns(S, 0, 66);
  check_patterns(S, 0, 66, all);
  CHECK(all.id[64] == 0 && all.id[65] == 3 && all.rep == (std::vector<int64_t>{0, 1, 2, 65}));
}

static void empty_and_short_traits() {
  const std::vector<double> Y = columns({column(0x00, 1.0), column(0x7F, 1.0), column(0x20, 2.0)});   // trait 1 has no observed row
  const TraitSet S = read_traits(Y.data(), N, 3, 8, 3, RowRule::NotOne);
  check_against_loops(Y, 3, 8, 3, S);
  CHECK(S.nt[1] == 0.0 && same_bits(S.mu[1], 0.0) && same_bits(S.vy[1], 0.0) && same_bits(S.sumy[1], 0.0));
  const Patterns P = find_patterns(S, 0, 3);
  CHECK((P.id == std::vector<int>{0, -1, 1}) && (P.rep == std::vector<int64_t>{0, 2}));
  check_patterns(S, 0, 3, P);
  check_packers(S, 0, 3, P);
  const TraitSet M = read_traits(Y.data(), N, 3, 8, 3, RowRule::AtLeastTwo);
  CHECK(M.bad == 1 && M.nt[1] == 0.0);
  // one observed row: refused by both rules, and it is the first offender that is reported
  const std::vector<double> Y1 = columns({column(0x00, 1.0), column(0x00, 3.0), column(0x7E, 1.0), column(0x7F, 1.0), column(0x7D, 1.0)});
  for (RowRule rule : {RowRule::AtLeastTwo, RowRule::NotOne}) {
    const TraitSet B = read_traits(Y1.data(), N, 5, 8, 5, rule);
    CHECK(B.bad == 2 && B.nt[2] == 1.0);
  }
  // exactly two observed rows (0 and 6): mean of the two, centred -d/2 and d/2, vy = d^2 / 2 over 1
  std::vector<double> Y2 = column(0x3E, 1.0);
  Y2[0] = 1.0; Y2[6] = 4.0;
  for (RowRule rule : {RowRule::AtLeastTwo, RowRule::NotOne}) {
    const TraitSet T = read_traits(Y2.data(), N, 1, 8, 1, rule);
    check_against_loops(Y2, 1, 8, 1, T);
    CHECK(T.nt[0] == 2.0 && T.mu[0] == 2.5 && T.y[0] == -1.5 && T.y[6] == 1.5 && same_bits(T.sumy[0], 0.0) && T.vy[0] == 4.5);
  }
}

static void signed_zero_and_subnormal() {
  const double sub = std::numeric_limits<double>::denorm_min() * 3.0;
  const std::vector<double> Y = columns({{-0.0, NA, -0.0, -0.0, NA, -0.0, -0.0}, {sub, -sub, 0.0, 4.0 * sub, -0.0, NA, sub}, {-0.0, 1.0, -1.0, 0.5, -0.5, sub, -sub}});
  for (int64_t ld : {(int64_t)8, (int64_t)128}) {
    const TraitSet S = read_traits(Y.data(), N, 3, ld, 3, RowRule::NotOne);
    check_against_loops(Y, 3, ld, 3, S);
    // by hand: five times -0.0 sum to +0.0 from a +0.0 start; -0.0 - +0.0 = -0.0 stays in the column, and the sums stay +0.0
    CHECK(same_bits(S.mu[0], 0.0) && same_bits(S.y[0], -0.0) && same_bits(S.y[1], 0.0) && same_bits(S.sumy[0], 0.0) && same_bits(S.vy[0], 0.0));
  }
}

static void z_without_padding() {
  const int64_t q = 3, ldz = N + 3;
  std::vector<double> Z((size_t)(q * ldz));
  for (size_t i = 0; i < Z.size(); ++i) Z[i] = (double)i * 0.25 - 3.0;
  for (int64_t j = 0; j < q; ++j) { Z[(size_t)(j * ldz + N)] = NA; Z[(size_t)(j * ldz + N + 2)] = INFINITY; }   // in the padding: ignored
  std::vector<double> out(1, 9.0);
  int64_t r = -5, c = -5;
  CHECK(compact_z(Z.data(), N, q, ldz, out, &r, &c) && r == -5 && c == -5 && (int64_t)out.size() == N * q);
  for (int64_t j = 0; j < q; ++j) for (int64_t i = 0; i < N; ++i) CHECK(same_bits(out[(size_t)(j * N + i)], Z[(size_t)(j * ldz + i)]));
  // the first in column-major order: (5, 1) comes before (2, 2) and (0, 2), and after nothing
  std::vector<double> Zb = Z;
  Zb[(size_t)(2 * ldz + 0)] = NA; Zb[(size_t)(2 * ldz + 2)] = -INFINITY; Zb[(size_t)(1 * ldz + 5)] = INFINITY; Zb[(size_t)(1 * ldz + 6)] = NA;
  CHECK(!compact_z(Zb.data(), N, q, ldz, out, &r, &c) && r == 5 && c == 1);
  Zb[(size_t)(1 * ldz + 5)] = 1.0;
  CHECK(!compact_z(Zb.data(), N, q, ldz, out, &r, &c) && r == 6 && c == 1);
  Zb[(size_t)(1 * ldz + 6)] = 1.0;
  CHECK(!compact_z(Zb.data(), N, q, ldz, out, &r, &c) && r == 0 && c == 2);
  CHECK(compact_z(Z.data(), N, 0, ldz, out, &r, &c) && out.empty());
}

// bwgr_em_order's definition: the identity shuffled with seeds 0 .. s
static void cumulative_order() {
  for (size_t p : {(size_t)1, (size_t)2, (size_t)65}) {
    CumulativeOrder ord(p);
    std::vector<int> ident(p);
    for (size_t j = 0; j < p; ++j) ident[j] = (int)j;
    CHECK(ord.current() == ident);
    for (int s = 0; s <= 3; ++s) {
      std::vector<int> want = ident;
      for (int i = 0; i <= s; ++i) std::shuffle(want.begin(), want.end(), std::mt19937(i));
      const std::vector<int> &got = ord.next(s);
      CHECK(got == want && ord.current() == want && &got == &ord.current());
      std::vector<int> sorted = got;
      std::sort(sorted.begin(), sorted.end());
      CHECK(sorted == ident);
    }
  }
}

int main() {
  one_trait_fully_observed();
  three_traits_two_patterns();
  sixty_six_traits_two_groups();
  empty_and_short_traits();
  signed_zero_and_subnormal();
  z_without_padding();
  cumulative_order();
  if (g_failed) { fprintf(stderr, "traits_check: %d check(s) failed\n", g_failed); return 1; }
  printf("traits_check ok\n");
  return 0;
}
