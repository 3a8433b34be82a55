// bwgr_amd/csrc/traits.h -- what the fp64 fits (mrr_host.hip.h, uvb_host.hip.h) do on the host before a kernel runs: reading Y, the missingness patterns,
// the observed-row masks in the layouts the kernels read, Z without its padding, and the cumulative marker order.  Plain C++17, no device
// runtime: tests/traits_check.cpp runs it as a program of its own under the sanitizers (tests/test_traits_cpu.py).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>

namespace bwgr {

// which counts of observed rows a trait may have
enum class RowRule {
  AtLeastTwo,   // mrr: a trait with fewer than two observed rows is refused
  NotOne        // the UVBETA family: exactly one is refused (the variances divide by n - 1); none is an empty trait -- zero column, no sweeps
};

// Y as the fits use it.  Y is n x k column-major, NaN = missing.
struct TraitSet {
  int64_t n = 0, k = 0, ld = 0;
  int64_t bad = -1;                 // the first trait that broke the rule (its nt is set; nothing after it is), or -1
  std::vector<double> nt, mu, sumy, vy;
  std::vector<double> y;            // ycols >= k columns of stride ld (those past k are zero): Y - mu on the observed rows, +0.0 on every other row and on the padding
  std::vector<uint8_t> obs;         // k columns of stride n: 1 where the row is observed, else 0 (as such, uvbeta_dense's mask)
  bool observed(int64_t t, int64_t r) const { return obs[(size_t)t * (size_t)n + (size_t)r] != 0; }
};

// mu: the observed values summed in ascending row order, over nt.  sumy and vy: the centred values and their squares summed in ascending
// row order from +0.0 (the rows skipped would add +0.0); vy over nt - 1 last.
inline TraitSet read_traits(const double *Y, int64_t n, int64_t k, int64_t ld, int64_t ycols, RowRule rule) {
  TraitSet S;
  S.n = n; S.k = k; S.ld = ld;
  const size_t nk = (size_t)k;
  S.nt.assign(nk, 0.0); S.mu.assign(nk, 0.0); S.sumy.assign(nk, 0.0); S.vy.assign(nk, 0.0);
  S.y.assign((size_t)ycols * (size_t)ld, 0.0); S.obs.assign(nk * (size_t)n, 0);
  for (int64_t t = 0; t < k; ++t) {
    const double *Yt = Y + (size_t)t * (size_t)n;
    uint8_t *ot = S.obs.data() + (size_t)t * (size_t)n;
    double cnt = 0.0, sum = 0.0;
    for (int64_t r = 0; r < n; ++r)
      if (!std::isnan(Yt[r])) { ot[r] = 1; cnt += 1.0; sum += Yt[r]; }
    S.nt[(size_t)t] = cnt;
    if (cnt == 1.0 || (rule == RowRule::AtLeastTwo && cnt < 2.0)) { S.bad = t; return S; }
    if (cnt == 0.0) continue;
    const double m = sum / cnt;
    double *yt = S.y.data() + (size_t)t * (size_t)ld, s1 = 0.0, s2 = 0.0;
    for (int64_t r = 0; r < n; ++r)
      if (ot[r]) { yt[r] = Yt[r] - m; s1 += yt[r]; s2 += yt[r] * yt[r]; }
    S.mu[(size_t)t] = m; S.sumy[(size_t)t] = s1; S.vy[(size_t)t] = s2 / (cnt - 1.0);
  }
  return S;
}

// The missingness patterns of traits t0 .. t1-1: traits with the same observed rows share a pattern.  id[t - t0] numbers the patterns from 0
// in first-seen order (-1: a trait without observed rows has none); rep[g] is the first trait of pattern g.
struct Patterns { std::vector<int> id; std::vector<int64_t> rep; };
inline Patterns find_patterns(const TraitSet &S, int64_t t0, int64_t t1) {
  Patterns P;
  P.id.assign((size_t)(t1 - t0), -1);
  const size_t n = (size_t)S.n;
  for (int64_t t = t0; t < t1; ++t) {
    if (S.nt[(size_t)t] == 0.0) continue;
    int g = -1;
    for (int q = 0; q < (int)P.rep.size() && g < 0; ++q)
      if (memcmp(S.obs.data() + (size_t)P.rep[(size_t)q] * n, S.obs.data() + (size_t)t * n, n) == 0) g = q;
    if (g < 0) { g = (int)P.rep.size(); P.rep.push_back(t); }
    P.id[(size_t)(t - t0)] = g;
  }
  return P;
}

// out[r] (ld words, the padding 0): bit j says whether row r is observed for trait traits[j], j < m.  With the traits 0 .. k-1 this is mrr's
// word per row, with a pattern's representatives its pattern word, with a group's traits the UVBETA family's 64-bit word per row and group.
template <typename W, typename I> inline void pack_row_bits(const TraitSet &S, const I *traits, int m, W *out) {
  std::fill(out, out + S.ld, (W)0);
  for (int j = 0; j < m; ++j)
    for (int64_t r = 0; r < S.n; ++r)
      if (S.observed((int64_t)traits[j], r)) out[r] |= (W)1 << j;
}
// (the m traits t0, t0 + 1, ...)
template <typename W> inline void pack_row_bits(const TraitSet &S, int64_t t0, int m, W *out) {
  std::vector<int64_t> traits((size_t)m);
  for (int j = 0; j < m; ++j) traits[(size_t)j] = t0 + j;
  pack_row_bits(S, traits.data(), m, out);
}
// appends, for each of the m traits, a byte column of stride ld: 0xFF on its observed rows, else 0 (what k_mrr_gram ANDs with)
template <typename I> inline void append_byte_masks(const TraitSet &S, const I *traits, int m, std::vector<uint8_t> &out) {
  const size_t at = out.size();
  out.resize(at + (size_t)m * (size_t)S.ld, 0);
  for (int j = 0; j < m; ++j)
    for (int64_t r = 0; r < S.n; ++r)
      if (S.observed((int64_t)traits[j], r)) out[at + (size_t)j * (size_t)S.ld + (size_t)r] = 0xFF;
}

// Z (n x q, column stride ldz >= n) without its padding.  False where an entry is not finite: *row, *col is the first in column-major order.
inline bool compact_z(const double *Z, int64_t n, int64_t q, int64_t ldz, std::vector<double> &out, int64_t *row, int64_t *col) {
  out.resize((size_t)n * (size_t)q);
  for (int64_t j = 0; j < q; ++j)
    for (int64_t r = 0; r < n; ++r) {
      const double v = Z[(size_t)j * (size_t)ldz + (size_t)r];
      if (!std::isfinite(v)) { *row = r; *col = j; return false; }
      out[(size_t)j * (size_t)n + (size_t)r] = v;
    }
  return true;
}

// The marker order of the sweeps: the identity, shuffled once more for every sweep -- std::shuffle(order, std::mt19937(sweep)) on the
// previous sweep's order, the reference's own call.  After next(0), ..., next(s) it is what bwgr_em_order(p, s) returns.
class CumulativeOrder {
 public:
  explicit CumulativeOrder(size_t p) : ord_(p) { for (size_t j = 0; j < p; ++j) ord_[j] = (int)j; }
  const std::vector<int> &next(int sweep) { std::shuffle(ord_.begin(), ord_.end(), std::mt19937(sweep)); return ord_; }
  const std::vector<int> &current() const { return ord_; }
 private:
  std::vector<int> ord_;
};
}  // namespace bwgr
