// kmx_spectra_stats.hpp -- what `kmx spectra` reads off its two tables, on the host (DESIGN.md section 26 states every formula).  Integers
// wherever the definition allows; a ratio is formed once, from two integers, in long double (64 bits of mantissa: both operands are exact).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

namespace kmxspectra {

// a sample's line of hist: C1 + 2 numbers -- the rows with a count of b for b < C1, of C1 and more, and the volume of that last bin
struct SampleStats { uint64_t rows, singletons, volume, tail_volume; uint32_t valley, peak; };
inline SampleStats sample_stats(const uint64_t* h, uint32_t C1)
{
  SampleStats s{};
  for (uint32_t b = 1; b <= C1; b++) s.rows += h[b];
  s.singletons = h[1];
  s.tail_volume = h[C1 + 1];
  s.volume = s.tail_volume;
  for (uint32_t b = 1; b < C1; b++) s.volume += (uint64_t)b * h[b];
  // valley: the least b with 1 <= b < C1 - 1 and h[b] < h[b + 1] (the end of the errors' slope); peak: the least b with valley < b < C1
  // that maximises h[b]; 0 where there is none
  for (uint32_t b = 1; b + 1 < C1; b++) if (h[b] < h[b + 1]) { s.valley = b; break; }
  for (uint32_t b = s.valley + 1; b < C1; b++) if (s.peak == 0 || h[b] > h[s.peak]) s.peak = b;
  return s;
}

// a pair's table J[C2 + 1][C2 + 1] (a: the count in x, b: the count in y).  solid_all = |{a >= t}|, solid_held = |{a >= t, b >= 1}|
struct PairStats { uint64_t both, x_only, y_only, solid_all, solid_held; };
inline PairStats pair_stats(const uint64_t* J, uint32_t C2, uint32_t solid)
{
  PairStats s{};
  const uint32_t W = C2 + 1;
  for (uint32_t a = 0; a < W; a++)
    for (uint32_t b = 0; b < W; b++) {
      const uint64_t n = J[(uint64_t)a * W + b];
      if (a && b) s.both += n; else if (a) s.x_only += n; else if (b) s.y_only += n;
      if (a >= solid) { s.solid_all += n; if (b) s.solid_held += n; }
    }
  return s;
}

// num / den to `digits` places; "nan" for 0 / 0
inline std::string ratio(uint64_t num, uint64_t den, int digits = 6)
{
  if (den == 0) return "nan";
  char t[64];
  snprintf(t, sizeof t, "%.*Lf", digits, (long double)num / (long double)den);
  return t;
}

// the consensus quality of y against x over DISTINCT k-mers (Merqury's formula on rows, not on multiplicities): E the rows y alone holds,
// K the rows y holds; QV = -10 log10(1 - (1 - E / K)^(1 / k)).  "inf" when E = 0, "nan" when K = 0
inline std::string qv(const PairStats& s, uint32_t k)
{
  const uint64_t E = s.y_only, K = s.both + s.y_only;
  if (K == 0) return "nan";
  if (E == 0) return "inf";
  // 1 - (1 - e)^(1 / k) = -expm1(log1p(-e) / k): no cancellation for a small e; E = K: an error rate of 1, QV 0
  const long double q = E < K ? -10.0L * log10l(-expm1l(log1pl(-(long double)E / (long double)K) / (long double)k)) : 0.0L;
  char t[64];
  snprintf(t, sizeof t, "%.4Lf", q < 5e-5L ? 0.0L : q);      // (no "-0.0000")
  return t;
}

}  // namespace kmxspectra
