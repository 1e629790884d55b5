// kmx_assoc_math.hpp -- the arithmetic of `kmx assoc` that needs no device: the design -- the covariates' orthonormal
// basis, the phenotype's residual, both in fixed point as kmx_assoc_* takes them -- and the constants that go with it.  Plain C++.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace kmxassoc {

constexpr uint32_t FRAC_BITS = 30;      // F: an entry is round(value * 2^30), |value| <= 1

struct Design {
  bool ok = false;
  std::string err;                  // why not
  uint32_t M = 0, q = 0;            // listed samples; columns of C = [1 | covariates]
  std::vector<int32_t> vecs;        // [M][q + 1]: vector 0 the residual phenotype / ymax, 1 ... q the basis
  double gain = 0, vmin = 0, ymax = 0, syy = 0;
};

// what quantisation and rounding can add to v = rec - h at the most.  With d = 2^-31 the fixed point moves an entry of Q by at most d,
// so a_j = sum over the rec present samples of vec_j / 2^30 is off x'q_j by e_j, |e_j| <= rec d <= M d.  |x'q_j| <= sqrt(rec) <=
// sqrt(M) (Cauchy-Schwarz, |q_j| = 1), and a_j^2 - (x'q_j)^2 = 2 (x'q_j) e_j + e_j^2: over the q vectors at most
// q (2 M sqrt(M) d + M^2 d^2).  The doubles add, with h <= about M: a rounding per square and per sum of h, one for v, and the basis'
// own orthonormality error after two passes of Gram-Schmidt, a few units of 2^-53 each: (q + 2) M 2^-50 covers them with room.
inline double v_bound(uint32_t M, uint32_t q)
{
  const double d = std::ldexp(1.0, -31), m = (double)M;
  return (double)q * (2.0 * m * std::sqrt(m) * d + m * m * d * d) + ((double)q + 2.0) * m * std::ldexp(1.0, -50);
}

// y[M]; cov[M][K] row-major (K may be 0).  Q: modified Gram-Schmidt applied twice; a column whose norm falls below 1e-8 of its original
// is dependent.  y~ = y - Q Q'y, the projection applied twice.
inline Design make_design(uint32_t M, uint32_t K, const std::vector<double>& y, const std::vector<double>& cov)
{
  Design D;
  D.M = M; D.q = K + 1;
  const uint32_t q = D.q, V = q + 1;
  if (K > 31) { D.err = "more than 31 covariate columns"; return D; }
  if (M < q + 2) { D.err = "too few samples: M - q must be at least 2 (" + std::to_string(M) + " samples, " + std::to_string(q) + " model columns with the intercept)"; return D; }
  bool constant = true;
  for (uint32_t m = 1; m < M; m++) if (y[m] != y[0]) constant = false;
  if (constant) { D.err = "the phenotype is constant"; return D; }
  std::vector<std::vector<double>> Q(q, std::vector<double>(M));
  auto dot = [&](const std::vector<double>& a, const std::vector<double>& b) { double s = 0; for (uint32_t m = 0; m < M; m++) s += a[m] * b[m]; return s; };
  for (uint32_t k = 0; k < q; k++) {
    std::vector<double>& v = Q[k];
    for (uint32_t m = 0; m < M; m++) v[m] = k == 0 ? 1.0 : cov[(size_t)m * K + (k - 1)];
    const double n0 = std::sqrt(dot(v, v));
    for (int pass = 0; pass < 2; pass++)
      for (uint32_t j = 0; j < k; j++) { const double c = dot(Q[j], v); for (uint32_t m = 0; m < M; m++) v[m] -= c * Q[j][m]; }
    const double n = std::sqrt(dot(v, v));
    if (!(n0 > 0.0) || !std::isfinite(n0) || !(n >= 1e-8 * n0)) { D.err = "covariates are linearly dependent"; return D; }
    for (uint32_t m = 0; m < M; m++) v[m] /= n;
  }
  std::vector<double> r(y.begin(), y.begin() + M);
  double ybig = 0;
  for (uint32_t m = 0; m < M; m++) ybig = std::max(ybig, std::fabs(y[m]));
  for (int pass = 0; pass < 2; pass++)
    for (uint32_t j = 0; j < q; j++) { const double c = dot(Q[j], r); for (uint32_t m = 0; m < M; m++) r[m] -= c * Q[j][m]; }
  for (uint32_t m = 0; m < M; m++) D.ymax = std::max(D.ymax, std::fabs(r[m]));
  if (!(D.ymax > 1e-12 * ybig) || !std::isfinite(D.ymax)) { D.ymax = 0; D.err = "the phenotype is a combination of the covariates: nothing is left to test"; return D; }
  const double one = std::ldexp(1.0, FRAC_BITS);
  D.vecs.assign((size_t)M * V, 0);
  unsigned __int128 ss = 0;
  for (uint32_t m = 0; m < M; m++) {
    const int64_t v0 = std::llround(r[m] / D.ymax * one);
    D.vecs[(size_t)m * V] = (int32_t)v0;
    ss += (unsigned __int128)(v0 * v0);
    for (uint32_t j = 0; j < q; j++) D.vecs[(size_t)m * V + 1 + j] = (int32_t)std::llround(Q[j][m] * one);
  }
  D.syy = std::ldexp((double)ss, -2 * (int)FRAC_BITS);      // the sum exact in 128 bits, one conversion
  D.gain = (double)(M - q) / D.syy;
  D.vmin = std::max(std::ldexp(1.0, -10), v_bound(M, q));
  D.ok = true;
  return D;
}

}  // namespace kmxassoc
