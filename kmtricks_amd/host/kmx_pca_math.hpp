// kmx_pca_math.hpp -- the host side of `kmx pca` (plain C++, no device): the class weights in fixed point, the centred and scaled Gram
// matrix of the samples from the device's tables, and the eigen-solve.
//
// A row of recurrence R over the M listed samples has frequency p_R = R / M and the EIGENSTRAT weight 1 / (p_R (1 - p_R)) =
// M^2 / (R (M - R)); in fixed point wt_R = round(2^F M^2 / (R (M - R))), worked out in integers as
// (2^(F + 1) M^2 + R (M - R)) / (2 R (M - R)).  F is the largest value <= 31 with every wt_R <= 2^32 - 1 and the sum over R of wt_R n_R
// < 2^63 (n_R the rows of class R, from the spectrum): no cell of the device's u64 table can wrap.  With w_R = wt_R / 2^F:
//   G_ij = (T_ij / 2^F - A_i - A_j + S) / n_used,   A_i = sum over R of w_R p_R sh[R][i],   S = sum over R of w_R p_R^2 n_R
// where T is the table of kmx_gram_*, sh the shared table of kmx_pan_*, and n_used the rows of the classes of a weight other than 0.
// Rounding: w_R R = wt_R R / 2^F is exact in double (below 2^47); a term of A_i is rounded twice (/ M, x sh), a term of S three times
// (x R, / M^2, x n_R), every term is non-negative and a sum has at most M + 1 of them; T_ij is rounded once on its way to double and
// four operations follow.  So |G_ij - exact| <= (M + 8) 2^-53 (T_ij / 2^F + A_i + A_j + S) / n_used.
//
// The eigen-solve is the cyclic Jacobi method: rotations that zero one off-diagonal pair at a time, swept until no pair is left above
// the rounding of the diagonal.  It is backward stable, it finds small eigenvalues to high relative accuracy, and the vectors come out
// orthogonal to working precision also inside a repeated eigenvalue.  O(M^3) a sweep, 6 to 10 sweeps.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

namespace kmxpca {

struct Weights {
  std::vector<uint32_t> wt;      // [M + 1]
  uint32_t F = 0;
  uint64_t n_used = 0;
  bool ok = false;               // false: even F = 0 does not fit (the sum of the weights of all rows reaches 2^63)
};

// n: the rows by recurrence, M + 1 entries.  Classes outside [lo, hi] get the weight 0; lo >= 1 and hi <= M - 1 for eigenstrat.
inline Weights class_weights(uint32_t M, const uint64_t* n, uint32_t lo, uint32_t hi, bool eigenstrat)
{
  typedef unsigned __int128 u128;
  Weights w;
  w.wt.assign((size_t)M + 1, 0);
  for (int F = eigenstrat ? 31 : 0; F >= 0 && !w.ok; F--) {
    u128 sum = 0;
    bool fits = true;
    for (uint32_t R = lo; R <= hi && R <= M && fits; R++) {
      u128 v = 1;
      if (eigenstrat) {
        const u128 d = (u128)R * (M - R);
        v = (((u128)1 << (F + 1)) * M * M + d) / (2 * d);
      }
      if (v > 0xFFFFFFFFull) { fits = false; break; }
      w.wt[R] = (uint32_t)v;
      sum += v * n[R];
      if (sum >= ((u128)1 << 63)) fits = false;
    }
    if (fits) { w.ok = true; w.F = (uint32_t)F; }
  }
  if (!w.ok) { std::fill(w.wt.begin(), w.wt.end(), 0u); return w; }
  for (uint32_t R = 0; R <= M; R++) if (w.wt[R]) w.n_used += n[R];
  return w;
}

// T: [N][N] by input column; sh: [M + 1][N] by input column; cols: the list (null: the identity, M = N) -> G [M][M] in list order
inline std::vector<double> gram_matrix(uint32_t M, uint32_t N, const uint32_t* cols, const Weights& w, const uint64_t* n, const uint64_t* sh,
                                       const uint64_t* T)
{
  const double scale = std::ldexp(1.0, -(int)w.F), dM = (double)M, dMM = (double)M * (double)M;
  std::vector<double> A(M, 0.0), G((size_t)M * M, 0.0);
  double S = 0.0;
  for (uint32_t R = 0; R <= M; R++) {
    if (!w.wt[R]) continue;
    const double wr = (double)((uint64_t)w.wt[R] * R) * scale;      // w_R R, exact
    S += wr * (double)R / dMM * (double)n[R];
    const double wp = wr / dM;
    for (uint32_t i = 0; i < M; i++) A[i] += wp * (double)sh[(size_t)R * N + (cols ? cols[i] : i)];
  }
  const double nu = (double)w.n_used;
  for (uint32_t i = 0; i < M; i++)
    for (uint32_t j = i; j < M; j++) {
      const uint64_t t = T[(size_t)(cols ? cols[i] : i) * N + (cols ? cols[j] : j)];
      const double g = (((double)t * scale - (A[i] + A[j])) + S) / nu;
      G[(size_t)i * M + j] = G[(size_t)j * M + i] = g;
    }
  return G;
}

// G: symmetric [M][M] (overwritten).  -> eigenvalues descending; vec[k * M + i]: component i of the k-th unit eigenvector, its sign such
// that the first component of largest magnitude is positive
inline void eigen_sym(uint32_t M, std::vector<double>& G, std::vector<double>* val, std::vector<double>* vec)
{
  const size_t n = M;
  std::vector<double> V(n * n, 0.0);
  for (size_t i = 0; i < n; i++) V[i * n + i] = 1.0;
  double frob = 0.0;
  for (double g : G) frob += g * g;
  const double floor_abs = 0x1p-80 * std::sqrt(frob);      // (far below the rounding of any entry that matters: the noise of a null space ends here)
  for (int sweep = 0; sweep < 64; sweep++) {
    bool turned = false;
    for (size_t p = 0; p + 1 < n; p++)
      for (size_t q = p + 1; q < n; q++) {
        const double apq = G[p * n + q];
        if (apq == 0.0) continue;
        const double app = G[p * n + p], aqq = G[q * n + q];
        // a pair below the rounding of both diagonal entries is taken for zero
        if (std::fabs(apq) <= floor_abs || (sweep > 0 && std::fabs(apq) <= 0x1p-54 * std::sqrt(std::fabs(app)) * std::sqrt(std::fabs(aqq)))) {
          G[p * n + q] = G[q * n + p] = 0.0;
          continue;
        }
        turned = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::hypot(theta, 1.0));
        const double c = 1.0 / std::hypot(t, 1.0), s = t * c;
        G[p * n + p] = app - t * apq;
        G[q * n + q] = aqq + t * apq;
        G[p * n + q] = G[q * n + p] = 0.0;
        for (size_t k = 0; k < n; k++) {
          if (k != p && k != q) {
            const double akp = G[k * n + p], akq = G[k * n + q];
            G[k * n + p] = G[p * n + k] = c * akp - s * akq;
            G[k * n + q] = G[q * n + k] = s * akp + c * akq;
          }
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
    if (!turned) break;
  }
  std::vector<size_t> at(n);
  std::iota(at.begin(), at.end(), (size_t)0);
  std::stable_sort(at.begin(), at.end(), [&](size_t a, size_t b) { return G[a * n + a] > G[b * n + b]; });
  val->assign(n, 0.0);
  vec->assign(n * n, 0.0);
  for (size_t k = 0; k < n; k++) {
    const size_t c = at[k];
    (*val)[k] = G[c * n + c];
    double norm = 0.0, big = 0.0;
    size_t arg = 0;
    for (size_t i = 0; i < n; i++) { const double v = V[i * n + c]; norm += v * v; if (std::fabs(v) > big) { big = std::fabs(v); arg = i; } }
    norm = std::sqrt(norm);
    const double f = (V[arg * n + c] < 0 ? -1.0 : 1.0) / (norm > 0 ? norm : 1.0);
    for (size_t i = 0; i < n; i++) (*vec)[k * n + i] = V[i * n + c] * f;
  }
}

}  // namespace kmxpca
