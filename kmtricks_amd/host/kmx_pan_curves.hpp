// kmx_pan_curves.hpp -- the pangenome growth and core curves of `kmx pan`, in closed form from the recurrence spectrum (plain C++, no
// device).  With h[r] the rows that r of the M samples hold and q_r(m) = C(M - r, m) / C(M, m), the share of the m-subsets that miss
// all r holders (the expectation over all M! orders of adding samples):
//   pan_mean(m)  = sum over r >= 1 of h[r] * (1 - q_r(m))                 rows met after m samples
//   core_mean(m) = sum over r >= m of h[r] * C(r, m) / C(M, m)            rows all of the first m samples hold
//   new_mean(m)  = sum over r of h[r] * q_r(m - 1) * r / (M - m + 1)      rows the m-th sample brings: pan(m) - pan(m - 1) without the
//                                                                         cancellation; at m = 1 it is pan_mean(1)
// Both ratios move from m - 1 to m by one factor: q_r(m) = q_r(m - 1) * (M - r - m + 1) / (M - m + 1) and C(r, m) / C(M, m) =
// C(r, m - 1) / C(M, m - 1) * (r - m + 1) / (M - m + 1), so all curves cost O(M * distinct r) multiplications in double and no lgamma.
// Every term is a product of at most 2 m factors that are each rounded once, all terms are non-negative, and they are weighted by h:
// the absolute error of a value is below 4 M * 2^-53 * sum(h).
// The ordered curves are integers: pan_order(m) = sum over j < m of first[j], core_order(m) = sum over j >= m of gap[j].
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace kmxpan {

struct Curves {
  std::vector<double> pan_mean, core_mean, new_mean;      // [M + 1], entry 0 unused
  std::vector<uint64_t> pan_order, core_order;            // [M + 1], entry 0 unused
  bool has_alpha = false;
  double heaps_alpha = 0.0;      // minus the least-squares slope of ln new_mean(m) on ln m over the m in 2 ... M with new_mean(m) > 0
};

// h, first, gap: M + 1 entries each
inline Curves curves(uint32_t M, const uint64_t* h, const uint64_t* first, const uint64_t* gap)
{
  Curves c;
  c.pan_mean.assign((size_t)M + 1, 0.0); c.core_mean.assign((size_t)M + 1, 0.0); c.new_mean.assign((size_t)M + 1, 0.0);
  c.pan_order.assign((size_t)M + 1, 0); c.core_order.assign((size_t)M + 1, 0);
  // the recurrences that occur, their weights and the two running ratios
  std::vector<uint32_t> rs; std::vector<double> w, q, k;
  for (uint32_t r = 1; r <= M; r++) if (h[r]) { rs.push_back(r); w.push_back((double)h[r]); q.push_back(1.0); k.push_back(1.0); }
  for (uint32_t m = 1; m <= M; m++) {
    const double left = (double)(M - m + 1);      // samples not yet added before the m-th
    double pan = 0.0, core = 0.0, nw = 0.0;
    for (size_t i = 0; i < rs.size(); i++) {
      const uint32_t r = rs[i];
      nw += w[i] * q[i] * ((double)r / left);                                        // q_r(m - 1)
      q[i] = M - r >= m ? q[i] * ((double)(M - r - m + 1) / left) : 0.0;             // q_r(m)
      k[i] = r >= m ? k[i] * ((double)(r - m + 1) / left) : 0.0;                     // C(r, m) / C(M, m)
      pan += w[i] * (1.0 - q[i]);
      core += w[i] * k[i];
    }
    c.pan_mean[m] = pan; c.core_mean[m] = core; c.new_mean[m] = nw;
  }
  uint64_t run = 0;
  for (uint32_t m = 1; m <= M; m++) { run += first[m - 1]; c.pan_order[m] = run; }
  run = 0;
  for (uint32_t m = M; m >= 1; m--) { run += gap[m]; c.core_order[m] = run; }
  // Heaps' law: new(m) ~ m^-alpha
  std::vector<double> xs, ys;
  for (uint32_t m = 2; m <= M; m++) if (c.new_mean[m] > 0.0) { xs.push_back(std::log((double)m)); ys.push_back(std::log(c.new_mean[m])); }
  if (xs.size() >= 3) {
    double mx = 0.0, my = 0.0;
    for (size_t i = 0; i < xs.size(); i++) { mx += xs[i]; my += ys[i]; }
    mx /= (double)xs.size(); my /= (double)xs.size();
    double sxy = 0.0, sxx = 0.0;
    for (size_t i = 0; i < xs.size(); i++) { sxy += (xs[i] - mx) * (ys[i] - my); sxx += (xs[i] - mx) * (xs[i] - mx); }
    if (sxx > 0.0) { c.has_alpha = true; c.heaps_alpha = -(sxy / sxx); }
  }
  return c;
}

}  // namespace kmxpan
