// kmer_dev.hpp -- the device code that says what a k-mer's minimizer and window hash ARE, shared by the kernels that must agree on
// them: the split (superk.hip), the count path (count.hip) and the query (query.hip).  One definition each, no copies.
#pragma once
#include "kmx_dev.hpp"

namespace kmx {

__device__ __forceinline__ bool nt_valid(u8 c)
{ // gatb tools/misc/api/Data.hpp:179-196
  const u8 u = c & 0xDF;
  return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

// value of an m-mer as the reference's minimizer table gives it: min(x, revcomp_m(x)), or 4^m - 1 when
// that contains AA anywhere but as a prefix (Model.hpp:1040-1064, 1220-1251) -- computed, not looked up
__device__ __forceinline__ u32 mmer_value(u32 x, int m)
{
  const u32 n1 = (1u << (2 * m)) - 1;                                     // m <= 15
  u32 t = __brev(x);
  t = ((t >> 1) & 0x55555555u) | ((t & 0x55555555u) << 1);                 // digits reversed, bits of a digit in order
  const u32 rc = (t >> (32 - 2 * m)) ^ (0xAAAAAAAAu & n1);                 // complement: A0 C1 T2 G3 -> digit ^ 2
  const u32 v = rc < x ? rc : x;
  const u64 mask_ma1 = 0x5555555555555555ULL & ((1ULL << ((m - 2) * 2)) - 1);
  u64 a1 = v; a1 = ~(a1 | (a1 >> 2)); a1 = ((a1 >> 1) & a1) & mask_ma1;
  return a1 ? n1 : v;
}
// bit i of y -> bit 2i (i < 16)
__device__ __forceinline__ u32 spread16(u32 y)
{
  y = (y | (y << 8)) & 0x00FF00FFu; y = (y | (y << 4)) & 0x0F0F0F0Fu;
  y = (y | (y << 2)) & 0x33333333u; y = (y | (y << 1)) & 0x55555555u;
  return y;
}
__device__ __forceinline__ u32 sk_at(u32 a, u32 b, int d, int lane)      // the value at position lane + d of the 128 positions (a: 0 .. 63, b: 64 .. 127), 0 <= d < 64
{
  const int src = (lane + d) & 63;
  const u32 x = (u32)__shfl((int)a, src), y = (u32)__shfl((int)b, src);
  return lane + d < 64 ? x : y;
}

__device__ __forceinline__ u64 rev_digits64(u64 x)
{ // reverse the 32 2-bit digits of a word
  x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
  return __builtin_bswap64(x);
}

// XXH64 of 8 / 16 bytes, seed 0 (Cyan4973/xxHash specification; KmXXHash sorting_count.hpp:346-363)
#define XP1 0x9E3779B185EBCA87ULL
#define XP2 0xC2B2AE3D27D4EB4FULL
#define XP3 0x165667B19E3779F9ULL
#define XP4 0x85EBCA77C2B2AE63ULL
#define XP5 0x27D4EB2F165667C5ULL
__device__ __forceinline__ u64 rotl64d(u64 x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ u64 xxh64_round(u64 acc, u64 in) { return rotl64d(acc + in * XP2, 31) * XP1; }
__device__ __forceinline__ u64 xxh64_merge(u64 h, u64 v) { return (h ^ xxh64_round(0, v)) * XP1 + XP4; }
__device__ __forceinline__ u64 xxh64_words(const u64* w, int nw)
{
  if (nw == 4) {      // 32 bytes (Kmer<128>): one stripe through the four accumulators, nothing left over
    const u64 v1 = xxh64_round(XP1 + XP2, w[0]), v2 = xxh64_round(XP2, w[1]), v3 = xxh64_round(0, w[2]), v4 = xxh64_round(0ULL - XP1, w[3]);
    u64 h = rotl64d(v1, 1) + rotl64d(v2, 7) + rotl64d(v3, 12) + rotl64d(v4, 18);
    h = xxh64_merge(h, v1); h = xxh64_merge(h, v2); h = xxh64_merge(h, v3); h = xxh64_merge(h, v4);
    h += 32;
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    return h;
  }
  u64 h = XP5 + (u64)nw * 8;
  for (int i = 0; i < nw; i++) {
    h ^= rotl64d(w[i] * XP2, 31) * XP1;
    h = rotl64d(h, 27) * XP1 + XP4;
  }
  h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
  return h;
}

}  // namespace kmx
