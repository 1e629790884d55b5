// kmer_dev.hpp -- the device code that says what a k-mer's minimizer and window hash ARE, shared by the kernels that must agree on
// them: the split (superk.hip), the count path (count.hip) and the queries (query.hip, kquery.hip).  One definition each, no copies.
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

// ---- the walk over a stream of query sequences (query.hip, kquery.hip): tiles of 64 positions, a wave a run of tiles, a lane a position ----
constexpr u32 QK_BLOCK = 256;          // threads of a workgroup of the key / scatter walk: four chunks

// bit i of y -> bit 2i (i < 32)
__device__ __forceinline__ u64 spread32(u32 y) { return (u64)spread16(y & 0xFFFFu) | ((u64)spread16(y >> 16) << 32); }
// bits [32 w, 32 w + 32) of the 128 bits (lo, hi)
__device__ __forceinline__ u32 q_bits32(u64 lo, u64 hi, int w) { return w == 0 ? (u32)lo : w == 1 ? (u32)(lo >> 32) : w == 2 ? (u32)hi : (u32)(hi >> 32); }
// the low k bits of (lo, hi) in reverse order (bit i <- bit k - 1 - i), 1 <= k <= 127; the bits from k on are zero in and out
__device__ __forceinline__ void q_rev(u64 lo, u64 hi, int k, u64& rlo, u64& rhi)
{
  const u64 RL = __brevll(hi), RH = __brevll(lo);      // the 128 bits reversed: RH:RL
  const int sft = 128 - k;                             // 1 .. 127
  if (sft >= 64) { rlo = RH >> (sft - 64); rhi = 0; }
  else { rlo = (RL >> sft) | (RH << (64 - sft)); rhi = RH >> sft; }
}

// the query that holds position pos: the greatest q in [lo, hi) with offsets[q] <= pos (offsets[lo] <= pos < offsets[hi]; empty
// queries share their offset with the one behind them and are skipped)
__device__ __forceinline__ u32 q_query_of(const u64* __restrict__ offsets, u32 lo, u32 hi, u64 pos)
{
  while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (offsets[mid] <= pos) lo = mid; else hi = mid; }
  return lo;
}
// ... for the 64 positions of the tile at t0, given a query qs at or in front of position t0's: a gallop finds the first query behind the tile
__device__ __forceinline__ u32 q_tile_query(const u64* __restrict__ offsets, u32 n_seqs, u32 qs, u64 t0, u64 pos)
{
  const u64 last = t0 + 63;
  u32 step = 1, hi = qs + 1;
  while (hi < n_seqs && offsets[hi] <= last) { step <<= 1; hi = n_seqs - qs > step ? qs + step : n_seqs; }      // (uniform over the wave)
  return q_query_of(offsets, qs, hi, pos);
}

struct QChunks { u32 n_tiles, n_chunks, tiles_per_chunk; };

// what a walk needs of (k, m), worked out once a wave
struct QWalk { int k, m, nbm; u32 mmask; u64 klo, khi; };
__device__ __forceinline__ QWalk q_walk(int k, int m)
{
  QWalk w;
  w.k = k; w.m = m;
  w.nbm = k - m + 1;                               // m-mers of a k-mer: 1 .. 124
  w.mmask = (1u << m) - 1;
  w.klo = k >= 64 ? ~0ULL : (1ULL << k) - 1ULL; w.khi = k > 64 ? (1ULL << (k - 64)) - 1ULL : 0ULL;
  return w;
}

// the k-mer at position pos = tile + lane, by the whole wave: the bases of the tile and of the 192 behind it become ballot bit planes,
// a lane's k-mer is k bits of each plane at its own position.  -> cw: the canonical k-mer's words, mini: its minimizer (the window
// minimum of mmer_value); returns whether its k bases are all ACGT (cw and mini mean nothing otherwise)
template <int KW>
__device__ __forceinline__ bool q_tile_kmer(const char* __restrict__ bases, u64 n_bases, u64 pos, int lane, const QWalk& wk, u64 (&cw)[KW], u32& mini)
{
  const int k = wk.k, m = wk.m, nbm = wk.nbm;
  const u32 mmask = wk.mmask;
  const u64 klo = wk.klo, khi = wk.khi;
  u8 cc[4];
#pragma unroll
  for (int i = 0; i < 4; i++) cc[i] = pos + 64u * i < n_bases ? (u8)bases[pos + 64u * i] : (u8)'N';
  u64 I[3], A[4], B[4];
#pragma unroll
  for (int i = 0; i < 4; i++) { if (i < 3) I[i] = __ballot(!nt_valid(cc[i])); A[i] = __ballot((cc[i] >> 1) & 1); B[i] = __ballot((cc[i] >> 2) & 1); }
  auto fun = [&](u64 x, u64 y) { return lane ? (x >> lane) | (y << (64 - lane)) : x; };
  const u64 fi_lo = fun(I[0], I[1]), fi_hi = fun(I[1], I[2]);
  const u64 fa_lo = fun(A[0], A[1]), fa_hi = fun(A[1], A[2]), fa_2 = fun(A[2], A[3]);
  const u64 fb_lo = fun(B[0], B[1]), fb_hi = fun(B[1], B[2]), fb_2 = fun(B[2], B[3]);
  // ---- the minimizer: the minimum of the m-mer values at positions lane .. lane + nbm - 1 of the 192 at hand ----
  auto mval = [&](u64 a, u64 b) {      // the m-mer that starts at bit 0 of (a, b): base j is digit m-1-j
    const u32 y0 = __brev((u32)a & mmask) >> (32 - m), y1 = __brev((u32)b & mmask) >> (32 - m);
    return mmer_value(spread16(y0) | (spread16(y1) << 1), m);
  };
  u32 v0 = mval(fa_lo, fb_lo), v1 = mval(fa_hi, fb_hi), v2 = mval(fa_2, fb_2);      // positions lane, 64 + lane, 128 + lane
  int span = 1;                                                                      // v holds the minimum over `span` positions
#pragma unroll
  for (int d = 1; d <= 32; d <<= 1) {
    if (2 * d > nbm) break;                                                          // (uniform)
    const u32 n0 = min(v0, sk_at(v0, v1, d, lane)), n1 = min(v1, sk_at(v1, v2, d, lane)), n2 = min(v2, sk_at(v2, 0xFFFFFFFFu, d, lane));
    v0 = n0; v1 = n1; v2 = n2; span = 2 * d;
  }
  // (span <= nbm < 2 span, or span = 64 and nbm <= 124: two spans cover the window; the second starts nbm - span < 64 positions on)
  mini = nbm > span ? min(v0, sk_at(v0, v1, nbm - span, lane)) : v0;
  // ---- the canonical k-mer: digit i is base k - 1 - i (A0 C1 T2 G3: plane A the low bit, plane B the high one) ----
  const u64 a_lo = fa_lo & klo, a_hi = fa_hi & khi, b_lo = fb_lo & klo, b_hi = fb_hi & khi;
  u64 ra_lo, ra_hi, rb_lo, rb_hi;
  q_rev(a_lo, a_hi, k, ra_lo, ra_hi); q_rev(b_lo, b_hi, k, rb_lo, rb_hi);
  const u64 nb_lo = ~b_lo & klo, nb_hi = ~b_hi & khi;      // the reverse complement's digit i is base i ^ 2
  u64 f[KW], r[KW];
#pragma unroll
  for (int w = 0; w < KW; w++) {
    f[w] = spread32(q_bits32(ra_lo, ra_hi, w)) | (spread32(q_bits32(rb_lo, rb_hi, w)) << 1);
    r[w] = spread32(q_bits32(a_lo, a_hi, w)) | (spread32(q_bits32(nb_lo, nb_hi, w)) << 1);
  }
  bool less = false, decided = false;
#pragma unroll
  for (int w = KW - 1; w >= 0; w--) if (!decided && f[w] != r[w]) { less = f[w] < r[w]; decided = true; }
#pragma unroll
  for (int w = 0; w < KW; w++) cw[w] = less ? f[w] : r[w];
  return (fi_lo & klo) == 0 && (fi_hi & khi) == 0;
}

// q_tile_kmer's sibling for a walk that has no minimizer (match.hip): the canonical words alone, from the tile's bases and the 128 behind
// them, and the strand -- fwd: the read shows the canonical k-mer itself (a palindrome counts as forward).  Of wk only k, klo and khi
// are read.  Returns whether the k bases are all ACGT.
template <int KW>
__device__ __forceinline__ bool q_tile_kmer_strand(const char* __restrict__ bases, u64 n_bases, u64 pos, int lane, const QWalk& wk, u64 (&cw)[KW], bool& fwd)
{
  const int k = wk.k;
  const u64 klo = wk.klo, khi = wk.khi;
  u8 cc[3];
#pragma unroll
  for (int i = 0; i < 3; i++) cc[i] = pos + 64u * i < n_bases ? (u8)bases[pos + 64u * i] : (u8)'N';
  u64 I[3], A[3], B[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { I[i] = __ballot(!nt_valid(cc[i])); A[i] = __ballot((cc[i] >> 1) & 1); B[i] = __ballot((cc[i] >> 2) & 1); }
  auto fun = [&](u64 x, u64 y) { return lane ? (x >> lane) | (y << (64 - lane)) : x; };
  const u64 fi_lo = fun(I[0], I[1]), fi_hi = fun(I[1], I[2]);
  const u64 a_lo = fun(A[0], A[1]) & klo, a_hi = fun(A[1], A[2]) & khi, b_lo = fun(B[0], B[1]) & klo, b_hi = fun(B[1], B[2]) & khi;
  u64 ra_lo, ra_hi, rb_lo, rb_hi;
  q_rev(a_lo, a_hi, k, ra_lo, ra_hi); q_rev(b_lo, b_hi, k, rb_lo, rb_hi);
  const u64 nb_lo = ~b_lo & klo, nb_hi = ~b_hi & khi;
  u64 f[KW], r[KW];
#pragma unroll
  for (int w = 0; w < KW; w++) {
    f[w] = spread32(q_bits32(ra_lo, ra_hi, w)) | (spread32(q_bits32(rb_lo, rb_hi, w)) << 1);
    r[w] = spread32(q_bits32(a_lo, a_hi, w)) | (spread32(q_bits32(nb_lo, nb_hi, w)) << 1);
  }
  bool less = false, decided = false;
#pragma unroll
  for (int w = KW - 1; w >= 0; w--) if (!decided && f[w] != r[w]) { less = f[w] < r[w]; decided = true; }
#pragma unroll
  for (int w = 0; w < KW; w++) cw[w] = less ? f[w] : r[w];
  fwd = less || !decided;
  return (fi_lo & klo) == 0 && (fi_hi & khi) == 0;
}

// the tile's adds: one per partition of the tile to its (partition, chunk) counter, one per query to n_kmers[query]
__device__ __forceinline__ void q_tile_adds(bool valid, u32 part, u32 q, int lane, u32* __restrict__ hist, u32 n_chunks, u32 c, u32* __restrict__ n_kmers)
{
  u64 vm = __ballot(valid);
  while (vm) {      // one add per partition of the tile (neighbouring k-mers share their minimizer: a handful)
    const int l = __builtin_ctzll(vm);
    const u32 pp = (u32)__shfl((int)part, l);
    const u64 same = __ballot(valid && part == pp);
    if (lane == l) atomicAdd(&hist[(size_t)pp * n_chunks + c], (u32)__popcll(same));
    vm &= ~same;
  }
  vm = __ballot(valid);
  while (vm) {      // one add per query of the tile
    const int l = __builtin_ctzll(vm);
    const u32 qq = (u32)__shfl((int)q, l);
    const u64 same = __ballot(valid && q == qq);
    if (lane == l) atomicAdd(&n_kmers[qq], (u32)__popcll(same));
    vm &= ~same;
  }
}

}  // namespace kmx
