// match.hip -- `kmx match` on the device: a set of k-mers held in a hash table built for membership at one look-up a base, and reads
// matched against it (include/kmx.h, sections "kset" and "match"; kmdiff's map-back, the read fetch of a k-mer GWAS, back_to_sequences).
// No reference counterpart in the kmtricks tree.  gfx950, wave64.
//
//   k_ks_build    a thread a key.  The key is checked (no bits from 2k upwards, key <= revcomp(key)) and put into the table: open
//                 addressing, linear, T = the power of two >= 2 n slots of 8 bytes, (tag << 32) | index, all ones for a free slot; the
//                 slot from the low bits of xxh64_words(key), the tag from its high 32.  atomicCAS(slot, FREE, mine): FREE -- the slot is
//                 this key's; else what the CAS found IS the look at the slot: an equal tag is confirmed word for word against the key
//                 of the index in it -- equal: atomicMin(slot, mine), the tags being equal the smaller index wins, so a key's slot ends
//                 with its least index whatever the schedule; unequal: the next slot.  A slot once taken keeps its key for good, so
//                 every instance of a key walks the same slots up to the one that holds it.
//   k_ks_ids      a look-up a key: ids[v] = the index in the slot of keys[v] (kmx_kset_copy_ids), and the count of v with ids[v] == v
//   k_mt_probe    a wave a tile of 64 positions, grid-stride; a lane a position.  q_tile_kmer_strand (kmer_dev.hpp) gives the canonical
//                 words and the strand, q_tile_query the read; a position whose k-mer does not end inside its read is skipped.  One
//                 look-up: the slot (8 bytes, one random load), and the key only behind an equal tag.  Per read of the tile one add each
//                 to n_kmers, hits and fwd and one atomicMin / atomicMax to first / last + 1 (q_tile_adds' ballot loop); the tile's hit
//                 ballot as one u64; with IDS the wave's ids as 256 contiguous bytes; with OCC equal ids of the wave combined before
//                 one u64 add each.
//   k_mt_cover    a wave a tile, grid-stride.  A hit at i covers i ... i + k - 1 and never leaves its read, so coverage is a dilation of
//                 the hit bits: covered(p) = OR of hit(p - d), d < k, over this tile's word and the two in front of it (k - 1 <= 126),
//                 by log-step shifts of the 192 bits (wave-uniform); then one add of popcount(covered & the lanes of read q) per read
//                 of the tile.  A tile without a covered base reads no offsets.
//   k_mt_init / k_mt_last   the records' start values (first = 0xFFFFFFFF, the others 0); last + 1 -> last (0 -> 0xFFFFFFFF)
// No kernel waits on another workgroup: any grid is a correct one.  Every device loop is bounded by T, by 64 or by the tiles.  Every index
// taken from a slot is tested (< n) before it becomes an address.  The launch knobs are this file's own: KMX_MATCH_CUS, KMX_MATCH_GRID
// and KMX_MATCH_HASH_BITS.
#include "matrix_host.hpp"
#include "seqquery_host.hpp"
#include "kmer_dev.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 KS_NONE = 0xFFFFFFFFu;       // no id
constexpr u64 KS_FREE = ~0ull;             // a free slot (an index is below 2^31: no taken slot is all ones)
constexpr u32 KS_TILE = 256;               // threads of a workgroup
constexpr u32 KS_WGS_PER_CU = 16;
constexpr u32 KS_MAX_GRID = 1u << 16;      // workgroups of a launch: the kernels stride over their work
enum { KS_ST_HIGH = 1, KS_ST_NONCANON = 2, KS_ST_BOUND = 8 };

static_assert(sizeof(kmx_kset_task) == 32, "kmx_kset_task is 32 bytes");
static_assert(sizeof(kmx_match_task) == 56, "kmx_match_task is 56 bytes");
static_assert(sizeof(kmx_match_rec) == 24, "kmx_match_rec is 24 bytes");

// ---- 2-bit key arithmetic: k digits in KW words, low word first (as unitigs.hip's) ------------------------------------------------
template <int KW> __device__ __forceinline__ u64 ks_top_mask(u32 k) { const u32 d = k - 32u * (KW - 1); return d >= 32 ? ~0ull : (1ull << (2 * d)) - 1ull; }
template <int KW> __device__ __forceinline__ Key<KW> ks_load(const u64* __restrict__ keys, u64 v)
{
  Key<KW> x;
#pragma unroll
  for (int i = 0; i < KW; i++) x.w[i] = keys[v * KW + i];
  return x;
}
template <int KW> __device__ __forceinline__ Key<KW> ks_revcomp(const Key<KW>& x, u32 k)
{
  u64 r[KW + 1];
#pragma unroll
  for (int i = 0; i < KW; i++) r[i] = rev_digits64(x.w[KW - 1 - i]);
  r[KW] = 0;
  const u32 sh = 64u * KW - 2u * k;      // 0 ... 62, even
  Key<KW> y;
#pragma unroll
  for (int i = 0; i < KW; i++) y.w[i] = sh ? (r[i] >> sh) | (r[i + 1] << (64 - sh)) : r[i];
#pragma unroll
  for (int i = 0; i < KW; i++) y.w[i] ^= 0xAAAAAAAAAAAAAAAAull;
  y.w[KW - 1] &= ks_top_mask<KW>(k);
  return y;
}
// keep: the hash bits that stay; the others are SET, for slot and tag alike (KMX_MATCH_HASH_BITS; all ones: nothing changes)
template <int KW> __device__ __forceinline__ u64 ks_hash(const Key<KW>& x, u64 keep) { return (xxh64_words(x.w, KW) & keep) | ~keep; }

// the id of x, or KS_NONE: the walk ends at the first free slot (the table is at most half full), after T slots at the latest.
// confirmed: += the keys read behind an equal tag
template <int KW>
__device__ __forceinline__ u32 ks_find(const u64* __restrict__ keys, u32 n, const u64* __restrict__ table, u64 tmask, u64 keep, const Key<KW>& x, u32& confirmed)
{
  const u64 h = ks_hash<KW>(x, keep);
  const u32 tag = (u32)(h >> 32);
  u64 slot = h & tmask;
  for (u64 probes = 0; probes <= tmask; probes++) {
    const u64 e = table[slot];
    if (e == KS_FREE) return KS_NONE;
    if ((u32)(e >> 32) == tag) {
      const u32 u = (u32)e;
      if (u < n) { confirmed++; if (key_eq<KW>(ks_load<KW>(keys, u), x)) return u; }
    }
    slot = (slot + 1) & tmask;
  }
  return KS_NONE;
}

// ---- the set -----------------------------------------------------------------------------------------------------------------------
template <int KW>
__global__ __launch_bounds__(KS_TILE)
void k_ks_build(const u64* __restrict__ keys, u32 n, u32 k, unsigned long long* __restrict__ table, u64 tmask, u64 keep, u32* __restrict__ status)
{
  for (u64 v = (u64)blockIdx.x * KS_TILE + threadIdx.x; v < n; v += (u64)gridDim.x * KS_TILE) {
    const Key<KW> x = ks_load<KW>(keys, v);
    u32 bad = 0;
    if (x.w[KW - 1] & ~ks_top_mask<KW>(k)) bad |= KS_ST_HIGH;
    else if (key_less<KW>(ks_revcomp<KW>(x, k), x)) bad |= KS_ST_NONCANON;
    if (!bad) {
      const u64 h = ks_hash<KW>(x, keep);
      const u32 tag = (u32)(h >> 32);
      const u64 mine = ((u64)tag << 32) | (u64)v;
      u64 slot = h & tmask;
      bool placed = false;
      for (u64 probes = 0; probes <= tmask; probes++) {
        const u64 prev = atomicCAS(&table[slot], (unsigned long long)KS_FREE, (unsigned long long)mine);
        if (prev == KS_FREE) { placed = true; break; }
        if ((u32)(prev >> 32) == tag) {
          const u32 u = (u32)prev;
          if (u < n && key_eq<KW>(ks_load<KW>(keys, u), x)) { atomicMin(&table[slot], (unsigned long long)mine); placed = true; break; }
        }
        slot = (slot + 1) & tmask;
      }
      if (!placed) bad |= KS_ST_BOUND;
    }
    if (bad) atomicOr(status, bad);
  }
}

// ids: null, or n u32; n_distinct: null, or the counter of the indices that are their own id
template <int KW>
__global__ __launch_bounds__(KS_TILE)
void k_ks_ids(const u64* __restrict__ keys, u32 n, const u64* __restrict__ table, u64 tmask, u64 keep, u32* __restrict__ ids, u32* __restrict__ n_distinct)
{
  u32 own = 0, confirmed = 0;
  for (u64 v = (u64)blockIdx.x * KS_TILE + threadIdx.x; v < n; v += (u64)gridDim.x * KS_TILE) {
    const u32 id = ks_find<KW>(keys, n, table, tmask, keep, ks_load<KW>(keys, v), confirmed);
    if (ids) ids[v] = id;
    own += id == (u32)v;
  }
  if (n_distinct) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) own += (u32)__shfl_xor((int)own, off);      // (every lane of the wave is here)
    if ((threadIdx.x & 63u) == 0 && own) atomicAdd(n_distinct, own);
  }
}

// ---- the reads ---------------------------------------------------------------------------------------------------------------------
struct MtRec { u32 n_kmers, hits, fwd, covered, first, last; };      // kmx_match_rec; last holds last + 1 until k_mt_last
enum { MT_KMERS = 0, MT_HITS = 1, MT_CONFIRMED = 2 };                // the call's u64 totals

__global__ __launch_bounds__(KS_TILE)
void k_mt_init(u32* __restrict__ recs, u64 n_words)
{
  for (u64 i = (u64)blockIdx.x * KS_TILE + threadIdx.x; i < n_words; i += (u64)gridDim.x * KS_TILE) recs[i] = i % 6 == 4 ? 0xFFFFFFFFu : 0u;
}
__global__ __launch_bounds__(KS_TILE)
void k_mt_last(MtRec* __restrict__ recs, u32 n_seqs)
{
  for (u64 q = (u64)blockIdx.x * KS_TILE + threadIdx.x; q < n_seqs; q += (u64)gridDim.x * KS_TILE) recs[q].last -= 1u;
}

template <int KW>
__global__ __launch_bounds__(KS_TILE)
void k_mt_probe(const char* __restrict__ bases, const u64* __restrict__ offsets, u32 n_seqs, u64 n_bases, u32 n_tiles, int k, const u64* __restrict__ keys,
                u32 n, const u64* __restrict__ table, u64 tmask, u64 keep, MtRec* __restrict__ recs, u64* __restrict__ hitbits, u32* __restrict__ ids,
                unsigned long long* __restrict__ occ, unsigned long long* __restrict__ totals)
{
  const int lane = threadIdx.x & 63;
  const u32 wave = (blockIdx.x * KS_TILE + threadIdx.x) >> 6, n_waves = (gridDim.x * KS_TILE) >> 6;
  const QWalk wk = q_walk(k, 0);      // (no minimizer here: k, klo and khi are all that is read)
  u64 t_kmers = 0, t_hits = 0;
  u32 confirmed = 0, qs = 0;
  for (u32 t = wave; t < n_tiles; t += n_waves) {      // (uniform over the wave)
    const u64 t0 = (u64)t * 64, pos = t0 + lane;
    Key<KW> c; bool fw;
    const bool whole = q_tile_kmer_strand<KW>(bases, n_bases, pos, lane, wk, c.w, fw);
    const u32 q = q_tile_query(offsets, n_seqs, qs, t0, pos);
    qs = (u32)__shfl((int)q, 63);
    bool valid = pos < n_bases && whole;
    u64 start = 0;
    if (valid) { start = offsets[q]; valid = pos >= start && pos + (u64)k <= offsets[q + 1]; }
    const u32 id = valid && n ? ks_find<KW>(keys, n, table, tmask, keep, c, confirmed) : KS_NONE;
    const bool hit = id != KS_NONE;
    const u64 vb = __ballot(valid), hb = __ballot(hit), fb = __ballot(hit && fw);
    if (lane == 0) hitbits[t] = hb;
    if (ids && pos < n_bases) ids[pos] = id;
    t_kmers += (u64)__popcll(vb); t_hits += (u64)__popcll(hb);
    u64 vm = vb;
    while (vm) {      // one add per read of the tile and field
      const int l = __builtin_ctzll(vm);
      const u32 qq = (u32)__shfl((int)q, l);
      const u64 same = __ballot(valid && q == qq), hs = same & hb, fs = same & fb;
      if (lane == l) {
        atomicAdd(&recs[qq].n_kmers, (u32)__popcll(same));
        if (hs) {
          const u64 rel = t0 - start;      // (the read's start is at or in front of every one of its valid positions)
          atomicAdd(&recs[qq].hits, (u32)__popcll(hs));
          if (fs) atomicAdd(&recs[qq].fwd, (u32)__popcll(fs));
          atomicMin(&recs[qq].first, (u32)(rel + (u64)__builtin_ctzll(hs)));
          atomicMax(&recs[qq].last, (u32)(rel + 63u - (u64)__builtin_clzll(hs)) + 1u);
        }
      }
      vm &= ~same;
    }
    if (occ) {
      u64 hm = hb;
      while (hm) {      // equal ids of the wave: one add
        const int l = __builtin_ctzll(hm);
        const u32 jj = (u32)__shfl((int)id, l);
        const u64 same = __ballot(hit && id == jj);
        if (lane == l) atomicAdd(&occ[jj], (unsigned long long)__popcll(same));
        hm &= ~same;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) confirmed += (u32)__shfl_xor((int)confirmed, off);
  if (lane == 0) {
    if (t_kmers) atomicAdd(&totals[MT_KMERS], (unsigned long long)t_kmers);
    if (t_hits) atomicAdd(&totals[MT_HITS], (unsigned long long)t_hits);
    if (confirmed) atomicAdd(&totals[MT_CONFIRMED], (unsigned long long)confirmed);
  }
}

// the 192 bits (w0 low) shifted up by s, 1 <= s <= 64
__device__ __forceinline__ void mt_shl192(u64& w0, u64& w1, u64& w2, u32 s)
{
  if (s == 64) { w2 = w1; w1 = w0; w0 = 0; }
  else { w2 = (w2 << s) | (w1 >> (64 - s)); w1 = (w1 << s) | (w0 >> (64 - s)); w0 <<= s; }
}

__global__ __launch_bounds__(KS_TILE)
void k_mt_cover(const u64* __restrict__ offsets, u32 n_seqs, u64 n_bases, u32 n_tiles, u32 k, const u64* __restrict__ hitbits, MtRec* __restrict__ recs)
{
  const int lane = threadIdx.x & 63;
  const u32 wave = (blockIdx.x * KS_TILE + threadIdx.x) >> 6, n_waves = (gridDim.x * KS_TILE) >> 6;
  u32 qs = 0;
  for (u32 t = wave; t < n_tiles; t += n_waves) {      // (uniform over the wave)
    u64 w2 = hitbits[t], w1 = t >= 1 ? hitbits[t - 1] : 0ull, w0 = t >= 2 ? hitbits[t - 2] : 0ull;
    if (!(w0 | w1 | w2)) continue;
    u32 span = 1;      // (w0, w1, w2) holds the OR over `span` shifts
    while (2 * span <= k) { u64 a = w0, b = w1, c = w2; mt_shl192(a, b, c, span); w0 |= a; w1 |= b; w2 |= c; span *= 2; }      // span <= 64
    if (span < k) { u64 a = w0, b = w1, c = w2; mt_shl192(a, b, c, k - span); w0 |= a; w1 |= b; w2 |= c; }                  // k - span < span
    const u64 cov = w2;
    if (!cov) continue;
    const u64 t0 = (u64)t * 64, pos = t0 + lane;
    const u32 q = q_tile_query(offsets, n_seqs, qs, t0, pos);
    qs = (u32)__shfl((int)q, 63);
    const bool mine = (cov >> lane) & 1ull;      // (a covered base lies inside the read of its hit: pos < n_bases)
    u64 cm = __ballot(mine);
    while (cm) {      // one add per read of the tile
      const int l = __builtin_ctzll(cm);
      const u32 qq = (u32)__shfl((int)q, l);
      const u64 same = __ballot(mine && q == qq);
      if (lane == l) atomicAdd(&recs[qq].covered, (u32)__popcll(same));
      cm &= ~same;
    }
  }
}
// ---- end of the kernels -------------------------------------------------------------------------------------------------------------

static u32 ks_cus(const kmx_ctx* ctx) { return (u32)std::max(kmx_env_cus("KMX_MATCH_CUS", ctx), 1); }
static u32 ks_grid(const kmx_ctx* ctx, u64 items)      // items: threads' worth of work
{
  const u64 planned = std::min<u64>((u64)ks_cus(ctx) * KS_WGS_PER_CU, KS_MAX_GRID);
  return (u32)std::min<u64>(std::max<u64>((items + KS_TILE - 1) / KS_TILE, 1), kmx_env_grid("KMX_MATCH_GRID", planned));
}
// KMX_MATCH_HASH_BITS=b, 0 <= b <= 63: the low b bits of every hash stay, all the others are set
static u64 ks_keep()
{
  const long b = kmx_env_int("KMX_MATCH_HASH_BITS");
  return b >= 0 && b <= 63 ? (1ull << b) - 1ull : ~0ull;
}
static u64 ks_table_slots(u64 n) { u64 t = 2; while (t < 2 * n) t <<= 1; return t; }

}  // namespace kmx

using namespace kmx;

#define KS_KW(kw, F, ...)                                                    \
  do {                                                                       \
    switch (kw) {                                                            \
      case 1: hipLaunchKernelGGL(F<1>, __VA_ARGS__); break;                  \
      case 2: hipLaunchKernelGGL(F<2>, __VA_ARGS__); break;                  \
      case 3: hipLaunchKernelGGL(F<3>, __VA_ARGS__); break;                  \
      default: hipLaunchKernelGGL(F<4>, __VA_ARGS__); break;                 \
    }                                                                        \
  } while (0)

// ---- C ABI: kset ----------------------------------------------------------------------------------------------------------------------
struct kmx_kset : MatResult {      // n_rows: n; row_bytes: 8 * key_words; h_tot: n_distinct and the status word on their way down
  u32 k = 0, kw = 0;
  u64 tmask = 0, hkeep = ~0ull;    // hkeep: as the table was built (a match call must hash as the build did)
  u64* d_keys = nullptr;           // the set's own copy of the keys
  u64* d_table = nullptr;
};

static int kset_check(kmx_ctx* ctx, const kmx_kset_task* T, const char* who)
{
  const MatCheck c{ctx, who};
  if (T->kmer_size < 8 || T->kmer_size > 127) return c.no(KMX_E_INVAL, ": kmer_size must be 8 ... 127");
  if (T->key_words != (T->kmer_size + 31) / 32) return c.no(KMX_E_INVAL, ": key_words must be ceil(kmer_size / 32)");
  int rc;
  if ((rc = c.flags(T->flags, 0))) return rc;
  if (T->n && !T->keys) return c.no(KMX_E_INVAL, ": null keys");
  if (T->n > (1ull << 31)) return c.no(KMX_E_UNSUPPORTED, ": more than 2^31 k-mers in one set (an index and the free slot's mark must fit in 32 bits)");
  return KMX_OK;
}

static int kset_queue(kmx_ctx* ctx, const kmx_kset_task* T, kmx_kset* S, bool host, const char* who)
{
  hipStream_t st = ctx->stream;
  const u32 n = (u32)T->n, k = S->k = T->kmer_size, kw = S->kw = T->key_words;
  const u64 N = T->n, slots = ks_table_slots(N), kbytes = 8ull * kw * N;
  S->tmask = slots - 1; S->hkeep = ks_keep();
  if (!(S->h_tot = (u32*)S->pin(8))) return ctx->fail(KMX_E_NOMEM, "kmx_kset: host allocation failed");
  S->h_tot[0] = 0; S->h_tot[1] = 0;
  u32* d_tot = (u32*)S->tmp(8);      // [0] n_distinct, [1] the status word
  if (N) { S->d_keys = (u64*)S->keep(kbytes); S->d_table = (u64*)S->keep(8 * slots); }
  if (S->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_kset: device allocation failed (the set must fit one device)");
  if (N) {
    if (host) {
      mat_upload(S, S->d_keys, T->keys, kbytes);
      if (int rc = mat_uploads_done(S, who)) return rc;
    } else KMX_HIP(ctx, hipMemcpyAsync(S->d_keys, T->keys, kbytes, hipMemcpyDeviceToDevice, st));
  }
  int rc = mat_queue_head(S, 2);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_tot, 0, 8, st));
  if (N) {
    const u32 grid = ks_grid(ctx, N);
    KMX_HIP(ctx, hipMemsetAsync(S->d_table, 0xFF, 8 * slots, st));
    KS_KW(kw, k_ks_build, dim3(grid), dim3(KS_TILE), 0, st, (const u64*)S->d_keys, n, k, (unsigned long long*)S->d_table, S->tmask, S->hkeep, d_tot + 1);
    KMX_HIP(ctx, hipGetLastError());
    KS_KW(kw, k_ks_ids, dim3(grid), dim3(KS_TILE), 0, st, (const u64*)S->d_keys, n, (const u64*)S->d_table, S->tmask, S->hkeep, (u32*)nullptr, d_tot);
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(S, d_tot, d_tot + 1);
}

static int kset_call(kmx_ctx* ctx, const kmx_kset_task* task, kmx_kset** out, bool host, const char* who)
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, std::string(who) + ": null argument");
  *out = nullptr;
  int rc = kset_check(ctx, task, who);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  kmx_kset* S = new kmx_kset();
  S->ctx = ctx; S->name = "kmx_kset"; S->n_rows = task->n; S->row_bytes = 8ull * task->key_words; S->n_cols = 0;
  return mat_finish(kset_queue(ctx, task, S, host, who), S, out, host);
}
extern "C" int kmx_kset_dev(kmx_ctx* ctx, const kmx_kset_task* task, kmx_kset** out) { return kset_call(ctx, task, out, false, "kmx_kset_dev"); }
extern "C" int kmx_kset_host(kmx_ctx* ctx, const kmx_kset_task* task, kmx_kset** out) { return kset_call(ctx, task, out, true, "kmx_kset_host"); }

// the status word the build left, as the refusal every accessor and every match call repeats
static int kset_status(kmx_kset* S)
{
  const u32 s = S->h_tot[1];
  kmx_ctx* c = S->ctx;
  if (s & KS_ST_HIGH) return c->fail(KMX_E_INVAL, "kmx_kset: a key has bits set from 2 * kmer_size upwards");
  if (s & KS_ST_NONCANON) return c->fail(KMX_E_INVAL, "kmx_kset: a key is not canonical (it is greater than its reverse complement)");
  if (s) return c->fail(KMX_E_INTERNAL, "kmx_kset: a probe sequence reached its bound");
  return KMX_OK;
}
extern "C" int kmx_kset_wait(kmx_kset* S)
{
  if (!S) return KMX_E_INVAL;
  if (S->waited) return S->status != KMX_OK ? S->status : kset_status(S);
  const int rc = mat_wait(S);
  return rc != KMX_OK ? rc : kset_status(S);
}
extern "C" uint64_t kmx_kset_n(kmx_kset* S) { return S && kmx_kset_wait(S) == KMX_OK ? S->n_rows : 0; }
extern "C" uint64_t kmx_kset_n_distinct(kmx_kset* S) { return S && kmx_kset_wait(S) == KMX_OK ? S->h_tot[0] : 0; }
extern "C" uint32_t kmx_kset_kmer_size(kmx_kset* S) { return S && kmx_kset_wait(S) == KMX_OK ? S->k : 0; }
extern "C" int kmx_kset_copy_ids(kmx_kset* S, uint32_t* host_dst, uint64_t dst_entries)
{
  if (!S) return KMX_E_INVAL;
  int rc = kmx_kset_wait(S);
  if (rc != KMX_OK) return rc;
  kmx_ctx* ctx = S->ctx;
  const u64 N = S->n_rows;
  if (dst_entries < N) return ctx->fail(KMX_E_INVAL, "destination too small");
  if (!N) return KMX_OK;
  if (!host_dst) return ctx->fail(KMX_E_INVAL, "null destination");
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  u32* d_ids = (u32*)ctx->dalloc(4 * N);
  if (!d_ids) return ctx->fail(KMX_E_NOMEM, "kmx_kset_copy_ids: device allocation failed");
  KS_KW(S->kw, k_ks_ids, dim3(ks_grid(ctx, N)), dim3(KS_TILE), 0, ctx->stream, (const u64*)S->d_keys, (u32)N, (const u64*)S->d_table, S->tmask, S->hkeep, d_ids,
        (u32*)nullptr);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  rc = e != hipSuccess ? ctx->fail(KMX_E_HIP, std::string("kmx_kset_copy_ids: ") + hipGetErrorString(e)) : kmx_copy_to_host(ctx, host_dst, d_ids, 4 * N);
  ctx->dfree(d_ids);
  return rc;
}
extern "C" double kmx_kset_kernel_ms(kmx_kset* S) { return S && S->ev[0] && kmx_kset_wait(S) == KMX_OK ? mat_kernel_ms(S) : -1.0; }
extern "C" void kmx_kset_free(kmx_kset* S)
{
  if (!S) return;
  (void)hipSetDevice(S->ctx->device);
  (void)hipStreamSynchronize(S->ctx->stream);      // (a match call queued on the set reads its blocks)
  mat_free(S);
}

// ---- C ABI: match -----------------------------------------------------------------------------------------------------------------------
struct kmx_match_result : MatResult {      // n_rows: n_seqs; h_tot: the three u64 totals on their way down
  u64 n_bases = 0, n_keys = 0;
  u32 kw = 0, flags = 0;
  MtRec* d_recs = nullptr;
  u32* d_ids = nullptr;                     // null without KMX_MATCH_IDS
  u64* d_occ = nullptr;                     // the table the call adds to, its own or the caller's; null without KMX_MATCH_OCC
  const u64* totals() const { return (const u64*)h_tot; }
};

static int match_check(kmx_ctx* ctx, const kmx_match_task* K, const char* who)
{
  const SeqCheck c{ctx, who};
  int rc;
  if (!K->set) return c.no(KMX_E_INVAL, ": null set");
  if (K->set->ctx != ctx) return c.no(KMX_E_INVAL, ": the set belongs to another context");
  if (K->flags & ~(KMX_MATCH_IDS | KMX_MATCH_OCC)) return c.no(KMX_E_INVAL, ": unknown flag bits");
  if ((rc = c.reads(K->offsets, K->n_seqs, K->bases))) return rc;
  if (K->occ && !(K->flags & KMX_MATCH_OCC)) return c.no(KMX_E_INVAL, ": an occ table without KMX_MATCH_OCC");
  return c.n_seqs(K->n_seqs);
}

// the kernels of one call, queued on ctx->stream; bases and offsets device pointers
static int match_queue(kmx_ctx* ctx, const kmx_match_task* K, kmx_match_result* R)
{
  hipStream_t st = ctx->stream;
  const kmx_kset* S = K->set;
  const u64 n_bases = R->n_bases, N = S->n_rows;
  const u32 n_seqs = (u32)K->n_seqs, n_tiles = (u32)((n_bases + 63) / 64);
  const bool want_ids = K->flags & KMX_MATCH_IDS, want_occ = K->flags & KMX_MATCH_OCC;
  R->kw = S->kw; R->flags = K->flags; R->n_keys = N;
  if (!(R->h_tot = (u32*)R->pin(24))) return ctx->fail(KMX_E_NOMEM, "kmx_match: host allocation failed");
  memset(R->h_tot, 0, 24);
  u64* d_totals = (u64*)R->tmp(24);
  u64* d_hitbits = (u64*)R->tmp(8ull * std::max(n_tiles, 1u));
  R->d_recs = (MtRec*)R->keep(24ull * std::max(n_seqs, 1u));
  if (want_ids) R->d_ids = (u32*)R->keep(4 * std::max<u64>(n_bases, 1));
  u64* occ_own = want_occ && !K->occ ? (u64*)R->keep(8 * std::max<u64>(N, 1)) : nullptr;
  R->d_occ = !want_occ ? nullptr : K->occ ? (u64*)K->occ : occ_own;
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_match: device allocation failed (send the reads in batches)");
  int rc = mat_queue_head(R, 3);      // ev: start, behind the probe, end
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_totals, 0, 24, st));
  if (occ_own && N) KMX_HIP(ctx, hipMemsetAsync(occ_own, 0, 8 * N, st));
  if (n_seqs) {
    hipLaunchKernelGGL(k_mt_init, dim3(ks_grid(ctx, 6ull * n_seqs)), dim3(KS_TILE), 0, st, (u32*)R->d_recs, 6ull * n_seqs);
    KMX_HIP(ctx, hipGetLastError());
  }
  const u32 g_tiles = ks_grid(ctx, 64ull * n_tiles);
  if (n_tiles) {
    KS_KW(S->kw, k_mt_probe, dim3(g_tiles), dim3(KS_TILE), 0, st, K->bases, (const u64*)K->offsets, n_seqs, n_bases, n_tiles, (int)S->k, (const u64*)S->d_keys,
          (u32)N, (const u64*)S->d_table, S->tmask, S->hkeep, R->d_recs, d_hitbits, R->d_ids, (unsigned long long*)R->d_occ, (unsigned long long*)d_totals);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[1], st));
  if (n_tiles) {
    hipLaunchKernelGGL(k_mt_cover, dim3(g_tiles), dim3(KS_TILE), 0, st, (const u64*)K->offsets, n_seqs, n_bases, n_tiles, S->k, (const u64*)d_hitbits, R->d_recs);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (n_seqs) {
    hipLaunchKernelGGL(k_mt_last, dim3(ks_grid(ctx, n_seqs)), dim3(KS_TILE), 0, st, R->d_recs, n_seqs);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[2], st));
  KMX_HIP(ctx, hipMemcpyAsync(R->h_tot, d_totals, 24, hipMemcpyDeviceToHost, st));
  KMX_HIP(ctx, hipEventCreateWithFlags(&R->ev_done, hipEventDisableTiming));
  KMX_HIP(ctx, hipEventRecord(R->ev_done, st));
  return KMX_OK;
}

static int match_call(kmx_ctx* ctx, const kmx_match_task* task, kmx_match_result** out, bool host, const char* who)
{
  u64 n_bases = 0;
  int rc = seq_args(ctx, task, out, who);
  if (rc == KMX_OK) rc = match_check(ctx, task, who);
  if (rc == KMX_OK) rc = kmx_kset_wait((kmx_kset*)task->set);      // (a data error of the set is this call's)
  if (rc == KMX_OK) rc = seq_n_bases(ctx, task->offsets, task->n_seqs, host, who, &n_bases);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  kmx_match_result* R = new kmx_match_result();
  R->ctx = ctx; R->name = "kmx_match"; R->n_rows = task->n_seqs; R->n_bases = n_bases;
  kmx_match_task dt = *task;
  if (host) {      // the blocks go back at wait
    dt.bases = (const char*)mat_upload_tmp(R, task->bases, n_bases);
    dt.offsets = (const uint64_t*)mat_upload_tmp(R, task->offsets, 8 * (task->n_seqs + 1));
    rc = R->nomem ? ctx->fail(KMX_E_NOMEM, std::string(who) + ": upload allocation failed (send the reads in batches)") : mat_uploads_done(R, who);
  }
  if (rc == KMX_OK) rc = match_queue(ctx, &dt, R);
  return mat_finish(rc, R, out, host);
}
extern "C" int kmx_match_dev(kmx_ctx* ctx, const kmx_match_task* task, kmx_match_result** out) { return match_call(ctx, task, out, false, "kmx_match_dev"); }
extern "C" int kmx_match_host(kmx_ctx* ctx, const kmx_match_task* task, kmx_match_result** out) { return match_call(ctx, task, out, true, "kmx_match_host"); }

extern "C" int kmx_match_result_wait(kmx_match_result* R) { return mat_wait(R); }
extern "C" uint64_t kmx_match_result_n_seqs(const kmx_match_result* R) { return R ? R->n_rows : 0; }
extern "C" uint64_t kmx_match_result_n_bases(const kmx_match_result* R) { return R ? R->n_bases : 0; }
extern "C" int kmx_match_result_copy_recs(kmx_match_result* R, kmx_match_rec* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_recs, R->n_rows, 24) : KMX_E_INVAL; }
extern "C" int kmx_match_result_copy_ids(kmx_match_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_ids, R->n_bases, 4, "kmx_match_result_copy_ids: the call was made without KMX_MATCH_IDS") : KMX_E_INVAL; }
extern "C" uint64_t* kmx_match_result_occ_dev(kmx_match_result* R) { return R && mat_wait(R) == KMX_OK ? (uint64_t*)R->d_occ : nullptr; }
extern "C" int kmx_match_result_copy_occ(kmx_match_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_occ, R->n_keys, 8, "kmx_match_result_copy_occ: the call was made without KMX_MATCH_OCC") : KMX_E_INVAL; }
extern "C" uint64_t kmx_match_result_total_kmers(kmx_match_result* R) { return R && mat_wait(R) == KMX_OK ? R->totals()[MT_KMERS] : 0; }
extern "C" uint64_t kmx_match_result_total_hits(kmx_match_result* R) { return R && mat_wait(R) == KMX_OK ? R->totals()[MT_HITS] : 0; }
extern "C" double kmx_match_result_kernel_ms(kmx_match_result* R) { return mat_kernel_ms(R); }
extern "C" int kmx_match_result_kernel_parts_ms(kmx_match_result* R, double* probe_ms, double* cover_ms) { return mat_kernel_parts_ms(R, {probe_ms, cover_ms}); }
extern "C" uint64_t kmx_match_result_algo_bytes(kmx_match_result* R)
{
  if (!R || mat_wait(R) != KMX_OK) return 0;
  const u64* t = R->totals();
  return R->n_bases + 8 * t[MT_KMERS] + 8ull * R->kw * t[MT_CONFIRMED] + 24 * R->n_rows + 16 * ((R->n_bases + 63) / 64) +
         (R->flags & KMX_MATCH_IDS ? 4 * R->n_bases : 0) + (R->flags & KMX_MATCH_OCC ? 8 * t[MT_HITS] : 0);
}
extern "C" void kmx_match_result_free(kmx_match_result* R) { mat_free(R); }
