// unitigs.hip -- `kmx unitigs` on the device: the compacted de Bruijn graph of a set of distinct canonical k-mers (include/kmx.h, section
// "unitigs"; what MUSET asks of ggcat behind `kmat_tools filter`, what kmdiff does when it merges its significant k-mers).  No reference
// counterpart in the kmtricks tree.  gfx950, wave64.
//
//   k_ug_table    a thread a node.  The key is checked (no bits from 2k upwards, key <= revcomp(key)) and put into the table: open
//                 addressing, linear, T = the power of two >= 2 n u32 slots of node indices, start xxh64_words(key) & (T - 1);
//                 atomicCAS(slot, EMPTY, v): EMPTY -- the slot is v's; else the key of the node found is compared word for word --
//                 equal: a duplicate; unequal: the next slot.  A bad key raises a bit of the status word; nothing waits.
//   k_ug_cand     a thread a state a = 2 v + s (node v, side s).  The four extensions of the side are shifted, reverse-complemented,
//                 canonicalised and looked up: the present ones are counted (strings, not nodes); cand[a] = 2 u + t when there is one,
//                 it is another node and neither node is its own reverse complement.  4 dependent random reads a state: the hot path.
//   k_ug_link     link[a] = cand[a] when cand[cand[a]] == a; the state's first tuple for the ranking: (pointer, hops, end, least node).
//   k_ug_jump     pointer doubling over the 2 n states, from one buffer into the other, R = bit_length(n - 1) + 1 launches fixed on the
//                 host.  next(a) = link[a] ^ 1: enter u at side t, leave it through the other.  A state that has reached a state without
//                 a link is through (pointer NONE) and knows that end, its hops to it and the least node index on the way.  A state
//                 whose pointer is live after R rounds lies on a cycle and has been round it: its least index is the cycle's.
//   k_ug_paths    a thread a node of a path: from the ends its two states reached, the two candidate first k-mers; the smaller one's
//                 end is the unitig's start, the node's hops to it its position.
//   k_ug_cycles   a thread a node: the one whose state 2 v + 1 is live with v the cycle's least index walks the cycle, once for the least
//                 key, once from there to write position and orientation -- at most 2 n steps, then the status word is raised.
//   k_ug_flag     start nodes (position 0) and their unitigs' k-mers counted per tile of 256 nodes; launch_filter_scan over both;
//   k_ug_number   a start node's rank is its unitig: start, len, circ, seq_off;   k_ug_ids   unitig[v] = rank[start of v], seq_off[U];
//   k_ug_emit     (behind the wait, when the sequences are first asked for: U is known then) a node writes one base, a start node k.
// No kernel waits on another workgroup: any grid is a correct one.  Every device loop is bounded by T, by 2 n or by R.
// Every index taken from the table, cand, link, a state tuple, start-of or rank is tested (< n, < 2 n) before it becomes an address, so bad
// input (duplicates, keys that are not canonical) leaves the kernels behind the table pass inside their arrays: they run, and the status
// word refuses their results.  The launch knobs are this file's own: KMX_UNITIG_CUS, KMX_UNITIG_GRID and KMX_UNITIG_HASH_BITS.
#include "matrix_host.hpp"
#include "kmer_dev.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 UG_NONE = 0xFFFFFFFFu;      // a free slot; no candidate, no link, no pointer (states are < 2 n <= 2^32 - 4)
constexpr u32 UG_TILE = 256;              // threads of a workgroup; nodes of a numbering tile
constexpr u32 UG_WGS_PER_CU = 16;
constexpr u32 UG_MAX_GRID = 1u << 16;     // workgroups of a launch: the kernels stride over their work
enum { UG_ST_HIGH = 1, UG_ST_NONCANON = 2, UG_ST_DUP = 4, UG_ST_BOUND = 8 };

static_assert(sizeof(kmx_unitigs_task) == 32, "kmx_unitigs_task is 32 bytes");

// ---- 2-bit key arithmetic: k digits in KW words, low word first ------------------------------------------------------------------
template <int KW> __device__ __forceinline__ u64 ug_top_mask(u32 k) { const u32 d = k - 32u * (KW - 1); return d >= 32 ? ~0ull : (1ull << (2 * d)) - 1ull; }
template <int KW> __device__ __forceinline__ Key<KW> ug_load(const u64* __restrict__ keys, u64 v)
{
  Key<KW> x;
#pragma unroll
  for (int i = 0; i < KW; i++) x.w[i] = keys[v * KW + i];
  return x;
}
template <int KW> __device__ __forceinline__ Key<KW> ug_revcomp(const Key<KW>& x, u32 k)
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
  y.w[KW - 1] &= ug_top_mask<KW>(k);
  return y;
}
// x[1:] + c
template <int KW> __device__ __forceinline__ Key<KW> ug_ext_right(const Key<KW>& x, u32 k, u32 c)
{
  Key<KW> y;
#pragma unroll
  for (int i = KW - 1; i > 0; i--) y.w[i] = (x.w[i] << 2) | (x.w[i - 1] >> 62);
  y.w[0] = (x.w[0] << 2) | c;
  y.w[KW - 1] &= ug_top_mask<KW>(k);
  return y;
}
// c + x[:-1]
template <int KW> __device__ __forceinline__ Key<KW> ug_ext_left(const Key<KW>& x, u32 k, u32 c)
{
  Key<KW> y;
#pragma unroll
  for (int i = 0; i < KW - 1; i++) y.w[i] = (x.w[i] >> 2) | (x.w[i + 1] << 62);
  y.w[KW - 1] = x.w[KW - 1] >> 2;
  y.w[KW - 1] |= (u64)c << (2 * ((k - 1) & 31u));      // (digit k - 1 lies in the top word: key_words = ceil(k / 32))
  return y;
}
// keep: the hash bits that stay; the others are SET (KMX_UNITIG_HASH_BITS; all ones: nothing changes)
template <int KW> __device__ __forceinline__ u64 ug_slot(const Key<KW>& x, u64 keep, u64 tmask) { return ((xxh64_words(x.w, KW) & keep) | ~keep) & tmask; }

// the node whose key is x, or UG_NONE; at most T probes, then the status word is raised
template <int KW>
__device__ __forceinline__ u32 ug_find(const u64* __restrict__ keys, u32 n, const u32* __restrict__ table, u64 tmask, u64 keep, const Key<KW>& x,
                                       u32* __restrict__ status)
{
  u64 slot = ug_slot<KW>(x, keep, tmask);
  for (u64 probes = 0; probes <= tmask; probes++) {
    const u32 u = table[slot];
    if (u == UG_NONE) return UG_NONE;
    if (u < n && key_eq<KW>(ug_load<KW>(keys, u), x)) return u;
    slot = (slot + 1) & tmask;
  }
  atomicOr(status, (u32)UG_ST_BOUND);
  return UG_NONE;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------
template <int KW>
__global__ __launch_bounds__(UG_TILE)
void k_ug_table(const u64* __restrict__ keys, u32 n, u32 k, u32* __restrict__ table, u64 tmask, u64 keep, u32* __restrict__ status)
{
  for (u64 v = (u64)blockIdx.x * UG_TILE + threadIdx.x; v < n; v += (u64)gridDim.x * UG_TILE) {
    const Key<KW> x = ug_load<KW>(keys, v);
    u32 bad = 0;
    if (x.w[KW - 1] & ~ug_top_mask<KW>(k)) bad |= UG_ST_HIGH;
    else if (key_less<KW>(ug_revcomp<KW>(x, k), x)) bad |= UG_ST_NONCANON;
    if (!bad) {
      u64 slot = ug_slot<KW>(x, keep, tmask);
      bool placed = false;
      for (u64 probes = 0; probes <= tmask; probes++) {
        const u32 prev = atomicCAS(&table[slot], UG_NONE, (u32)v);
        if (prev == UG_NONE) { placed = true; break; }
        if (prev < n && key_eq<KW>(ug_load<KW>(keys, prev), x)) { bad |= UG_ST_DUP; placed = true; break; }
        slot = (slot + 1) & tmask;
      }
      if (!placed) bad |= UG_ST_BOUND;
    }
    if (bad) atomicOr(status, bad);
  }
}

template <int KW>
__global__ __launch_bounds__(UG_TILE)
void k_ug_cand(const u64* __restrict__ keys, u32 n, u32 k, const u32* __restrict__ table, u64 tmask, u64 keep, u32* __restrict__ cand,
               u32* __restrict__ status)
{
  const u64 n_states = 2ull * n;
  for (u64 a = (u64)blockIdx.x * UG_TILE + threadIdx.x; a < n_states; a += (u64)gridDim.x * UG_TILE) {
    const u32 v = (u32)(a >> 1), s = (u32)(a & 1);
    const Key<KW> x = ug_load<KW>(keys, v);
    const bool pal_v = key_eq<KW>(ug_revcomp<KW>(x, k), x);
    u32 deg = 0, to = UG_NONE;
    bool pal_u = false;
    for (u32 c = 0; c < 4; c++) {
      const Key<KW> y = s ? ug_ext_right<KW>(x, k, c) : ug_ext_left<KW>(x, k, c);
      const Key<KW> ry = ug_revcomp<KW>(y, k);
      const bool fwd = !key_less<KW>(ry, y);      // y is its own canonical form: y == key(u)
      const u32 u = ug_find<KW>(keys, n, table, tmask, keep, fwd ? y : ry, status);
      if (u != UG_NONE) {
        deg++;
        // from side 1, y == key(u) enters u on side 0; from side 0, on side 1
        to = 2u * u + (s ? (fwd ? 0u : 1u) : (fwd ? 1u : 0u));
        pal_u = key_eq<KW>(y, ry);
      }
    }
    cand[a] = deg == 1 && (to >> 1) != v && !pal_v && !pal_u ? to : UG_NONE;
  }
}

// a state's tuple: x the state to jump to (NONE: through), y the hops so far, z the end (valid when through), w the least node index
__global__ __launch_bounds__(UG_TILE)
void k_ug_link(const u32* __restrict__ cand, u32 n, u32* __restrict__ link, uint4* __restrict__ st)
{
  const u64 n_states = 2ull * n;
  for (u64 a = (u64)blockIdx.x * UG_TILE + threadIdx.x; a < n_states; a += (u64)gridDim.x * UG_TILE) {
    const u32 b = cand[a];
    const u32 l = b < n_states && cand[b] == (u32)a ? b : UG_NONE;
    link[a] = l;
    st[a] = l == UG_NONE ? make_uint4(UG_NONE, 0u, (u32)a, (u32)(a >> 1)) : make_uint4(l ^ 1u, 1u, UG_NONE, (u32)(a >> 1));
  }
}

__global__ __launch_bounds__(UG_TILE)
void k_ug_jump(const uint4* __restrict__ in, uint4* __restrict__ out, u32 n)
{
  const u64 n_states = 2ull * n;
  for (u64 a = (u64)blockIdx.x * UG_TILE + threadIdx.x; a < n_states; a += (u64)gridDim.x * UG_TILE) {
    uint4 t = in[a];
    if (t.x < n_states) {
      const uint4 o = in[t.x];
      t.y += o.y; t.w = min(t.w, o.w);
      if (o.x == UG_NONE) { t.x = UG_NONE; t.z = o.z; } else t.x = o.x;
    }
    out[a] = t;
  }
}

// sof[v]: the start node of v's unitig; nlen[start]: its k-mers.  The nodes of a cycle are left to k_ug_cycles.
template <int KW>
__global__ __launch_bounds__(UG_TILE)
void k_ug_paths(const u64* __restrict__ keys, u32 n, u32 k, const uint4* __restrict__ st, u32* __restrict__ sof, u32* __restrict__ pos,
                u8* __restrict__ ori, u32* __restrict__ nlen)
{
  const u64 n_states = 2ull * n;
  for (u64 v = (u64)blockIdx.x * UG_TILE + threadIdx.x; v < n; v += (u64)gridDim.x * UG_TILE) {
    const uint4 t0 = st[2 * v], t1 = st[2 * v + 1];
    if (t0.x != UG_NONE || t1.x != UG_NONE || t0.z >= n_states || t1.z >= n_states) continue;
    // the traversal from an end leaves it through the side opposite the one without a link: read forward when that dead side is 0
    Key<KW> c0 = ug_load<KW>(keys, t0.z >> 1), c1 = ug_load<KW>(keys, t1.z >> 1);
    if (t0.z & 1u) c0 = ug_revcomp<KW>(c0, k);
    if (t1.z & 1u) c1 = ug_revcomp<KW>(c1, k);
    const u32 s = key_less<KW>(c1, c0) ? 1u : 0u;      // (equal: the single node, forward)
    const uint4 t = s ? t1 : t0;
    sof[v] = t.z >> 1; pos[v] = t.y; ori[v] = (u8)s;
    if (t.y == 0) nlen[v] = t0.y + t1.y + 1u;
  }
}

template <int KW>
__global__ __launch_bounds__(UG_TILE)
void k_ug_cycles(const u64* __restrict__ keys, u32 n, const uint4* __restrict__ st, const u32* __restrict__ link, u32* __restrict__ sof,
                 u32* __restrict__ pos, u8* __restrict__ ori, u32* __restrict__ nlen, u8* __restrict__ ncirc, u32* __restrict__ status)
{
  const u64 n_states = 2ull * n;
  for (u64 v = (u64)blockIdx.x * UG_TILE + threadIdx.x; v < n; v += (u64)gridDim.x * UG_TILE) {
    const uint4 t = st[2 * v + 1];
    if (t.x == UG_NONE || t.w != (u32)v) continue;      // not on a cycle, or not the cycle's least index
    // once round for the least key and the length
    const u32 a0 = (u32)(2 * v + 1);
    u32 a = a0, best = (u32)v, L = 0;
    Key<KW> kb = ug_load<KW>(keys, v);
    bool closed = false;
    for (u64 i = 0; i < n_states; i++) {
      const u32 w = a >> 1;
      const Key<KW> kw_ = ug_load<KW>(keys, w);
      if (key_less<KW>(kw_, kb)) { kb = kw_; best = w; }
      L++;
      const u32 l = link[a];
      if (l >= n_states) break;
      a = l ^ 1u;
      if (a == a0) { closed = true; break; }
    }
    if (!closed) { atomicOr(status, (u32)UG_ST_BOUND); continue; }
    // once more from the least key, read forward and left through side 1
    a = 2u * best + 1u;
    for (u32 i = 0; i < L; i++) {
      const u32 w = a >> 1;
      sof[w] = best; pos[w] = i; ori[w] = (u8)((a & 1u) ^ 1u);
      const u32 l = link[a];
      if (l >= n_states) { atomicOr(status, (u32)UG_ST_BOUND); break; }
      a = l ^ 1u;
    }
    nlen[best] = L; ncirc[best] = 1;
  }
}

__global__ __launch_bounds__(UG_TILE)
void k_ug_flag(const u32* __restrict__ pos, const u32* __restrict__ nlen, u32 n, u32* __restrict__ tile_cnt, u32* __restrict__ tile_len)
{
  __shared__ u32 s_len;
  const u64 n_tiles = ((u64)n + UG_TILE - 1) / UG_TILE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    if (threadIdx.x == 0) s_len = 0;
    const u64 v = t * UG_TILE + threadIdx.x;
    const bool flag = v < n && pos[v] == 0;
    const int c = __syncthreads_count(flag);
    u32 l = flag ? nlen[v] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) l += __shfl_xor(l, off);
    if ((threadIdx.x & 63u) == 0 && l) atomicAdd(&s_len, l);      // (LDS)
    __syncthreads();
    if (threadIdx.x == 0) { tile_cnt[t] = (u32)c; tile_len[t] = s_len; }
    __syncthreads();
  }
}

// tile_cnt / tile_len: scanned.  The start nodes' ranks are the unitig ids: ascending by start node
__global__ __launch_bounds__(UG_TILE)
void k_ug_number(const u32* __restrict__ pos, const u32* __restrict__ nlen, const u8* __restrict__ ncirc, u32 n, u32 k,
                 const u32* __restrict__ tile_cnt, const u32* __restrict__ tile_len, u32* __restrict__ rank, u32* __restrict__ start,
                 u32* __restrict__ len, u8* __restrict__ circ, u64* __restrict__ seq_off)
{
  __shared__ u32 s_c[UG_TILE / 64], s_l[UG_TILE / 64];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u64 n_tiles = ((u64)n + UG_TILE - 1) / UG_TILE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 v = t * UG_TILE + threadIdx.x;
    const bool flag = v < n && pos[v] == 0;
    const u32 l = flag ? nlen[v] : 0u;
    const u64 bal = __ballot(flag);
    const u32 incl = wave_incl_scan(l, (int)lane);
    if (lane == 63) { s_c[wave] = (u32)__popcll(bal); s_l[wave] = incl; }
    __syncthreads();
    u32 r = (u32)__popcll(bal & ((1ULL << lane) - 1ULL));
    u64 before = incl - l;
    for (u32 w = 0; w < wave; w++) { r += s_c[w]; before += s_l[w]; }
    if (flag) {
      const u64 u = (u64)tile_cnt[t] + r;
      if (u < n) {
        rank[v] = (u32)u; start[u] = (u32)v; len[u] = l; circ[u] = ncirc[v];
        seq_off[u] = (u64)tile_len[t] + before + u * (u64)(k - 1);
      }
    }
    __syncthreads();
  }
}

// n_unitigs: the scan's total, on the device
__global__ __launch_bounds__(UG_TILE)
void k_ug_ids(const u32* __restrict__ sof, const u32* __restrict__ rank, u32 n, u32 k, const u32* __restrict__ n_unitigs, u32* __restrict__ unitig,
              u64* __restrict__ seq_off)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) { const u64 U = min(*n_unitigs, n); seq_off[U] = (u64)n + U * (u64)(k - 1); }
  for (u64 v = (u64)blockIdx.x * UG_TILE + threadIdx.x; v < n; v += (u64)gridDim.x * UG_TILE) {
    const u32 s = sof[v];
    unitig[v] = s < n ? rank[s] : UG_NONE;
  }
}

// base j of the string of x read forward is digit k - 1 - j; read as its reverse complement, digit j ^ 2
template <int KW>
__global__ __launch_bounds__(UG_TILE)
void k_ug_emit(const u64* __restrict__ keys, u32 n, u32 k, u32 U, const u32* __restrict__ unitig, const u32* __restrict__ pos, const u8* __restrict__ ori,
               const u64* __restrict__ seq_off, u64 total, u8* __restrict__ seqs)
{
  for (u64 v = (u64)blockIdx.x * UG_TILE + threadIdx.x; v < n; v += (u64)gridDim.x * UG_TILE) {
    const u32 u = unitig[v];
    if (u >= U) continue;
    const Key<KW> x = ug_load<KW>(keys, v);
    const u32 p = pos[v], o = ori[v];
    const u64 off = seq_off[u];
    auto base = [&](u32 j) {
      const u32 d = o ? j : k - 1 - j;
      const u32 g = (u32)(x.w[d >> 5] >> (2 * (d & 31u))) & 3u;
      return (u8)((0x47544341u >> (8 * (o ? g ^ 2u : g))) & 0xFFu);      // "ACTG"
    };
    if (p == 0) { for (u32 j = 0; j < k; j++) if (off + j < total) seqs[off + j] = base(j); }
    else if (off + k - 1 + p < total) seqs[off + k - 1 + p] = base(k - 1);
  }
}
// ---- end of the kernels -------------------------------------------------------------------------------------------------------------

static u32 ug_cus(const kmx_ctx* ctx) { return (u32)std::max(kmx_env_cus("KMX_UNITIG_CUS", ctx), 1); }
static u32 ug_grid(const kmx_ctx* ctx, u64 items)
{
  const u64 planned = std::min<u64>((u64)ug_cus(ctx) * UG_WGS_PER_CU, UG_MAX_GRID);
  return (u32)std::min<u64>(std::max<u64>((items + UG_TILE - 1) / UG_TILE, 1), kmx_env_grid("KMX_UNITIG_GRID", planned));
}
// KMX_UNITIG_HASH_BITS=b, 0 <= b <= 63: the low b bits of every hash stay, all the others are set
static u64 ug_keep()
{
  const long b = kmx_env_int("KMX_UNITIG_HASH_BITS");
  return b >= 0 && b <= 63 ? (1ull << b) - 1ull : ~0ull;
}
static u64 ug_table_slots(u64 n) { u64 t = 2; while (t < 2 * n) t <<= 1; return t; }
static u64 ug_tiles(u64 n) { return (n + UG_TILE - 1) / UG_TILE; }
static u32 ug_rounds(u64 n) { u32 r = 1; for (u64 x = n ? n - 1 : 0; x; x >>= 1) r++; return r; }      // bit_length(n - 1) + 1

}  // namespace kmx

using namespace kmx;

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
struct kmx_unitigs_result : MatResult {      // n_rows: n; row_bytes: 8 * key_words; h_tot: U and the status word on their way down
  u32 k = 0, kw = 0, rounds = 0;
  u64* d_keys = nullptr;                     // the call's own copy of the keys: the sequences are made behind the wait
  u32 *d_unitig = nullptr, *d_pos = nullptr, *d_start = nullptr, *d_len = nullptr;
  u8 *d_ori = nullptr, *d_circ = nullptr, *d_seqs = nullptr;
  u64* d_seq_off = nullptr;
};

#define UG_KW(kw, F, ...)                                                    \
  do {                                                                       \
    switch (kw) {                                                            \
      case 1: hipLaunchKernelGGL(F<1>, __VA_ARGS__); break;                  \
      case 2: hipLaunchKernelGGL(F<2>, __VA_ARGS__); break;                  \
      case 3: hipLaunchKernelGGL(F<3>, __VA_ARGS__); break;                  \
      default: hipLaunchKernelGGL(F<4>, __VA_ARGS__); break;                 \
    }                                                                        \
  } while (0)

static int unitigs_check(kmx_ctx* ctx, const kmx_unitigs_task* T, const char* who)
{
  const MatCheck c{ctx, who};
  if (T->kmer_size < 8 || T->kmer_size > 127) return c.no(KMX_E_INVAL, ": kmer_size must be 8 ... 127");
  if (T->key_words != (T->kmer_size + 31) / 32) return c.no(KMX_E_INVAL, ": key_words must be ceil(kmer_size / 32)");
  int rc;
  if ((rc = c.flags(T->flags, 0))) return rc;
  if (T->n && !T->keys) return c.no(KMX_E_INVAL, ": null keys");
  if (T->n > 0x7FFFFFFEull) return c.no(KMX_E_UNSUPPORTED, ": more than 2^31 - 2 k-mers in one call (a state 2 v + s and the sentinel must fit in 32 bits)");
  return KMX_OK;
}

static int unitigs_queue(kmx_ctx* ctx, const kmx_unitigs_task* T, kmx_unitigs_result* R, bool host, const char* who)
{
  hipStream_t st = ctx->stream;
  const u32 n = (u32)T->n, k = R->k = T->kmer_size, kw = R->kw = T->key_words;
  const u64 N = n, slots = ug_table_slots(N), tiles = ug_tiles(N), kbytes = 8ull * kw * N;
  R->rounds = ug_rounds(N);
  if (!(R->h_tot = (u32*)R->pin(8))) return ctx->fail(KMX_E_NOMEM, "kmx_unitigs: host allocation failed");
  R->h_tot[0] = 0; R->h_tot[1] = 0;
  u32* d_tcnt = (u32*)R->tmp(4 * (tiles + 1));
  u32* d_tlen = (u32*)R->tmp(4 * (tiles + 1));
  u32* d_status = (u32*)R->tmp(4);
  u32 *d_table = nullptr, *d_cand = nullptr, *d_link = nullptr, *d_sof = nullptr, *d_nlen = nullptr, *d_rank = nullptr;
  uint4 *d_sa = nullptr, *d_sb = nullptr;
  u8* d_ncirc = nullptr;
  R->d_seq_off = (u64*)R->keep(8 * (N + 1));
  if (n) {
    d_table = (u32*)R->tmp(4 * slots); d_cand = (u32*)R->tmp(8 * N); d_link = (u32*)R->tmp(8 * N);
    d_sa = (uint4*)R->tmp(32 * N); d_sb = (uint4*)R->tmp(32 * N);
    d_sof = (u32*)R->tmp(4 * N); d_nlen = (u32*)R->tmp(4 * N); d_rank = (u32*)R->tmp(4 * N); d_ncirc = (u8*)R->tmp(N);
    R->d_keys = (u64*)R->keep(kbytes);
    R->d_unitig = (u32*)R->keep(4 * N); R->d_pos = (u32*)R->keep(4 * N); R->d_start = (u32*)R->keep(4 * N); R->d_len = (u32*)R->keep(4 * N);
    R->d_ori = (u8*)R->keep(N); R->d_circ = (u8*)R->keep(N);
  }
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_unitigs: device allocation failed");
  if (n) {
    if (host) {
      mat_upload(R, R->d_keys, T->keys, kbytes);
      if (int rc = mat_uploads_done(R, who)) return rc;
    } else KMX_HIP(ctx, hipMemcpyAsync(R->d_keys, T->keys, kbytes, hipMemcpyDeviceToDevice, st));
  }
  int rc = mat_queue_head(R, 5);      // ev: start, behind the table, behind the links, behind the ranking, end
  if (rc != KMX_OK) return rc;
  const u64* keys = R->d_keys;
  const u64 tmask = slots - 1, keep = ug_keep();
  const u32 g_nodes = ug_grid(ctx, N), g_states = ug_grid(ctx, 2 * N), g_tiles = (u32)std::min<u64>(std::max<u64>(tiles, 1), ug_grid(ctx, ~0ull >> 8));
  KMX_HIP(ctx, hipMemsetAsync(d_tcnt, 0, 4 * (tiles + 1), st));
  KMX_HIP(ctx, hipMemsetAsync(d_tlen, 0, 4 * (tiles + 1), st));
  KMX_HIP(ctx, hipMemsetAsync(d_status, 0, 4, st));
  if (n) {
    KMX_HIP(ctx, hipMemsetAsync(d_table, 0xFF, 4 * slots, st));
    UG_KW(kw, k_ug_table, dim3(g_nodes), dim3(UG_TILE), 0, st, keys, n, k, d_table, tmask, keep, d_status);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[1], st));
  if (n) {
    UG_KW(kw, k_ug_cand, dim3(g_states), dim3(UG_TILE), 0, st, keys, n, k, (const u32*)d_table, tmask, keep, d_cand, d_status);
    KMX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ug_link, dim3(g_states), dim3(UG_TILE), 0, st, (const u32*)d_cand, n, d_link, d_sa);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[2], st));
  if (n) {
    for (u32 r = 0; r < R->rounds; r++) {
      hipLaunchKernelGGL(k_ug_jump, dim3(g_states), dim3(UG_TILE), 0, st, (const uint4*)d_sa, d_sb, n);
      KMX_HIP(ctx, hipGetLastError());
      std::swap(d_sa, d_sb);
    }
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[3], st));
  if (n) {
    KMX_HIP(ctx, hipMemsetAsync(d_sof, 0xFF, 4 * N, st));
    KMX_HIP(ctx, hipMemsetAsync(R->d_pos, 0xFF, 4 * N, st));
    KMX_HIP(ctx, hipMemsetAsync(R->d_ori, 0, N, st));
    KMX_HIP(ctx, hipMemsetAsync(d_nlen, 0, 4 * N, st));
    KMX_HIP(ctx, hipMemsetAsync(d_ncirc, 0, N, st));
    UG_KW(kw, k_ug_paths, dim3(g_nodes), dim3(UG_TILE), 0, st, keys, n, k, (const uint4*)d_sa, d_sof, R->d_pos, R->d_ori, d_nlen);
    KMX_HIP(ctx, hipGetLastError());
    UG_KW(kw, k_ug_cycles, dim3(g_nodes), dim3(UG_TILE), 0, st, keys, n, (const uint4*)d_sa, (const u32*)d_link, d_sof, R->d_pos, R->d_ori, d_nlen, d_ncirc,
          d_status);
    KMX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ug_flag, dim3(g_tiles), dim3(UG_TILE), 0, st, (const u32*)R->d_pos, (const u32*)d_nlen, n, d_tcnt, d_tlen);
    KMX_HIP(ctx, hipGetLastError());
    KMX_HIP(ctx, launch_filter_scan(d_tcnt, (u32)tiles, st));
    KMX_HIP(ctx, launch_filter_scan(d_tlen, (u32)tiles, st));
    hipLaunchKernelGGL(k_ug_number, dim3(g_tiles), dim3(UG_TILE), 0, st, (const u32*)R->d_pos, (const u32*)d_nlen, (const u8*)d_ncirc, n, k, (const u32*)d_tcnt,
                       (const u32*)d_tlen, d_rank, R->d_start, R->d_len, R->d_circ, R->d_seq_off);
    KMX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ug_ids, dim3(g_nodes), dim3(UG_TILE), 0, st, (const u32*)d_sof, (const u32*)d_rank, n, k, (const u32*)(d_tcnt + tiles), R->d_unitig,
                       R->d_seq_off);
    KMX_HIP(ctx, hipGetLastError());
  } else KMX_HIP(ctx, hipMemsetAsync(R->d_seq_off, 0, 8, st));
  return mat_queue_tail(R, d_tcnt + tiles, d_status);
}

static int unitigs_call(kmx_ctx* ctx, const kmx_unitigs_task* task, kmx_unitigs_result** out, bool host, const char* who)
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, std::string(who) + ": null argument");
  *out = nullptr;
  int rc = unitigs_check(ctx, task, who);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  kmx_unitigs_result* R = new kmx_unitigs_result();
  R->ctx = ctx; R->name = "kmx_unitigs"; R->n_rows = task->n; R->row_bytes = 8ull * task->key_words; R->n_cols = 0;
  return mat_finish(unitigs_queue(ctx, task, R, host, who), R, out, host);
}

extern "C" int kmx_unitigs_dev(kmx_ctx* ctx, const kmx_unitigs_task* task, kmx_unitigs_result** out) { return unitigs_call(ctx, task, out, false, "kmx_unitigs_dev"); }
extern "C" int kmx_unitigs_host(kmx_ctx* ctx, const kmx_unitigs_task* task, kmx_unitigs_result** out) { return unitigs_call(ctx, task, out, true, "kmx_unitigs_host"); }

// the status word a call left, as the refusal every accessor repeats
static int unitigs_status(kmx_unitigs_result* R)
{
  const u32 s = R->h_tot[1];
  kmx_ctx* c = R->ctx;
  if (s & UG_ST_HIGH) return c->fail(KMX_E_INVAL, "kmx_unitigs: a key has bits set from 2 * kmer_size upwards");
  if (s & UG_ST_NONCANON) return c->fail(KMX_E_INVAL, "kmx_unitigs: a key is not canonical (it is greater than its reverse complement)");
  if (s & UG_ST_DUP) return c->fail(KMX_E_INVAL, "kmx_unitigs: a key occurs twice (the keys must be distinct)");
  if (s || R->h_tot[0] > R->n_rows) return c->fail(KMX_E_INTERNAL, "kmx_unitigs: a probe sequence or a cycle walk reached its bound");
  return KMX_OK;
}
extern "C" int kmx_unitigs_result_wait(kmx_unitigs_result* R)
{
  if (!R) return KMX_E_INVAL;
  if (R->waited) return R->status != KMX_OK ? R->status : unitigs_status(R);
  const int rc = mat_wait(R);
  if (rc != KMX_OK) return rc;
  return unitigs_status(R);
}
extern "C" uint64_t kmx_unitigs_result_n_unitigs(kmx_unitigs_result* R) { return kmx_unitigs_result_wait(R) == KMX_OK ? R->h_tot[0] : 0; }
extern "C" const uint32_t* kmx_unitigs_result_unitig_dev(kmx_unitigs_result* R) { return kmx_unitigs_result_wait(R) == KMX_OK ? R->d_unitig : nullptr; }
extern "C" uint64_t kmx_unitigs_result_seq_bytes(kmx_unitigs_result* R)
{ return kmx_unitigs_result_wait(R) == KMX_OK ? R->n_rows + (u64)R->h_tot[0] * (R->k - 1) : 0; }
static int unitigs_copy_out(kmx_unitigs_result* R, void* dst, uint64_t dst_entries, const void* src, u64 entries, u32 entry_bytes)
{
  const int rc = kmx_unitigs_result_wait(R);
  return rc != KMX_OK ? rc : mat_copy_out(R, dst, dst_entries, src, entries, entry_bytes);
}
extern "C" int kmx_unitigs_result_copy_unitig(kmx_unitigs_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? unitigs_copy_out(R, host_dst, dst_entries, R->d_unitig, R->n_rows, 4) : KMX_E_INVAL; }
extern "C" int kmx_unitigs_result_copy_pos(kmx_unitigs_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? unitigs_copy_out(R, host_dst, dst_entries, R->d_pos, R->n_rows, 4) : KMX_E_INVAL; }
extern "C" int kmx_unitigs_result_copy_ori(kmx_unitigs_result* R, uint8_t* host_dst, uint64_t dst_entries)
{ return R ? unitigs_copy_out(R, host_dst, dst_entries, R->d_ori, R->n_rows, 1) : KMX_E_INVAL; }
extern "C" int kmx_unitigs_result_copy_start(kmx_unitigs_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? unitigs_copy_out(R, host_dst, dst_entries, R->d_start, kmx_unitigs_result_n_unitigs(R), 4) : KMX_E_INVAL; }
extern "C" int kmx_unitigs_result_copy_len(kmx_unitigs_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? unitigs_copy_out(R, host_dst, dst_entries, R->d_len, kmx_unitigs_result_n_unitigs(R), 4) : KMX_E_INVAL; }
extern "C" int kmx_unitigs_result_copy_circ(kmx_unitigs_result* R, uint8_t* host_dst, uint64_t dst_entries)
{ return R ? unitigs_copy_out(R, host_dst, dst_entries, R->d_circ, kmx_unitigs_result_n_unitigs(R), 1) : KMX_E_INVAL; }
extern "C" int kmx_unitigs_result_copy_seq_off(kmx_unitigs_result* R, uint64_t* host_dst, uint64_t dst_entries)
{
  if (!R) return KMX_E_INVAL;
  const int rc = kmx_unitigs_result_wait(R);
  return rc != KMX_OK ? rc : mat_copy_out(R, host_dst, dst_entries, R->d_seq_off, (u64)R->h_tot[0] + 1, 8);
}
// the sequences: made by the first call that asks for them, n + U (k - 1) bytes -- U is known on the host behind the wait
extern "C" int kmx_unitigs_result_copy_seqs(kmx_unitigs_result* R, uint8_t* host_dst, uint64_t dst_bytes)
{
  if (!R) return KMX_E_INVAL;
  int rc = kmx_unitigs_result_wait(R);
  if (rc != KMX_OK) return rc;
  kmx_ctx* ctx = R->ctx;
  const u64 total = kmx_unitigs_result_seq_bytes(R);
  if (total && !R->d_seqs) {
    KMX_HIP(ctx, hipSetDevice(ctx->device));
    if (!(R->d_seqs = (u8*)R->keep(total))) return ctx->fail(KMX_E_NOMEM, "kmx_unitigs: device allocation failed (the sequences)");
    const u32 n = (u32)R->n_rows;
    UG_KW(R->kw, k_ug_emit, dim3(ug_grid(ctx, n)), dim3(UG_TILE), 0, ctx->stream, (const u64*)R->d_keys, n, R->k, R->h_tot[0], (const u32*)R->d_unitig,
          (const u32*)R->d_pos, (const u8*)R->d_ori, (const u64*)R->d_seq_off, total, R->d_seqs);
    KMX_HIP(ctx, hipGetLastError());
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return mat_copy_out(R, host_dst, dst_bytes, R->d_seqs, total, 1);
}
extern "C" double kmx_unitigs_result_kernel_ms(kmx_unitigs_result* R) { return R && R->ev[0] && kmx_unitigs_result_wait(R) == KMX_OK ? mat_kernel_ms(R) : -1.0; }
extern "C" int kmx_unitigs_result_kernel_parts_ms(kmx_unitigs_result* R, double* table_ms, double* links_ms, double* rank_ms, double* finish_ms)
{
  if (R && R->ev[0]) (void)kmx_unitigs_result_wait(R);      // (without profiling nothing is waited for)
  return mat_kernel_parts_ms(R, {table_ms, links_ms, rank_ms, finish_ms});
}
extern "C" uint64_t kmx_unitigs_result_algo_bytes(kmx_unitigs_result* R)
{
  if (kmx_unitigs_result_wait(R) != KMX_OK) return 0;
  const u64 n = R->n_rows, U = R->h_tot[0], kb = R->row_bytes;
  // the keys read by the table pass, written into the table and read back by 8 look-ups a node; the table cleared; candidates and links;
  // a state tuple read twice and written once a round; the per-node and per-unitig outputs
  return n * kb + 4 * ug_table_slots(n) + 8 * n * (kb + 4) + 2 * n * (4 + 4 + 4 + 16) + (u64)R->rounds * 2 * n * 48 + n * (2 * kb + 32) + n * 9 + U * 17 + 8;
}
extern "C" void kmx_unitigs_result_free(kmx_unitigs_result* R) { mat_free(R); }
