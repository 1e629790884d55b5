// zquery.hip -- `kmx query --z`: the findere trick over the Bloom matrices of a run (query.hip has the plain query).  The index holds
// k-mers; the query asks for (k + z)-mers: a position counts for a sample only when the rows of its z + 1 overlapping k-mers all have
// the sample's bit.  The neighbours of a window fall into different partitions (and partition groups), so the rows cannot be summed
// partition by partition as k_query_gather does: they are first laid out by POSITION.  gfx950, wave64.
//
//   k_query_keys      query.hip's, as it stands: per position (partition << 32 | row) or none; its per-query k-mer counts go to scratch
//   scan, k_query_parts   as in query.hip: every record's place in partition order
//   k_zquery_scatter  k_query_scatter's sibling: (row, position) records instead of (row, query)
//   k_zquery_rows     a group of L lanes takes ZR_RUN consecutive records, a lane one dword of the row (more when a row has more than
//                     64): the row is loaded at whatever alignment it has, masked to the columns below N and stored as aligned dwords
//                     at bits + position * pitch.  A position has one record and a partition is part of one call of a series: every
//                     cell of the table has one writer, plain stores.
//   k_zquery_window   (the last call of a series) items of QG_RUN consecutive positions; a lane's value at position j is the AND of its
//                     dword at j .. j + z (z + 1 loads of a block of (63 + z) * pitch bytes that the group has to itself: L1 / L2 hits),
//                     added into QG_PLANES bit-sliced planes and flushed to hits[query] with u32 atomic adds when the query changes
//                     and at the item's end.  j is a K-position when keys[j] and keys[j + z] are both set (z < k: the positions
//                     between them are valid and lie in the same query).  The lane that owns dword 0 counts them into n_kmers.
// Nothing holds a row or a query in LDS; no kernel uses scratch memory.
#include "kmx_host.hpp"
#include "kmer_dev.hpp"

namespace kmx {

constexpr u32 ZW_PLANES = 6;           // bit-sliced counter planes: column sums up to 63 ...
constexpr u32 ZW_RUN = 63;             // ... so an item of the window pass has 63 positions
constexpr u32 ZR_RUN = 64;             // records of an item of the row fetch
constexpr u64 ZK_NONE = ~0ULL;         // k_query_keys' mark of a position without a k-mer

__global__ __launch_bounds__(QK_BLOCK)
void k_zquery_scatter(const u64* __restrict__ keys, u64 n_bases, QChunks ch, u32* __restrict__ cell, u64* __restrict__ recs)
{
  const int lane = threadIdx.x & 63;
  const u32 c = (blockIdx.x * QK_BLOCK + threadIdx.x) >> 6;
  if (c >= ch.n_chunks) return;
  const u32 tile0 = c * ch.tiles_per_chunk, tile1 = min(tile0 + ch.tiles_per_chunk, ch.n_tiles);
  for (u32 t = tile0; t < tile1; t++) {
    const u64 t0 = (u64)t * 64, pos = t0 + lane;
    const u64 key = pos < n_bases ? keys[pos] : ZK_NONE;
    const bool valid = key != ZK_NONE;
    const u32 part = (u32)(key >> 32);
    u64 vm = __ballot(valid);
    while (vm) {      // the tile's partitions one by one: the lanes of one keep their order
      const int l = __builtin_ctzll(vm);
      const u32 pp = (u32)__shfl((int)part, l);
      const bool mine = valid && part == pp;
      const u64 same = __ballot(mine);
      u32 base = 0;
      if (lane == l) base = atomicAdd(&cell[(size_t)pp * ch.n_chunks + c], (u32)__popcll(same));      // (this wave is the cell's only writer)
      base = (u32)__shfl((int)base, l);
      if (mine) recs[base + (u32)__popcll(same & ((1ULL << lane) - 1ULL))] = (key & 0xFFFFFFFFULL) | (pos << 32);      // (pos < 2^32)
      vm &= ~same;
    }
    if (t0 + 63 >= n_bases) break;
  }
}

struct __attribute__((packed, aligned(1))) ZDword { u32 v; };      // a dword at any address: one global_load_dword

// LOG_L: log2 of the lanes of a group (a group's lane wl owns the row's dwords wl, wl + L, ...)
template <int LOG_L>
__global__ __launch_bounds__(256)
void k_zquery_rows(const u64* __restrict__ recs, const u32* __restrict__ pstart, u32 n_parts, const u8* const* __restrict__ rows,
                   u32 nb, u32 n_cols, u8* __restrict__ bits)
{
  constexpr u32 L = 1u << LOG_L, S = 64u / L;
  const u32 total = pstart[n_parts];
  const u32 lane = threadIdx.x & 63u, wl = lane & (L - 1u), sub = lane >> LOG_L;
  const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
  const u64 n_items = ((u64)total + ZR_RUN - 1) / ZR_RUN;
  const u32 nw = (nb + 3u) / 4u;                   // dwords of a row, the last one maybe short; the table's pitch is 4 * nw
  for (u64 g = wave * S + sub; g < n_items; g += n_waves * S) {
    const u32 i0 = (u32)(g * ZR_RUN), i1 = (u32)min((u64)total, (u64)i0 + ZR_RUN);
    u32 p = 0;
    { u32 lo = 0, hi = n_parts; while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (pstart[mid] <= i0) lo = mid; else hi = mid; } p = lo; }      // pstart[p] <= i0 (pstart[0] = 0)
    u32 pend = pstart[p + 1];
    const u8* base = rows[p];
    for (u32 i = i0; i < i1; i++) {
      while (i >= pend) { p++; pend = pstart[p + 1]; base = rows[p]; }      // (i < total = pstart[n_parts]: p stays below n_parts)
      if (!base) continue;                         // a partition that is not part of this call: another call of the series writes it
      const u64 rec = recs[i];
      const u8* row = base + (u64)(u32)rec * nb;   // 64-bit row offsets: window * nb passes 4 GiB
      u32* dst = reinterpret_cast<u32*>(bits + (rec >> 32) * (4ull * nw));
      for (u32 ws = wl; ws < nw; ws += L) {        // (one pass for rows of up to 64 dwords: 2048 columns)
        const u8* rp = row + 4u * ws;
        const u32 col0 = 32u * ws;
        const u32 cmask = n_cols - col0 >= 32u ? 0xFFFFFFFFu : (1u << (n_cols - col0)) - 1u;      // the padding bits never reach the table
        u32 x;
        if (4u * ws + 4u <= nb) x = reinterpret_cast<const ZDword*>(rp)->v;
        else { x = 0; for (u32 b = 0; 4u * ws + b < nb; b++) x |= (u32)rp[b] << (8u * b); }      // nothing behind a body is read
        dst[ws] = x & cmask;
      }
    }
  }
}

template <int LOG_L>
__global__ __launch_bounds__(256)
void k_zquery_window(const u64* __restrict__ keys, const u64* __restrict__ offsets, u32 n_seqs, u64 n_bases, u32 z,
                     const u8* __restrict__ bits, u32 nb, u32 n_cols, u32* __restrict__ n_kmers, u32* __restrict__ hits)
{
  constexpr u32 L = 1u << LOG_L, S = 64u / L;
  const u32 lane = threadIdx.x & 63u, wl = lane & (L - 1u), sub = lane >> LOG_L;
  const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
  const u64 n_items = (n_bases + ZW_RUN - 1) / ZW_RUN;
  const u32 nw = (nb + 3u) / 4u;
  const u32* __restrict__ tab = reinterpret_cast<const u32*>(bits);
  for (u64 g = wave * S + sub; g < n_items; g += n_waves * S) {
    const u64 j0 = g * ZW_RUN, j1 = min(n_bases, j0 + ZW_RUN);
    const u32 q0 = q_query_of(offsets, 0, n_seqs, j0);      // (j0 < n_bases = offsets[n_seqs], offsets[0] = 0)
    for (u32 ws = wl; ws < nw; ws += L) {
      const u32 col0 = 32u * ws;
      const u32 cmask = n_cols - col0 >= 32u ? 0xFFFFFFFFu : (1u << (n_cols - col0)) - 1u;      // (the table holds no bit from N on: a column index stays below N whatever a given table holds)
      u32 pl[ZW_PLANES];
#pragma unroll
      for (u32 j = 0; j < ZW_PLANES; j++) pl[j] = 0;
      u32 cnt = 0;
      auto flush = [&](u32 q) {
        if (ws == 0 && cnt) atomicAdd(&n_kmers[q], cnt);      // (ws == 0: the group's lane 0 in its first pass)
        cnt = 0;
        u32 any = 0;
#pragma unroll
        for (u32 j = 0; j < ZW_PLANES; j++) any |= pl[j];
        for (u32 left = any; left; left &= left - 1u) {
          const u32 b = (u32)__builtin_ctz(left);
          u32 c = 0;
#pragma unroll
          for (u32 j = 0; j < ZW_PLANES; j++) c |= ((pl[j] >> b) & 1u) << j;
          atomicAdd(&hits[(u64)q * n_cols + col0 + b], c);
        }
#pragma unroll
        for (u32 j = 0; j < ZW_PLANES; j++) pl[j] = 0;
      };
      u32 q = q0;
      u64 qend = offsets[q0 + 1];
      for (u64 j = j0; j < j1; j++) {
        if (j >= qend) {      // the next query that has a base (empty queries share an offset and are skipped; j < offsets[n_seqs])
          flush(q);
          do { q++; qend = offsets[q + 1]; } while (j >= qend);
        }
        if (j + z >= n_bases || keys[j] == ZK_NONE || keys[j + z] == ZK_NONE) continue;
        cnt++;
        const u32* cp = tab + j * nw + ws;
        u32 x = cp[0];
        for (u32 t = 1; t <= z; t++) x &= cp[(u64)t * nw];
        x &= cmask;
#pragma unroll
        for (u32 j2 = 0; j2 < ZW_PLANES; j2++) { const u32 carry = pl[j2] & x; pl[j2] ^= x; x = carry; }
      }
      flush(q);
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
hipError_t launch_zquery_scatter(const u64* keys, u64 n_bases, u32 n_tiles, u32 n_chunks, u32 tiles_per_chunk, u32* cell, u64* recs, hipStream_t st)
{
  const QChunks ch{n_tiles, n_chunks, tiles_per_chunk};
  const u32 grid = (n_chunks + QK_BLOCK / 64 - 1) / (QK_BLOCK / 64);
  hipLaunchKernelGGL(k_zquery_scatter, dim3(grid), dim3(QK_BLOCK), 0, st, keys, n_bases, ch, cell, recs);
  return hipGetLastError();
}

static int zquery_log_l(u32 nb)
{
  const u32 nw = (nb + 3) / 4;
  int log_l = 0;
  while (log_l < 6 && (1u << log_l) < nw) log_l++;
  return log_l;
}

static u32 zquery_grid(u64 items, int log_l, u32 n_cu)
{
  const u64 per_block = 4ull * (64u >> log_l);      // groups of lanes a workgroup holds
  return (u32)std::max<u64>(1, std::min<u64>((items + per_block - 1) / per_block, (u64)std::max(n_cu, 1u) * 8));
}

hipError_t launch_zquery_rows(const u64* recs, u64 rec_bound, const u32* pstart, u32 n_parts, const u8* const* rows, u32 nb, u32 n_cols,
                              u8* bits, u32 n_cu, hipStream_t st)
{
  const int log_l = zquery_log_l(nb);
  const u32 grid = zquery_grid((rec_bound + ZR_RUN - 1) / ZR_RUN, log_l, n_cu);
#define KMX_ZR(LL) hipLaunchKernelGGL((k_zquery_rows<LL>), dim3(grid), dim3(256), 0, st, recs, pstart, n_parts, rows, nb, n_cols, bits)
  switch (log_l) {
    case 0: KMX_ZR(0); break; case 1: KMX_ZR(1); break; case 2: KMX_ZR(2); break; case 3: KMX_ZR(3); break;
    case 4: KMX_ZR(4); break; case 5: KMX_ZR(5); break; default: KMX_ZR(6); break;
  }
#undef KMX_ZR
  return hipGetLastError();
}

hipError_t launch_zquery_window(const u64* keys, const u64* offsets, u32 n_seqs, u64 n_bases, u32 z, const u8* bits, u32 nb, u32 n_cols,
                                u32* n_kmers, u32* hits, u32 n_cu, hipStream_t st)
{
  const int log_l = zquery_log_l(nb);
  const u32 grid = zquery_grid((n_bases + ZW_RUN - 1) / ZW_RUN, log_l, n_cu);
#define KMX_ZW(LL) hipLaunchKernelGGL((k_zquery_window<LL>), dim3(grid), dim3(256), 0, st, keys, offsets, n_seqs, n_bases, z, bits, nb, n_cols, n_kmers, hits)
  switch (log_l) {
    case 0: KMX_ZW(0); break; case 1: KMX_ZW(1); break; case 2: KMX_ZW(2); break; case 3: KMX_ZW(3); break;
    case 4: KMX_ZW(4); break; case 5: KMX_ZW(5); break; default: KMX_ZW(6); break;
  }
#undef KMX_ZW
  return hipGetLastError();
}

}  // namespace kmx
