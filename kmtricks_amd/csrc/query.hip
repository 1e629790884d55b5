// query.hip -- `kmx query` on the device: which samples of a Bloom matrix (--mode hash:bf:bin, one .cmbf a partition) hold the k-mers
// of a set of query sequences.  No reference counterpart in the 1.6.0 tree (kmtricks 1.0's `kmtricks query` moved to kmindex); the
// addressing is the published one: repartition.hpp:94-103 get_partition, kmer_hash.hpp:244-328 WinHasher.  gfx950, wave64.
//
//   k_query_keys     the concatenated base stream is cut in tiles of 64 positions, a WAVE takes a run of tiles (a chunk), a lane one
//                    position: the bases of the tile and of the 192 behind it become ballot bit planes, a lane's k-mer is k bits of
//                    each plane at its own position -- canonical form by bit reversal, minimizer = window minimum of mmer_value
//                    (a sparse table over the 192 m-mer values, wave shuffles; q_tile_kmer in kmer_dev.hpp, shared with kquery.hip),
//                    row = XXH64(words) % window.  The query of a position
//                    is a search of `offsets`, bounded by a gallop from the query of the tile before.  Per valid position one u64
//                    (partition << 32 | row) at the position's own slot; one add per partition of the tile to its (partition, chunk)
//                    counter and one per query to n_kmers[query].
//   scan             launch_filter_scan over the counters laid out [partition][chunk]: every cell's place in partition order, position
//                    order kept inside a partition (a stable counting sort, one wave the only writer of its cells)
//   k_query_parts    first record of every partition
//   k_query_scatter  the same chunks again: (row, query) records to their place
//   k_query_gather   a group of L lanes (L = the row's dwords rounded up to a power of two, at most 64) takes QG_RUN consecutive records,
//                    a lane one dword of the row (more when a row has more than 64): rows are loaded at whatever alignment they have,
//                    summed per bit column in QG_PLANES bit-sliced planes (a ripple-carry add of one bit a row and plane), and the
//                    non-zero column sums go to hits[query][column] with u32 atomic adds whenever the query changes and at the end.
//                    Integer adds commute: the table does not depend on scheduling.
// Nothing holds a row or a query in LDS: no limit on columns or on a query's length below 2^32 positions.
#include "seqquery_host.hpp"
#include "kmer_dev.hpp"

namespace kmx {

constexpr u32 QG_PLANES = 6;           // bit-sliced counter planes: column sums up to 63
constexpr u32 QG_RUN = 63;             // records of a gather item: what the planes hold without a flush
constexpr u64 QK_NONE = ~0ULL;
constexpr u32 QG_NO_ROW = 0xFFFFFFFFu; // keyed gather: the record's k-mer is no row's key (a partition has at most 2^32 - 256 rows)

template <int KW>
__global__ __launch_bounds__(QK_BLOCK)
void k_query_keys(const char* __restrict__ bases, const u64* __restrict__ offsets, u32 n_seqs, u64 n_bases, int k, int m,
                  const u16* __restrict__ repart, u64 window, QChunks ch, u64* __restrict__ keys, u32* __restrict__ hist, u32* __restrict__ n_kmers)
{
  const int lane = threadIdx.x & 63;
  const u32 c = (blockIdx.x * QK_BLOCK + threadIdx.x) >> 6;
  if (c >= ch.n_chunks) return;
  const u32 tile0 = c * ch.tiles_per_chunk, tile1 = min(tile0 + ch.tiles_per_chunk, ch.n_tiles);
  if (tile0 >= tile1) return;
  const QWalk wk = q_walk(k, m);
  u32 qs = q_query_of(offsets, 0, n_seqs, (u64)tile0 * 64);      // (position tile0 * 64 < n_bases = offsets[n_seqs])
  for (u32 t = tile0; t < tile1; t++) {
    const u64 t0 = (u64)t * 64, pos = t0 + lane;
    u64 cw[KW]; u32 mini;
    const bool whole = q_tile_kmer<KW>(bases, n_bases, pos, lane, wk, cw, mini);
    const u64 h = xxh64_words(cw, KW) % window;
    // ---- which query, and is the k-mer whole and inside it ----
    const u32 q = q_tile_query(offsets, n_seqs, qs, t0, pos);
    bool valid = pos < n_bases && whole;
    if (valid) valid = pos >= offsets[q] && pos + (u64)k <= offsets[q + 1];      // (bases in front of offsets[0] belong to no query)
    const u32 part = valid ? (u32)repart[mini] : 0u;
    if (pos < n_bases) keys[pos] = valid ? ((u64)part << 32) | h : QK_NONE;
    q_tile_adds(valid, part, q, lane, hist, ch.n_chunks, c, n_kmers);
    qs = (u32)__shfl((int)q, 63);      // (lanes behind the last base searched with pos >= n_bases: the walk ends with this tile)
    if (t0 + 63 >= n_bases) break;
  }
}

__global__ void k_query_parts(const u32* __restrict__ cell, u32 n_parts, u32 n_chunks, u32* __restrict__ pstart)
{
  const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p <= n_parts) pstart[p] = cell[(size_t)p * n_chunks];      // (cell[n_parts * n_chunks]: the total)
}

__global__ __launch_bounds__(QK_BLOCK)
void k_query_scatter(const u64* __restrict__ keys, const u64* __restrict__ offsets, u32 n_seqs, u64 n_bases, QChunks ch,
                     u32* __restrict__ cell, u64* __restrict__ recs)
{
  const int lane = threadIdx.x & 63;
  const u32 c = (blockIdx.x * QK_BLOCK + threadIdx.x) >> 6;
  if (c >= ch.n_chunks) return;
  const u32 tile0 = c * ch.tiles_per_chunk, tile1 = min(tile0 + ch.tiles_per_chunk, ch.n_tiles);
  if (tile0 >= tile1) return;
  u32 qs = q_query_of(offsets, 0, n_seqs, (u64)tile0 * 64);
  for (u32 t = tile0; t < tile1; t++) {
    const u64 t0 = (u64)t * 64, pos = t0 + lane;
    const u64 key = pos < n_bases ? keys[pos] : QK_NONE;
    const bool valid = key != QK_NONE;
    const u32 q = q_tile_query(offsets, n_seqs, qs, t0, pos);
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
      if (mine) recs[base + (u32)__popcll(same & ((1ULL << lane) - 1ULL))] = (key & 0xFFFFFFFFULL) | ((u64)q << 32);
      vm &= ~same;
    }
    qs = (u32)__shfl((int)q, 63);
    if (t0 + 63 >= n_bases) break;
  }
}


// LOG_L: log2 of the lanes of a group (a group's lane wl owns the row's dwords wl, wl + L, ...)
// KEYED: the rows of a k-mer matrix (kquery.hip) -- a record's row lies at row * stride + skip (the nb presence/absence bytes behind the
// key) and a record whose row is QG_NO_ROW met no row; else the rows of a Bloom matrix: row * nb, every record has one
template <int LOG_L, bool KEYED>
__global__ __launch_bounds__(256)
void k_query_gather(const u64* __restrict__ recs, const u32* __restrict__ pstart, u32 n_parts, const u8* const* __restrict__ rows,
                    u32 nb, u32 n_cols, u32* __restrict__ hits, u64 stride, u32 skip)
{
  constexpr u32 L = 1u << LOG_L, S = 64u / L;
  const u32 total = pstart[n_parts];
  const u32 lane = threadIdx.x & 63u, wl = lane & (L - 1u), sub = lane >> LOG_L;
  const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
  const u64 n_items = ((u64)total + QG_RUN - 1) / QG_RUN;
  const u32 nw = (nb + 3u) / 4u;                   // dwords of a row, the last one maybe short
  for (u64 g = wave * S + sub; g < n_items; g += n_waves * S) {
    const u32 i0 = (u32)(g * QG_RUN), i1 = (u32)min((u64)total, (u64)i0 + QG_RUN);
    u32 p0 = 0;
    { u32 lo = 0, hi = n_parts; while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (pstart[mid] <= i0) lo = mid; else hi = mid; } p0 = lo; }      // pstart[p0] <= i0 (pstart[0] = 0)
    for (u32 ws = wl; ws < nw; ws += L) {          // (one pass for rows of up to 64 dwords: 2048 columns)
      const u32 whole = 4u * ws + 4u <= nb;
      const u32 col0 = 32u * ws;
      const u32 cmask = n_cols - col0 >= 32u ? 0xFFFFFFFFu : (1u << (n_cols - col0)) - 1u;      // the padding bits of the last byte are never read into a sum
      u32 pl[QG_PLANES];
#pragma unroll
      for (u32 j = 0; j < QG_PLANES; j++) pl[j] = 0;
      auto flush = [&](u32 q) {
        u32 any = 0;
#pragma unroll
        for (u32 j = 0; j < QG_PLANES; j++) any |= pl[j];
        for (u32 left = any; left; left &= left - 1u) {
          const u32 b = (u32)__builtin_ctz(left);
          u32 cnt = 0;
#pragma unroll
          for (u32 j = 0; j < QG_PLANES; j++) cnt |= ((pl[j] >> b) & 1u) << j;
          atomicAdd(&hits[(u64)q * n_cols + col0 + b], cnt);
        }
#pragma unroll
        for (u32 j = 0; j < QG_PLANES; j++) pl[j] = 0;
      };
      u32 p = p0, pend = pstart[p0 + 1];
      const u8* base = rows[p0];
      u32 cur_q = (u32)(recs[i0] >> 32);
      for (u32 i = i0; i < i1; i++) {
        const u64 rec = recs[i];
        const u32 q = (u32)(rec >> 32);
        while (i >= pend) { p++; pend = pstart[p + 1]; base = rows[p]; }      // (i < total = pstart[n_parts]: p stays below n_parts)
        if (q != cur_q) { flush(cur_q); cur_q = q; }
        if (!base) continue;                       // a partition that is not part of this call
        if (KEYED && (u32)rec == QG_NO_ROW) continue;
        const u8* rp = KEYED ? base + (u64)(u32)rec * stride + skip + 4u * ws
                             : base + (u64)(u32)rec * nb + 4u * ws;      // 64-bit row offsets: window * nb passes 4 GiB
        u32 x;
        if (whole) x = reinterpret_cast<const UDword*>(rp)->v;
        else { x = 0; for (u32 b = 0; 4u * ws + b < nb; b++) x |= (u32)rp[b] << (8u * b); }
        x &= cmask;
#pragma unroll
        for (u32 j = 0; j < QG_PLANES; j++) { const u32 carry = pl[j] & x; pl[j] ^= x; x = carry; }
      }
      flush(cur_q);
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
void query_chunks(u64 n_bases, u32 n_parts, u32* n_tiles, u32* n_chunks, u32* tiles_per_chunk)
{
  const u32 tiles = (u32)((n_bases + 63) / 64);
  u32 chunks = std::max(1u, std::min(tiles, 2048u));
  while (chunks > 1 && (u64)chunks * n_parts > 262144) chunks >>= 1;       // (the scan of the cells is one workgroup's: at most 262144 of them)
  const u32 tpc = std::max(1u, (tiles + chunks - 1) / chunks);
  *n_tiles = tiles; *tiles_per_chunk = tpc; *n_chunks = std::max(1u, (tiles + tpc - 1) / tpc);
}

hipError_t launch_query_keys(int kw, const char* bases, const u64* offsets, u32 n_seqs, u64 n_bases, int k, int m, const u16* repart, u64 window,
                             u32 n_tiles, u32 n_chunks, u32 tiles_per_chunk, u64* keys, u32* hist, u32* n_kmers, hipStream_t st)
{
  const QChunks ch{n_tiles, n_chunks, tiles_per_chunk};
  const u32 grid = (n_chunks + QK_BLOCK / 64 - 1) / (QK_BLOCK / 64);
  switch (kw) {
    case 1: hipLaunchKernelGGL(k_query_keys<1>, dim3(grid), dim3(QK_BLOCK), 0, st, bases, offsets, n_seqs, n_bases, k, m, repart, window, ch, keys, hist, n_kmers); break;
    case 2: hipLaunchKernelGGL(k_query_keys<2>, dim3(grid), dim3(QK_BLOCK), 0, st, bases, offsets, n_seqs, n_bases, k, m, repart, window, ch, keys, hist, n_kmers); break;
    case 3: hipLaunchKernelGGL(k_query_keys<3>, dim3(grid), dim3(QK_BLOCK), 0, st, bases, offsets, n_seqs, n_bases, k, m, repart, window, ch, keys, hist, n_kmers); break;
    case 4: hipLaunchKernelGGL(k_query_keys<4>, dim3(grid), dim3(QK_BLOCK), 0, st, bases, offsets, n_seqs, n_bases, k, m, repart, window, ch, keys, hist, n_kmers); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_query_parts(const u32* cell, u32 n_parts, u32 n_chunks, u32* pstart, hipStream_t st)
{
  hipLaunchKernelGGL(k_query_parts, dim3((n_parts + 256) / 256), dim3(256), 0, st, cell, n_parts, n_chunks, pstart);
  return hipGetLastError();
}

hipError_t launch_query_scatter(const u64* keys, const u64* offsets, u32 n_seqs, u64 n_bases, u32 n_tiles, u32 n_chunks, u32 tiles_per_chunk,
                                u32* cell, u64* recs, hipStream_t st)
{
  const QChunks ch{n_tiles, n_chunks, tiles_per_chunk};
  const u32 grid = (n_chunks + QK_BLOCK / 64 - 1) / (QK_BLOCK / 64);
  hipLaunchKernelGGL(k_query_scatter, dim3(grid), dim3(QK_BLOCK), 0, st, keys, offsets, n_seqs, n_bases, ch, cell, recs);
  return hipGetLastError();
}

template <bool KEYED>
static hipError_t query_gather(const u64* recs, u64 rec_bound, const u32* pstart, u32 n_parts, const u8* const* rows, u32 nb, u32 n_cols,
                               u32* hits, u64 stride, u32 skip, u32 n_cu, hipStream_t st)
{
  const u32 nw = (nb + 3) / 4;
  int log_l = 0;
  while (log_l < 6 && (1u << log_l) < nw) log_l++;
  const u64 groups = (rec_bound + QG_RUN - 1) / QG_RUN, per_block = 4ull * (64u >> log_l);      // groups of lanes a workgroup holds
  const u32 grid = (u32)std::max<u64>(1, std::min<u64>((groups + per_block - 1) / per_block, (u64)std::max(n_cu, 1u) * 8));
#define KMX_QG(LL) hipLaunchKernelGGL((k_query_gather<LL, KEYED>), dim3(grid), dim3(256), 0, st, recs, pstart, n_parts, rows, nb, n_cols, hits, stride, skip)
  switch (log_l) {
    case 0: KMX_QG(0); break; case 1: KMX_QG(1); break; case 2: KMX_QG(2); break; case 3: KMX_QG(3); break;
    case 4: KMX_QG(4); break; case 5: KMX_QG(5); break; default: KMX_QG(6); break;
  }
#undef KMX_QG
  return hipGetLastError();
}

hipError_t launch_query_gather(const u64* recs, u64 rec_bound, const u32* pstart, u32 n_parts, const u8* const* rows, u32 nb, u32 n_cols,
                               u32* hits, u32 n_cu, hipStream_t st)
{ return query_gather<false>(recs, rec_bound, pstart, n_parts, rows, nb, n_cols, hits, nb, 0, n_cu, st); }

// the same gather over the presence/absence rows of a k-mer matrix: records (row, query) as k_kquery_search leaves them (kquery.hip)
hipError_t launch_query_gather_keyed(const u64* recs, u64 rec_bound, const u32* pstart, u32 n_parts, const u8* const* rows, u64 stride, u32 skip,
                                     u32 nb, u32 n_cols, u32* hits, u32 n_cu, hipStream_t st)
{ return query_gather<true>(recs, rec_bound, pstart, n_parts, rows, nb, n_cols, hits, stride, skip, n_cu, st); }

}  // namespace kmx

using namespace kmx;

// ---- query -------------------------------------------------------------------------------------------------------------------------
// kmx_query_dev / kmx_query_host: query sequences against the Bloom matrices of a run.  The shared host path: seqquery_host.hpp.
struct kmx_query_result : SeqResult {
  u32 nb = 0;
  u32 *d_kmers = nullptr, *d_hits = nullptr;      // d_hits: the result's own table or the caller's
};

// the kernels of one call, queued on ctx->stream; every pointer of K a device pointer but K->rows (a host array of device pointers)
static int query_queue(kmx_ctx* ctx, const kmx_query_task* K, kmx_query_result* R)
{
  hipStream_t st = ctx->stream;
  const u64 n_bases = R->n_bases;
  const u32 n_seqs = (u32)R->n_seqs, P = K->nb_parts, N = K->n_cols, nb = R->nb, kw = (K->kmer_size + 31) / 32;
  u32 n_tiles = 0, n_chunks = 1, tpc = 1;
  query_chunks(n_bases, P, &n_tiles, &n_chunks, &tpc);
  const u64 cells = (u64)P * n_chunks + 1, table = (u64)n_seqs * N;
  u64* d_keys = (u64*)R->tmp(8 * n_bases);
  u64* d_recs = (u64*)R->tmp(8 * n_bases);
  u32* d_cell = (u32*)R->tmp(4 * cells);
  u32* d_pstart = (u32*)R->tmp(4ull * (P + 1));
  R->d_kmers = (u32*)R->keep(4ull * n_seqs);
  u32* hits_own = K->hits ? nullptr : (u32*)R->keep(4 * table);
  R->d_hits = K->hits ? K->hits : hits_own;
  const int rc = seq_queue_head(R, K->rows, nullptr, 64);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_cell, 0, 4 * cells, st));
  KMX_HIP(ctx, hipMemsetAsync(d_pstart, 0, 4ull * (P + 1), st));
  if (n_seqs) KMX_HIP(ctx, hipMemsetAsync(R->d_kmers, 0, 4ull * n_seqs, st));
  if (hits_own && table) KMX_HIP(ctx, hipMemsetAsync(hits_own, 0, 4 * table, st));
  if (n_bases) {
    KMX_HIP(ctx, launch_query_keys((int)kw, K->bases, (const u64*)K->offsets, n_seqs, n_bases, (int)K->kmer_size, (int)K->minim_size, K->repart, K->window,
                                   n_tiles, n_chunks, tpc, d_keys, d_cell, R->d_kmers, st));
    KMX_HIP(ctx, launch_filter_scan(d_cell, (u32)(cells - 1), st));
    KMX_HIP(ctx, launch_query_parts(d_cell, P, n_chunks, d_pstart, st));
    KMX_HIP(ctx, launch_query_scatter(d_keys, (const u64*)K->offsets, n_seqs, n_bases, n_tiles, n_chunks, tpc, d_cell, d_recs, st));
    KMX_HIP(ctx, launch_query_gather(d_recs, n_bases, d_pstart, P, R->d_rows, nb, N, R->d_hits, (u32)kmx_plan_cus(ctx), st));
  }
  return seq_queue_tail(R, d_pstart + P, 1);      // h_tot[0]: the valid k-mers of the call
}

static int query_call(kmx_ctx* ctx, const kmx_query_task* task, kmx_query_result** out, bool host, const char* who)
{
  u64 n_bases = 0;
  int rc = seq_args(ctx, task, out, who);
  if (rc == KMX_OK) rc = seq_check_bloom(ctx, task, who);
  if (rc == KMX_OK) rc = seq_n_bases(ctx, task->offsets, task->n_seqs, host, who, &n_bases);
  if (rc != KMX_OK) return rc;
  kmx_query_result* R = new kmx_query_result();
  R->init(ctx, "kmx_query", *task, n_bases); R->nb = (task->n_cols + 7) / 8;
  kmx_query_task dt = *task;
  std::vector<const uint8_t*> drows(task->nb_parts, nullptr);
  if (host) rc = seq_upload(R, &dt, drows, who, [&](u32) { return task->window * R->nb; });
  if (rc == KMX_OK) rc = query_queue(ctx, &dt, R);
  return seq_finish(R, rc, host, out);
}
extern "C" int kmx_query_dev(kmx_ctx* ctx, const kmx_query_task* task, kmx_query_result** out) { return query_call(ctx, task, out, false, "kmx_query_dev"); }
extern "C" int kmx_query_host(kmx_ctx* ctx, const kmx_query_task* task, kmx_query_result** out) { return query_call(ctx, task, out, true, "kmx_query_host"); }

extern "C" int kmx_query_result_wait(kmx_query_result* R) { return seq_wait(R); }
extern "C" uint64_t kmx_query_result_n_seqs(const kmx_query_result* R) { return R ? R->n_seqs : 0; }
extern "C" int kmx_query_result_copy_kmers(kmx_query_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? seq_copy_out(R, host_dst, dst_entries, R->d_kmers, R->n_seqs, 4) : KMX_E_INVAL; }
extern "C" int kmx_query_result_copy_hits(kmx_query_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? seq_copy_out(R, host_dst, dst_entries, R->d_hits, R->n_seqs * R->n_cols, 4) : KMX_E_INVAL; }
extern "C" uint32_t* kmx_query_result_hits_dev(kmx_query_result* R) { return R && seq_wait(R) == KMX_OK ? R->d_hits : nullptr; }
extern "C" double kmx_query_result_kernel_ms(kmx_query_result* R) { return seq_kernel_ms(R); }
extern "C" uint64_t kmx_query_result_algo_bytes(kmx_query_result* R)
{ return R && seq_wait(R) == KMX_OK ? R->n_bases + (u64)R->h_tot[0] * R->nb + 4 * R->n_seqs * R->n_cols : 0; }
extern "C" void kmx_query_result_free(kmx_query_result* R) { seq_free(R); }
