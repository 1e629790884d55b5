// kquery.hip -- `kmx query --kmer-index` on the device: which samples of a k-mer matrix (--mode kmer:count:bin / kmer:pa:bin, one
// .count / .pa a partition) hold the k-mers of a set of query sequences, and how often.  Exact: a k-mer is found or it is not.  No
// reference counterpart in the 1.6.0 tree; k-mer, minimizer and partition are those of query.hip (q_tile_kmer, kmer_dev.hpp).
// gfx950, wave64.
//
//   k_kquery_keys     query.hip's walk (tiles of 64 positions, a wave a chunk of tiles, a lane a position).  Per position: the partition
//                     (KQ_NO_PART: no k-mer here) and the canonical words, word w of all positions in one array -- a wave's store of a
//                     word is 512 contiguous bytes.  The same adds per (partition, chunk) and per query.
//   scan, k_query_parts   query.hip's: every (partition, chunk) cell's place in partition order
//   k_kquery_scatter  the same chunks again: (position, query) records to their place, position order kept inside a partition
//   k_kquery_search   a thread a record: lower bound of the position's k-mer over its partition's row keys at the row stride; the
//                     record becomes (row, query), row = KQ_NO_ROW when no row has the key or the partition is not part of the call
//   gather            PA: k_query_gather<., true> of query.hip (the bit-sliced planes, rows at the matrix's stride behind the key)
//                     COUNT: k_kquery_gather -- a group of L lanes takes KQ_RUN consecutive records, a lane the columns wl, wl + L, ...
//                     (KQ_COLS of them a pass): a u32 hit sum and a u64 count sum per column in registers across the records of one
//                     query, flushed with atomic adds when the query changes and at the run's end
// Nothing holds a row in LDS: no limit on columns.
#include "seqquery_host.hpp"
#include "kmer_dev.hpp"

namespace kmx {

constexpr u32 KQ_NO_PART = 0xFFFFu;       // partitions are 0 .. 65534
constexpr u32 KQ_NO_ROW = 0xFFFFFFFFu;    // a partition has at most 2^32 - 256 rows
constexpr u32 KQ_RUN = 128;               // records of a count gather item
constexpr u32 KQ_COLS = 4;                // columns a lane sums in one pass of a count gather

template <int KW>
__global__ __launch_bounds__(QK_BLOCK)
void k_kquery_keys(const char* __restrict__ bases, const u64* __restrict__ offsets, u32 n_seqs, u64 n_bases, int k, int m,
                   const u16* __restrict__ repart, QChunks ch, u16* __restrict__ parts, u64* __restrict__ words, u32* __restrict__ hist,
                   u32* __restrict__ n_kmers)
{
  const int lane = threadIdx.x & 63;
  const u32 c = (blockIdx.x * QK_BLOCK + threadIdx.x) >> 6;
  if (c >= ch.n_chunks) return;
  const u32 tile0 = c * ch.tiles_per_chunk, tile1 = min(tile0 + ch.tiles_per_chunk, ch.n_tiles);
  if (tile0 >= tile1) return;
  const QWalk wk = q_walk(k, m);
  u32 qs = q_query_of(offsets, 0, n_seqs, (u64)tile0 * 64);
  for (u32 t = tile0; t < tile1; t++) {
    const u64 t0 = (u64)t * 64, pos = t0 + lane;
    u64 cw[KW]; u32 mini;
    const bool whole = q_tile_kmer<KW>(bases, n_bases, pos, lane, wk, cw, mini);
    const u32 q = q_tile_query(offsets, n_seqs, qs, t0, pos);
    bool valid = pos < n_bases && whole;
    if (valid) valid = pos >= offsets[q] && pos + (u64)k <= offsets[q + 1];
    const u32 part = valid ? (u32)repart[mini] : 0u;
    if (pos < n_bases) {
      parts[pos] = (u16)(valid ? part : KQ_NO_PART);
#pragma unroll
      for (int w = 0; w < KW; w++) words[(u64)w * n_bases + pos] = cw[w];
    }
    q_tile_adds(valid, part, q, lane, hist, ch.n_chunks, c, n_kmers);
    qs = (u32)__shfl((int)q, 63);
    if (t0 + 63 >= n_bases) break;
  }
}

__global__ __launch_bounds__(QK_BLOCK)
void k_kquery_scatter(const u16* __restrict__ parts, const u64* __restrict__ offsets, u32 n_seqs, u64 n_bases, QChunks ch,
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
    const u32 part = pos < n_bases ? (u32)parts[pos] : KQ_NO_PART;
    const bool valid = part != KQ_NO_PART;
    const u32 q = q_tile_query(offsets, n_seqs, qs, t0, pos);
    u64 vm = __ballot(valid);
    while (vm) {      // the tile's partitions one by one: the lanes of one keep their order
      const int l = __builtin_ctzll(vm);
      const u32 pp = (u32)__shfl((int)part, l);
      const bool mine = valid && part == pp;
      const u64 same = __ballot(mine);
      u32 base = 0;
      if (lane == l) base = atomicAdd(&cell[(size_t)pp * ch.n_chunks + c], (u32)__popcll(same));      // (this wave is the cell's only writer)
      base = (u32)__shfl((int)base, l);
      if (mine) recs[base + (u32)__popcll(same & ((1ULL << lane) - 1ULL))] = (u64)(u32)pos | ((u64)q << 32);      // (fewer than 2^32 bases a call)
      vm &= ~same;
    }
    qs = (u32)__shfl((int)q, 63);
    if (t0 + 63 >= n_bases) break;
  }
}

// the partition of record i: the greatest p below n_parts with pstart[p] <= i (pstart[0] = 0; the empty partitions in front of it share its start)
__device__ __forceinline__ u32 kq_part_of(const u32* __restrict__ pstart, u32 n_parts, u32 i)
{
  u32 lo = 0, hi = n_parts;
  while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (pstart[mid] <= i) lo = mid; else hi = mid; }
  return lo;
}

template <int KW>
__global__ __launch_bounds__(256)
void k_kquery_search(u64* __restrict__ recs, const u32* __restrict__ pstart, u32 n_parts, const u8* const* __restrict__ rows,
                     const u32* __restrict__ n_rows, u64 stride, const u64* __restrict__ words, u64 n_bases, u32* __restrict__ n_found)
{
  const u32 total = pstart[n_parts];
  const u64 n_threads = (u64)gridDim.x * blockDim.x;
  u32 met = 0;      // this thread's records that met a row (the rows the gather reads: the call's algorithmic bytes)
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += n_threads) {
    const u64 rec = recs[i];
    const u32 pos = (u32)rec, p = kq_part_of(pstart, n_parts, (u32)i);
    const u8* base = rows[p];
    u32 found = KQ_NO_ROW;
    if (base) {
      Key<KW> key;
#pragma unroll
      for (int w = 0; w < KW; w++) key.w[w] = words[(u64)w * n_bases + pos];
      const u32 n = n_rows[p];
      u32 lo = 0, hi = n;      // the first row whose key is not below `key`
      while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (key_less<KW>(load_row_key<KW>(base + (u64)mid * stride), key)) lo = mid + 1; else hi = mid;
      }
      if (lo < n && key_eq<KW>(load_row_key<KW>(base + (u64)lo * stride), key)) found = lo;
    }
    recs[i] = (rec & 0xFFFFFFFF00000000ULL) | found;
    met += found != KQ_NO_ROW;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) met += (u32)__shfl_xor((int)met, off);      // (every lane of the wave is here)
  if ((threadIdx.x & 63u) == 0 && met) atomicAdd(n_found, met);
}


// LOG_L: log2 of the lanes of a group; SUMS: the u64 count sums are asked for
template <int LOG_L, bool SUMS>
__global__ __launch_bounds__(256)
void k_kquery_gather(const u64* __restrict__ recs, const u32* __restrict__ pstart, u32 n_parts, const u8* const* __restrict__ rows,
                     u64 stride, u32 skip, u32 n_cols, u32* __restrict__ hits, u64* __restrict__ sums)
{
  constexpr u32 L = 1u << LOG_L, S = 64u / L;
  const u32 total = pstart[n_parts];
  const u32 lane = threadIdx.x & 63u, wl = lane & (L - 1u), sub = lane >> LOG_L;
  const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
  const u64 n_items = ((u64)total + KQ_RUN - 1) / KQ_RUN;
  for (u64 g = wave * S + sub; g < n_items; g += n_waves * S) {
    const u32 i0 = (u32)(g * KQ_RUN), i1 = (u32)min((u64)total, (u64)i0 + KQ_RUN);
    const u32 p0 = kq_part_of(pstart, n_parts, i0);
    for (u32 c0 = wl; c0 < n_cols; c0 += KQ_COLS * L) {      // a pass: the lane's columns c0, c0 + L, ... (KQ_COLS of them)
      u32 h[KQ_COLS]; u64 s[KQ_COLS];
#pragma unroll
      for (u32 j = 0; j < KQ_COLS; j++) { h[j] = 0; s[j] = 0; }
      auto flush = [&](u32 q) {
#pragma unroll
        for (u32 j = 0; j < KQ_COLS; j++) {
          if (h[j]) {      // (a column without a hit has no count either)
            const u64 at = (u64)q * n_cols + c0 + j * L;
            atomicAdd(&hits[at], h[j]);
            if (SUMS) atomicAdd(&sums[at], s[j]);
          }
          h[j] = 0; s[j] = 0;
        }
      };
      u32 p = p0, pend = pstart[p0 + 1];
      const u8* base = rows[p0];
      u32 cur_q = (u32)(recs[i0] >> 32);
      for (u32 i = i0; i < i1; i++) {
        const u64 rec = recs[i];
        const u32 q = (u32)(rec >> 32);
        while (i >= pend) { p++; pend = pstart[p + 1]; base = rows[p]; }      // (i < total = pstart[n_parts]: p stays below n_parts)
        if (q != cur_q) { flush(cur_q); cur_q = q; }
        if (!base || (u32)rec == KQ_NO_ROW) continue;
        const u8* rp = base + (u64)(u32)rec * stride + skip;      // 64-bit row offsets
#pragma unroll
        for (u32 j = 0; j < KQ_COLS; j++) {
          const u32 col = c0 + j * L;
          if (col < n_cols) {
            const u32 x = reinterpret_cast<const UDword*>(rp + 4ull * col)->v;
            h[j] += x != 0;
            s[j] += x;
          }
        }
      }
      flush(cur_q);
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
hipError_t launch_kquery_keys(int kw, const char* bases, const u64* offsets, u32 n_seqs, u64 n_bases, int k, int m, const u16* repart,
                              u32 n_tiles, u32 n_chunks, u32 tiles_per_chunk, u16* parts, u64* words, u32* hist, u32* n_kmers, hipStream_t st)
{
  const QChunks ch{n_tiles, n_chunks, tiles_per_chunk};
  const u32 grid = (n_chunks + QK_BLOCK / 64 - 1) / (QK_BLOCK / 64);
#define KMX_KQK(W) hipLaunchKernelGGL(k_kquery_keys<W>, dim3(grid), dim3(QK_BLOCK), 0, st, bases, offsets, n_seqs, n_bases, k, m, repart, ch, parts, words, hist, n_kmers)
  switch (kw) {
    case 1: KMX_KQK(1); break; case 2: KMX_KQK(2); break; case 3: KMX_KQK(3); break; case 4: KMX_KQK(4); break;
    default: return hipErrorInvalidValue;
  }
#undef KMX_KQK
  return hipGetLastError();
}

hipError_t launch_kquery_scatter(const u16* parts, const u64* offsets, u32 n_seqs, u64 n_bases, u32 n_tiles, u32 n_chunks, u32 tiles_per_chunk,
                                 u32* cell, u64* recs, hipStream_t st)
{
  const QChunks ch{n_tiles, n_chunks, tiles_per_chunk};
  const u32 grid = (n_chunks + QK_BLOCK / 64 - 1) / (QK_BLOCK / 64);
  hipLaunchKernelGGL(k_kquery_scatter, dim3(grid), dim3(QK_BLOCK), 0, st, parts, offsets, n_seqs, n_bases, ch, cell, recs);
  return hipGetLastError();
}

hipError_t launch_kquery_search(int kw, u64* recs, u64 rec_bound, const u32* pstart, u32 n_parts, const u8* const* rows, const u32* n_rows,
                                u64 stride, const u64* words, u64 n_bases, u32* n_found, u32 n_cu, hipStream_t st)
{
  const u32 grid = (u32)std::max<u64>(1, std::min<u64>((rec_bound + 255) / 256, (u64)std::max(n_cu, 1u) * 32));
#define KMX_KQS(W) hipLaunchKernelGGL(k_kquery_search<W>, dim3(grid), dim3(256), 0, st, recs, pstart, n_parts, rows, n_rows, stride, words, n_bases, n_found)
  switch (kw) {
    case 1: KMX_KQS(1); break; case 2: KMX_KQS(2); break; case 3: KMX_KQS(3); break; case 4: KMX_KQS(4); break;
    default: return hipErrorInvalidValue;
  }
#undef KMX_KQS
  return hipGetLastError();
}

template <bool SUMS>
static hipError_t kquery_gather(const u64* recs, u64 rec_bound, const u32* pstart, u32 n_parts, const u8* const* rows, u64 stride, u32 skip,
                                u32 n_cols, u32* hits, u64* sums, u32 n_cu, hipStream_t st)
{
  int log_l = 0;
  while (log_l < 6 && (1u << log_l) < n_cols) log_l++;
  const u64 groups = (rec_bound + KQ_RUN - 1) / KQ_RUN, per_block = 4ull * (64u >> log_l);      // groups of lanes a workgroup holds
  const u32 grid = (u32)std::max<u64>(1, std::min<u64>((groups + per_block - 1) / per_block, (u64)std::max(n_cu, 1u) * 8));
#define KMX_KQG(LL) hipLaunchKernelGGL((k_kquery_gather<LL, SUMS>), dim3(grid), dim3(256), 0, st, recs, pstart, n_parts, rows, stride, skip, n_cols, hits, sums)
  switch (log_l) {
    case 0: KMX_KQG(0); break; case 1: KMX_KQG(1); break; case 2: KMX_KQG(2); break; case 3: KMX_KQG(3); break;
    case 4: KMX_KQG(4); break; case 5: KMX_KQG(5); break; default: KMX_KQG(6); break;
  }
#undef KMX_KQG
  return hipGetLastError();
}

hipError_t launch_kquery_gather(const u64* recs, u64 rec_bound, const u32* pstart, u32 n_parts, const u8* const* rows, u64 stride, u32 skip,
                                u32 n_cols, u32* hits, u64* sums, u32 n_cu, hipStream_t st)
{
  return sums ? kquery_gather<true>(recs, rec_bound, pstart, n_parts, rows, stride, skip, n_cols, hits, sums, n_cu, st)
              : kquery_gather<false>(recs, rec_bound, pstart, n_parts, rows, stride, skip, n_cols, hits, sums, n_cu, st);
}

}  // namespace kmx

using namespace kmx;

// ---- kquery ------------------------------------------------------------------------------------------------------------------------
// kmx_kquery_dev / kmx_kquery_host: query sequences against the k-mer matrices of a run.  The shared host path: seqquery_host.hpp;
// h_tot[0] the valid k-mers of the call, [1] those that met a row.
struct kmx_kquery_result : SeqResult {
  u64 stride = 0;
  u32 kw = 0;
  u32 *d_kmers = nullptr, *d_hits = nullptr;
  u64* d_sums = nullptr;                // null: the call was made without want_sums
};

static int kquery_check(kmx_ctx* ctx, const kmx_kquery_task* K, const char* who, u64* stride)
{
  const SeqCheck c{ctx, who};
  int rc;
  if ((rc = c.kmer_size(K->kmer_size)) || (rc = c.minim_size(K->minim_size, K->kmer_size))) return rc;
  if (K->key_words != (K->kmer_size + 31) / 32) return c.no(KMX_E_INVAL, ": key_words must be ceil(kmer_size / 32)");
  if ((rc = c.nb_parts(K->nb_parts))) return rc;
  if (K->mode == KMX_MODE_BF || K->mode == KMX_MODE_BFC || K->mode == KMX_MODE_BFT)
    return c.no(KMX_E_UNSUPPORTED, ": Bloom filter matrices are kmx_query's (KMX_MODE_COUNT and KMX_MODE_PA rows of k-mer matrices only; hash matrices neither)");
  if (K->mode != KMX_MODE_COUNT && K->mode != KMX_MODE_PA) return c.no(KMX_E_INVAL, ": mode must be KMX_MODE_COUNT or KMX_MODE_PA");
  if ((rc = c.n_cols(K->n_cols))) return rc;
  if (K->want_sums && K->mode != KMX_MODE_COUNT) return c.no(KMX_E_INVAL, ": presence/absence rows have no counts to sum (want_sums needs KMX_MODE_COUNT)");
  if (K->sums && !K->want_sums) return c.no(KMX_E_INVAL, ": a sums table without want_sums");
  if (!K->repart || !K->rows || !K->n_rows) return c.no(KMX_E_INVAL, ": null repartition table, row pointer array or row count array");
  if ((rc = c.reads(K->offsets, K->n_seqs, K->bases))) return rc;
  *stride = 8ull * K->key_words + (K->mode == KMX_MODE_COUNT ? 4ull * K->n_cols : ((u64)K->n_cols + 7) / 8);
  if ((rc = c.row_fits(*stride))) return rc;
  for (u32 p = 0; p < K->nb_parts; p++)
    if (K->rows[p] && K->n_rows[p] > 0xFFFFFF00ull) return c.no(KMX_E_UNSUPPORTED, ": more than 2^32 - 256 rows in a partition");
  return c.n_seqs(K->n_seqs);
}

// the kernels of one call, queued on ctx->stream; every pointer of K a device pointer but K->rows and K->n_rows (host arrays)
static int kquery_queue(kmx_ctx* ctx, const kmx_kquery_task* K, kmx_kquery_result* R)
{
  hipStream_t st = ctx->stream;
  const u64 n_bases = R->n_bases, stride = R->stride;
  const u32 n_seqs = (u32)R->n_seqs, P = K->nb_parts, N = K->n_cols, kw = K->key_words, skip = 8 * kw;
  u32 n_tiles = 0, n_chunks = 1, tpc = 1;
  query_chunks(n_bases, P, &n_tiles, &n_chunks, &tpc);
  const u64 cells = (u64)P * n_chunks + 1, table = (u64)n_seqs * N;
  u16* d_parts = (u16*)R->tmp(2 * n_bases);
  u64* d_words = (u64*)R->tmp(8 * n_bases * kw);
  u64* d_recs = (u64*)R->tmp(8 * n_bases);
  u32* d_cell = (u32*)R->tmp(4 * cells);
  u32* d_pstart = (u32*)R->tmp(4ull * (P + 1));
  R->d_kmers = (u32*)R->keep(4ull * n_seqs);
  u32* d_found = (u32*)R->tmp(4);
  u32* hits_own = K->hits ? nullptr : (u32*)R->keep(4 * table);
  R->d_hits = K->hits ? K->hits : hits_own;
  u64* sums_own = K->want_sums && !K->sums ? (u64*)R->keep(8 * table) : nullptr;
  R->d_sums = !K->want_sums ? nullptr : K->sums ? (u64*)K->sums : sums_own;
  const int rc = seq_queue_head(R, K->rows, K->n_rows, 64);      // the row counts travel as u32 behind the row pointers
  if (rc != KMX_OK) return rc;
  const u32* d_nrows = (const u32*)(R->d_rows + P);
  KMX_HIP(ctx, hipMemsetAsync(d_cell, 0, 4 * cells, st));
  KMX_HIP(ctx, hipMemsetAsync(d_pstart, 0, 4ull * (P + 1), st));
  KMX_HIP(ctx, hipMemsetAsync(d_found, 0, 4, st));
  if (n_seqs) KMX_HIP(ctx, hipMemsetAsync(R->d_kmers, 0, 4ull * n_seqs, st));
  if (hits_own && table) KMX_HIP(ctx, hipMemsetAsync(hits_own, 0, 4 * table, st));
  if (sums_own && table) KMX_HIP(ctx, hipMemsetAsync(sums_own, 0, 8 * table, st));
  if (n_bases) {
    KMX_HIP(ctx, launch_kquery_keys((int)kw, K->bases, (const u64*)K->offsets, n_seqs, n_bases, (int)K->kmer_size, (int)K->minim_size, K->repart,
                                    n_tiles, n_chunks, tpc, d_parts, d_words, d_cell, R->d_kmers, st));
    KMX_HIP(ctx, launch_filter_scan(d_cell, (u32)(cells - 1), st));
    KMX_HIP(ctx, launch_query_parts(d_cell, P, n_chunks, d_pstart, st));
    KMX_HIP(ctx, launch_kquery_scatter(d_parts, (const u64*)K->offsets, n_seqs, n_bases, n_tiles, n_chunks, tpc, d_cell, d_recs, st));
    KMX_HIP(ctx, launch_kquery_search((int)kw, d_recs, n_bases, d_pstart, P, R->d_rows, d_nrows, stride, d_words, n_bases, d_found, (u32)kmx_plan_cus(ctx), st));
    if (K->mode == KMX_MODE_PA)
      KMX_HIP(ctx, launch_query_gather_keyed(d_recs, n_bases, d_pstart, P, R->d_rows, stride, skip, (N + 7) / 8, N, R->d_hits, (u32)kmx_plan_cus(ctx), st));
    else
      KMX_HIP(ctx, launch_kquery_gather(d_recs, n_bases, d_pstart, P, R->d_rows, stride, skip, N, R->d_hits, R->d_sums, (u32)kmx_plan_cus(ctx), st));
  }
  return seq_queue_tail(R, d_pstart + P, 1, d_found);
}

static int kquery_call(kmx_ctx* ctx, const kmx_kquery_task* task, kmx_kquery_result** out, bool host, const char* who)
{
  u64 n_bases = 0, stride = 0;
  int rc = seq_args(ctx, task, out, who);
  if (rc == KMX_OK) rc = kquery_check(ctx, task, who, &stride);
  if (rc == KMX_OK) rc = seq_n_bases(ctx, task->offsets, task->n_seqs, host, who, &n_bases);
  if (rc != KMX_OK) return rc;
  kmx_kquery_result* R = new kmx_kquery_result();
  R->init(ctx, "kmx_kquery", *task, n_bases); R->stride = stride; R->kw = task->key_words;
  kmx_kquery_task dt = *task;
  std::vector<const uint8_t*> drows(task->nb_parts, nullptr);
  if (host) rc = seq_upload(R, &dt, drows, who, [&](u32 p) { return task->n_rows[p] * stride; });
  if (rc == KMX_OK) rc = kquery_queue(ctx, &dt, R);
  return seq_finish(R, rc, host, out);
}
extern "C" int kmx_kquery_dev(kmx_ctx* ctx, const kmx_kquery_task* task, kmx_kquery_result** out) { return kquery_call(ctx, task, out, false, "kmx_kquery_dev"); }
extern "C" int kmx_kquery_host(kmx_ctx* ctx, const kmx_kquery_task* task, kmx_kquery_result** out) { return kquery_call(ctx, task, out, true, "kmx_kquery_host"); }

extern "C" int kmx_kquery_result_wait(kmx_kquery_result* R) { return seq_wait(R); }
extern "C" uint64_t kmx_kquery_result_n_seqs(const kmx_kquery_result* R) { return R ? R->n_seqs : 0; }
extern "C" int kmx_kquery_result_copy_kmers(kmx_kquery_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? seq_copy_out(R, host_dst, dst_entries, R->d_kmers, R->n_seqs, 4) : KMX_E_INVAL; }
extern "C" int kmx_kquery_result_copy_hits(kmx_kquery_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? seq_copy_out(R, host_dst, dst_entries, R->d_hits, R->n_seqs * R->n_cols, 4) : KMX_E_INVAL; }
extern "C" int kmx_kquery_result_copy_sums(kmx_kquery_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? seq_copy_out(R, host_dst, dst_entries, R->d_sums, R->n_seqs * R->n_cols, 8, "kmx_kquery_result_copy_sums: the call was made without want_sums") : KMX_E_INVAL; }
extern "C" uint32_t* kmx_kquery_result_hits_dev(kmx_kquery_result* R) { return R && seq_wait(R) == KMX_OK ? R->d_hits : nullptr; }
extern "C" uint64_t* kmx_kquery_result_sums_dev(kmx_kquery_result* R) { return R && seq_wait(R) == KMX_OK ? (uint64_t*)R->d_sums : nullptr; }
extern "C" double kmx_kquery_result_kernel_ms(kmx_kquery_result* R) { return seq_kernel_ms(R); }
extern "C" uint64_t kmx_kquery_result_algo_bytes(kmx_kquery_result* R)
{
  if (!R || seq_wait(R) != KMX_OK) return 0;
  const u64 table = R->n_seqs * R->n_cols;
  return R->n_bases + (u64)R->h_tot[1] * R->stride + (u64)R->h_tot[0] * 8 * R->kw + 4 * table + (R->d_sums ? 8 * table : 0);
}
extern "C" void kmx_kquery_result_free(kmx_kquery_result* R) { seq_free(R); }
