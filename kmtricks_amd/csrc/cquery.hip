// cquery.hip -- `kmx query` over a counting Bloom index on the device: which samples of the .cmbf matrices of a `--mode hash:bfc:bin` run
// hold the k-mers of a set of query sequences, and at what abundance class (include/kmx.h, section "cquery").  No reference counterpart
// in the 1.6.0 tree; the rows are the ones k_merge_bf<BFC> writes (merge_bf.hip: N fields of w bits, bitpacker's MSB-first order).
// gfx950, wave64.
//
//   keys, scan, parts, scatter   query.hip's, unchanged: (row, query) records in partition order, position order kept inside a partition
//   k_cquery_gather   a group of L lanes takes CQ_RUN consecutive records, a lane BLOCKS of 8 consecutive columns (block wl, wl + L, ...:
//                     a pass each): the 8 fields of w bits of a block are exactly the w bytes at byte (c0 / 8) * w of the row, so every
//                     lane's piece starts on a byte for every w, no field lies in two lanes and neighbouring lanes read neighbouring
//                     bytes.  The w bytes become one big-endian u64, the 8 classes are shifted out of it; 8 u32 hit counters (class >=
//                     min_class) and 8 u64 sums of floor_of(class) stay in registers across the records of one query and are flushed
//                     with atomic adds when the query changes and at the run's end -- a column's hits and its sum each on their own
//                     test: with min_class > 1 a column has a sum and no hit.  Integer adds commute: the tables do not depend on
//                     scheduling.
// Nothing holds a row in LDS: no limit on columns.
// Every load of a body byte is inside [rows[p], rows[p] + window * nb) by construction: an address is rows[p] + row * nb + b with row <
// window (k_query_keys' modulus) and b < nb tested by the lane that loads -- a block's w bytes in pieces of 4, 2 and 1 when b0 + w <= nb,
// byte by byte up to nb in the row's last, short block; nothing is loaded in wider pieces than was tested and no address is rounded down.
// The bytes behind nb are never loaded, the fields of columns >= N are never added.
//
// The C ABI of the section lies here too (kmx_cquery_*), as dist.hip and diff.hip hold theirs.
#include "seqquery_host.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 CQ_RUN = 128;               // records of a gather item: 128 x 2^31 fits a u64 sum, 128 a u32 hit counter


// the w bytes (1 ... 8) at rp as one big-endian number, in pieces of 4, 2 and 1 bytes (w is the same in every lane: no divergence)
__device__ __forceinline__ u64 cq_load_be(const u8* rp, u32 w)
{
  u64 x = 0;
  if (w == 8) { x = __builtin_bswap32(reinterpret_cast<const UDword*>(rp)->v); rp += 4; w = 4; }
  if (w & 4u) { x = (x << 32) | __builtin_bswap32(reinterpret_cast<const UDword*>(rp)->v); rp += 4; }
  if (w & 2u) { x = (x << 16) | __builtin_bswap16(reinterpret_cast<const UShort*>(rp)->v); rp += 2; }
  if (w & 1u) x = (x << 8) | rp[0];
  return x;
}

// LOG_L: log2 of the lanes of a group (a group's lane wl owns the row's blocks of 8 columns wl, wl + L, ...)
template <int LOG_L>
__global__ __launch_bounds__(256)
void k_cquery_gather(const u64* __restrict__ recs, const u32* __restrict__ pstart, u32 n_parts, const u8* const* __restrict__ rows,
                     u32 nb, u32 w, u32 n_cols, u32 min_class, u32* __restrict__ hits, unsigned long long* __restrict__ sums)
{
  constexpr u32 L = 1u << LOG_L, S = 64u / L;
  const u32 total = pstart[n_parts];
  const u32 lane = threadIdx.x & 63u, wl = lane & (L - 1u), sub = lane >> LOG_L;
  const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((u64)gridDim.x * blockDim.x) >> 6;
  const u64 n_items = ((u64)total + CQ_RUN - 1) / CQ_RUN;
  const u32 n_blocks = (n_cols + 7u) / 8u;         // blocks of 8 columns, the last one maybe short
  const u32 cmask = (1u << w) - 1u;                // (w <= 8)
  for (u64 g = wave * S + sub; g < n_items; g += n_waves * S) {
    const u32 i0 = (u32)(g * CQ_RUN), i1 = (u32)min((u64)total, (u64)i0 + CQ_RUN);
    u32 p0 = 0;
    { u32 lo = 0, hi = n_parts; while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (pstart[mid] <= i0) lo = mid; else hi = mid; } p0 = lo; }      // pstart[p0] <= i0 (pstart[0] = 0)
    for (u32 bk = wl; bk < n_blocks; bk += L) {    // a pass: the lane's block of columns 8 bk ... 8 bk + 7 (one pass for rows of up to 512 columns)
      const u32 b0 = bk * w;                                       // (8 bk < n_cols, so b0 < nb)
      const bool whole = b0 + w <= nb;                             // the block's w bytes lie inside the row
      const u32 c0 = 8u * bk, nc = min(8u, n_cols - c0);           // its columns: fields behind nc are padding (or the next row)
      u32 h[8]; u64 s[8];
#pragma unroll
      for (u32 j = 0; j < 8; j++) { h[j] = 0; s[j] = 0; }
      auto flush = [&](u32 q) {
        const u64 at = (u64)q * n_cols + c0;
#pragma unroll
        for (u32 j = 0; j < 8; j++) {      // (h[j] = s[j] = 0 for j >= nc: no cell behind the row is touched)
          if (h[j]) atomicAdd(&hits[at + j], h[j]);
          if (s[j]) atomicAdd(&sums[at + j], (unsigned long long)s[j]);
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
        if (!base) continue;                       // a partition that is not part of this call
        const u8* rp = base + (u64)(u32)rec * nb + b0;      // 64-bit row offsets: window * nb passes 4 GiB
        u64 x;
        if (whole) x = cq_load_be(rp, w);
        else { x = 0; for (u32 b = 0; b < w; b++) { x <<= 8; if (b0 + b < nb) x |= rp[b]; } }      // the row's last block: zeros behind nb
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
          const u32 v = j < nc ? (u32)(x >> (w * (7u - j))) & cmask : 0u;
          h[j] += v >= min_class;                  // (min_class >= 1: class 0 is no hit)
          s[j] += v ? 1ull << (min(v, 32u) - 1u) : 0ull;      // floor_of
        }
      }
      flush(cur_q);
    }
  }
}

hipError_t launch_cquery_gather(const u64* recs, u64 rec_bound, const u32* pstart, u32 n_parts, const u8* const* rows, u32 nb, u32 bitw,
                                u32 n_cols, u32 min_class, u32* hits, u64* sums, u32 n_cu, hipStream_t st)
{
  if (bitw < 1 || bitw > 8) return hipErrorInvalidValue;
  const u32 n_blocks = (n_cols + 7) / 8;
  int log_l = 0;
  while (log_l < 6 && (1u << log_l) < n_blocks) log_l++;
  const u64 groups = (rec_bound + CQ_RUN - 1) / CQ_RUN, per_block = 4ull * (64u >> log_l);      // groups of lanes a workgroup holds
  const u32 grid = (u32)std::max<u64>(1, std::min<u64>((groups + per_block - 1) / per_block, (u64)std::max(n_cu, 1u) * 8));
#define KMX_CQG(LL) hipLaunchKernelGGL((k_cquery_gather<LL>), dim3(grid), dim3(256), 0, st, recs, pstart, n_parts, rows, nb, bitw, n_cols, min_class, hits, (unsigned long long*)sums)
  switch (log_l) {
    case 0: KMX_CQG(0); break; case 1: KMX_CQG(1); break; case 2: KMX_CQG(2); break; case 3: KMX_CQG(3); break;
    case 4: KMX_CQG(4); break; case 5: KMX_CQG(5); break; default: KMX_CQG(6); break;
  }
#undef KMX_CQG
  return hipGetLastError();
}

}  // namespace kmx

using namespace kmx;

// ---- cquery ------------------------------------------------------------------------------------------------------------------------
// kmx_cquery_dev / kmx_cquery_host: query sequences against the counting Bloom matrices of a run.  The shared host path:
// seqquery_host.hpp.
struct kmx_cquery_result : SeqResult {
  u32 nb = 0;                           // bytes of a row: n_cols fields of bitw bits
  u32 *d_kmers = nullptr, *d_hits = nullptr;
  u64* d_sums = nullptr;
};

static u64 cquery_row_bytes(const kmx_cquery_task* K) { return ((u64)K->n_cols * K->bitw + 7) / 8; }

// the query section's limits, the section's own among them where a task with several faults has always met them
static int cquery_check(kmx_ctx* ctx, const kmx_cquery_task* K, const char* who)
{
  const SeqCheck c{ctx, who};
  int rc;
  if ((rc = c.kmer_size(K->kmer_size)) || (rc = c.minim_size(K->minim_size, K->kmer_size)) || (rc = c.nb_parts(K->nb_parts)) || (rc = c.n_cols(K->n_cols)) ||
      (rc = c.tables(K->repart, K->rows)) || (rc = c.reads(K->offsets, K->n_seqs, K->bases)) || (rc = c.window(K->window))) return rc;
  if (K->bitw == 0 || K->bitw > 32) return c.no(KMX_E_INVAL, ": bitw must be in [1, 32]");
  if (K->bitw > 8) return c.no(KMX_E_UNSUPPORTED, ": bitw above 8 (a class never exceeds 32: 6 bits hold every class)");
  if (K->min_class < 1 || K->min_class > (1u << K->bitw) - 1u) return c.no(KMX_E_INVAL, ": min_class must be in [1, 2^bitw - 1]");
  if ((K->hits == nullptr) != (K->sums == nullptr)) return c.no(KMX_E_INVAL, ": hits and sums are both null or both device tables");
  if ((rc = c.window_fits(K->window)) || (rc = c.n_seqs(K->n_seqs)) || (rc = c.row_fits(cquery_row_bytes(K)))) return rc;
  if (K->n_seqs * (u64)K->n_cols >= (1ull << 61)) return c.no(KMX_E_UNSUPPORTED, ": tables of 2^61 cells and more (send the queries in batches)");
  return KMX_OK;
}

// the kernels of one call, queued on ctx->stream; every pointer of K a device pointer but K->rows (a host array of device pointers)
static int cquery_queue(kmx_ctx* ctx, const kmx_cquery_task* K, kmx_cquery_result* R)
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
  const bool own = !K->hits;      // (hits and sums: both or neither, cquery_check)
  R->d_hits = own ? (u32*)R->keep(4 * table) : K->hits;
  R->d_sums = own ? (u64*)R->keep(8 * table) : (u64*)K->sums;
  const int rc = seq_queue_head(R, K->rows, nullptr, 64);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_cell, 0, 4 * cells, st));
  KMX_HIP(ctx, hipMemsetAsync(d_pstart, 0, 4ull * (P + 1), st));
  if (n_seqs) KMX_HIP(ctx, hipMemsetAsync(R->d_kmers, 0, 4ull * n_seqs, st));
  if (own && table) {
    KMX_HIP(ctx, hipMemsetAsync(R->d_hits, 0, 4 * table, st));
    KMX_HIP(ctx, hipMemsetAsync(R->d_sums, 0, 8 * table, st));
  }
  if (n_bases) {
    KMX_HIP(ctx, launch_query_keys((int)kw, K->bases, (const u64*)K->offsets, n_seqs, n_bases, (int)K->kmer_size, (int)K->minim_size, K->repart, K->window,
                                   n_tiles, n_chunks, tpc, d_keys, d_cell, R->d_kmers, st));
    KMX_HIP(ctx, launch_filter_scan(d_cell, (u32)(cells - 1), st));
    KMX_HIP(ctx, launch_query_parts(d_cell, P, n_chunks, d_pstart, st));
    KMX_HIP(ctx, launch_query_scatter(d_keys, (const u64*)K->offsets, n_seqs, n_bases, n_tiles, n_chunks, tpc, d_cell, d_recs, st));
    KMX_HIP(ctx, launch_cquery_gather(d_recs, n_bases, d_pstart, P, R->d_rows, nb, K->bitw, N, K->min_class, R->d_hits, R->d_sums, (u32)kmx_plan_cus(ctx), st));
  }
  return seq_queue_tail(R, d_pstart + P, 1);      // h_tot[0]: the valid k-mers of the call
}

static int cquery_call(kmx_ctx* ctx, const kmx_cquery_task* task, kmx_cquery_result** out, bool host, const char* who)
{
  u64 n_bases = 0;
  int rc = seq_args(ctx, task, out, who);
  if (rc == KMX_OK) rc = cquery_check(ctx, task, who);
  if (rc == KMX_OK) rc = seq_n_bases(ctx, task->offsets, task->n_seqs, host, who, &n_bases);
  if (rc != KMX_OK) return rc;
  kmx_cquery_result* R = new kmx_cquery_result();
  R->init(ctx, "kmx_cquery", *task, n_bases); R->nb = (u32)cquery_row_bytes(task);
  kmx_cquery_task dt = *task;
  std::vector<const uint8_t*> drows(task->nb_parts, nullptr);
  if (host) rc = seq_upload(R, &dt, drows, who, [&](u32) { return task->window * R->nb; });
  if (rc == KMX_OK) rc = cquery_queue(ctx, &dt, R);
  return seq_finish(R, rc, host, out);
}
extern "C" int kmx_cquery_dev(kmx_ctx* ctx, const kmx_cquery_task* task, kmx_cquery_result** out) { return cquery_call(ctx, task, out, false, "kmx_cquery_dev"); }
extern "C" int kmx_cquery_host(kmx_ctx* ctx, const kmx_cquery_task* task, kmx_cquery_result** out) { return cquery_call(ctx, task, out, true, "kmx_cquery_host"); }

extern "C" int kmx_cquery_result_wait(kmx_cquery_result* R) { return seq_wait(R); }
extern "C" uint64_t kmx_cquery_result_n_seqs(const kmx_cquery_result* R) { return R ? R->n_seqs : 0; }
extern "C" int kmx_cquery_result_copy_kmers(kmx_cquery_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? seq_copy_out(R, host_dst, dst_entries, R->d_kmers, R->n_seqs, 4) : KMX_E_INVAL; }
extern "C" int kmx_cquery_result_copy_hits(kmx_cquery_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? seq_copy_out(R, host_dst, dst_entries, R->d_hits, R->n_seqs * R->n_cols, 4) : KMX_E_INVAL; }
extern "C" int kmx_cquery_result_copy_sums(kmx_cquery_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? seq_copy_out(R, host_dst, dst_entries, R->d_sums, R->n_seqs * R->n_cols, 8) : KMX_E_INVAL; }
extern "C" uint32_t* kmx_cquery_result_hits_dev(kmx_cquery_result* R) { return R && seq_wait(R) == KMX_OK ? R->d_hits : nullptr; }
extern "C" uint64_t* kmx_cquery_result_sums_dev(kmx_cquery_result* R) { return R && seq_wait(R) == KMX_OK ? (uint64_t*)R->d_sums : nullptr; }
extern "C" double kmx_cquery_result_kernel_ms(kmx_cquery_result* R) { return seq_kernel_ms(R); }
extern "C" uint64_t kmx_cquery_result_algo_bytes(kmx_cquery_result* R)
{ return R && seq_wait(R) == KMX_OK ? R->n_bases + (u64)R->h_tot[0] * R->nb + 12 * R->n_seqs * R->n_cols : 0; }
extern "C" void kmx_cquery_result_free(kmx_cquery_result* R) { seq_free(R); }
