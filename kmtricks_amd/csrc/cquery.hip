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
#include "kmx_host.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 CQ_RUN = 128;               // records of a gather item: 128 x 2^31 fits a u64 sum, 128 a u32 hit counter

struct __attribute__((packed, aligned(1))) CQDword { u32 v; };      // a dword at any address: one global_load_dword
struct __attribute__((packed, aligned(1))) CQShort { u16 v; };      // two bytes at any address: one global_load_ushort

// the w bytes (1 ... 8) at rp as one big-endian number, in pieces of 4, 2 and 1 bytes (w is the same in every lane: no divergence)
__device__ __forceinline__ u64 cq_load_be(const u8* rp, u32 w)
{
  u64 x = 0;
  if (w == 8) { x = __builtin_bswap32(reinterpret_cast<const CQDword*>(rp)->v); rp += 4; w = 4; }
  if (w & 4u) { x = (x << 32) | __builtin_bswap32(reinterpret_cast<const CQDword*>(rp)->v); rp += 4; }
  if (w & 2u) { x = (x << 16) | __builtin_bswap16(reinterpret_cast<const CQShort*>(rp)->v); rp += 2; }
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
// kmx_cquery_dev / kmx_cquery_host: query sequences against the counting Bloom matrices of a run.
struct kmx_cquery_result {
  kmx_ctx* ctx = nullptr;
  u64 n_seqs = 0, n_bases = 0;
  u32 n_cols = 0, nb = 0, n_parts = 0;
  u64 *d_keys = nullptr, *d_recs = nullptr, *d_sums_own = nullptr, *d_sums = nullptr;
  u32 *d_cell = nullptr, *d_pstart = nullptr, *d_kmers = nullptr, *d_hits_own = nullptr, *d_hits = nullptr;
  const u8** d_rows = nullptr;
  const u8** h_rows = nullptr;          // page-locked: the row pointers on their way up
  std::vector<void*> d_in;              // kmx_cquery_host: the uploads
  u32* h_tot = nullptr;                 // page-locked: [0] valid k-mers of the call
  hipEvent_t ev_in = nullptr, ev_done = nullptr, ev0 = nullptr, ev1 = nullptr;
  bool waited = false; int status = KMX_OK;
};

static u64 cquery_row_bytes(const kmx_cquery_task* K) { return ((u64)K->n_cols * K->bitw + 7) / 8; }

// the query section's limits, then the section's own
static int cquery_check(kmx_ctx* ctx, const kmx_cquery_task* K, const char* who)
{
  const std::string w(who);
  if (K->kmer_size < 8 || K->kmer_size > 127) return ctx->fail(KMX_E_INVAL, w + ": kmer_size must be in [8, 127]");
  if (K->minim_size < 4 || K->minim_size > 15 || K->minim_size >= K->kmer_size) return ctx->fail(KMX_E_INVAL, w + ": minim_size must be in [4, 15] and below kmer_size");
  if (K->nb_parts < 1 || K->nb_parts > 65535) return ctx->fail(KMX_E_INVAL, w + ": nb_parts must be in [1, 65535]");
  if (K->n_cols == 0) return ctx->fail(KMX_E_INVAL, w + ": a matrix has at least one column");
  if (!K->repart || !K->rows) return ctx->fail(KMX_E_INVAL, w + ": null repartition table or row pointer array");
  if (!K->offsets || (K->n_seqs && !K->bases)) return ctx->fail(KMX_E_INVAL, w + ": null reads");
  if (K->window == 0) return ctx->fail(KMX_E_INVAL, w + ": a window has at least one row");
  if (K->bitw == 0 || K->bitw > 32) return ctx->fail(KMX_E_INVAL, w + ": bitw must be in [1, 32]");
  if (K->bitw > 8) return ctx->fail(KMX_E_UNSUPPORTED, w + ": bitw above 8 (a class never exceeds 32: 6 bits hold every class)");
  if (K->min_class < 1 || K->min_class > (1u << K->bitw) - 1u) return ctx->fail(KMX_E_INVAL, w + ": min_class must be in [1, 2^bitw - 1]");
  if ((K->hits == nullptr) != (K->sums == nullptr)) return ctx->fail(KMX_E_INVAL, w + ": hits and sums are both null or both device tables");
  if (K->window > 0xFFFFFFFFull) return ctx->fail(KMX_E_UNSUPPORTED, w + ": windows of 2^32 rows and more");
  if (K->n_seqs >= (1ull << 31)) return ctx->fail(KMX_E_UNSUPPORTED, w + ": 2^31 queries and more in one call (send them in batches)");
  if (cquery_row_bytes(K) > 0xFFFFFFFFull) return ctx->fail(KMX_E_UNSUPPORTED, w + ": rows of 4 GiB and more");
  if (K->n_seqs * (u64)K->n_cols >= (1ull << 61)) return ctx->fail(KMX_E_UNSUPPORTED, w + ": tables of 2^61 cells and more (send the queries in batches)");
  return KMX_OK;
}

static void cquery_release(kmx_cquery_result* R)
{
  kmx_ctx* c = R->ctx;
  void* blocks[] = {R->d_keys, R->d_recs, R->d_cell, R->d_pstart, R->d_kmers, R->d_hits_own, R->d_sums_own, (void*)R->d_rows};
  for (void* p : blocks) c->dfree(p);
  for (void* p : R->d_in) c->dfree(p);
  c->hfree(R->h_tot); c->hfree((void*)R->h_rows);
  for (hipEvent_t e : {R->ev_in, R->ev_done, R->ev0, R->ev1}) if (e) (void)hipEventDestroy(e);
  delete R;
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
  if (!(R->h_tot = (u32*)ctx->halloc(64)) || !(R->h_rows = (const u8**)ctx->halloc(8ull * P))) return ctx->fail(KMX_E_NOMEM, "kmx_cquery: host allocation failed");
  R->h_tot[0] = 0;
  for (u32 p = 0; p < P; p++) R->h_rows[p] = K->rows[p];
  R->d_keys = (u64*)ctx->dalloc(8 * n_bases);
  R->d_recs = (u64*)ctx->dalloc(8 * n_bases);
  R->d_cell = (u32*)ctx->dalloc(4 * cells);
  R->d_pstart = (u32*)ctx->dalloc(4ull * (P + 1));
  R->d_kmers = (u32*)ctx->dalloc(4ull * n_seqs);
  R->d_rows = (const u8**)ctx->dalloc(8ull * P);
  R->d_hits = K->hits; R->d_sums = (u64*)K->sums;
  if (!R->d_hits) {      // (both or neither: cquery_check)
    R->d_hits = R->d_hits_own = (u32*)ctx->dalloc(4 * table);
    R->d_sums = R->d_sums_own = (u64*)ctx->dalloc(8 * table);
  }
  if (!R->d_keys || !R->d_recs || !R->d_cell || !R->d_pstart || !R->d_kmers || !R->d_rows || !R->d_hits || !R->d_sums)
    return ctx->fail(KMX_E_NOMEM, "kmx_cquery: device allocation failed");
  KMX_HIP(ctx, hipMemcpyAsync((void*)R->d_rows, (const void*)R->h_rows, 8ull * P, hipMemcpyHostToDevice, st));
  if (ctx->profiling) {
    KMX_HIP(ctx, hipEventCreate(&R->ev0)); KMX_HIP(ctx, hipEventCreate(&R->ev1));
    KMX_HIP(ctx, hipEventRecord(R->ev0, st));
  }
  KMX_HIP(ctx, hipMemsetAsync(R->d_cell, 0, 4 * cells, st));
  KMX_HIP(ctx, hipMemsetAsync(R->d_pstart, 0, 4ull * (P + 1), st));
  if (n_seqs) KMX_HIP(ctx, hipMemsetAsync(R->d_kmers, 0, 4ull * n_seqs, st));
  if (R->d_hits_own && table) {
    KMX_HIP(ctx, hipMemsetAsync(R->d_hits_own, 0, 4 * table, st));
    KMX_HIP(ctx, hipMemsetAsync(R->d_sums_own, 0, 8 * table, st));
  }
  if (n_bases) {
    KMX_HIP(ctx, launch_query_keys((int)kw, K->bases, (const u64*)K->offsets, n_seqs, n_bases, (int)K->kmer_size, (int)K->minim_size, K->repart, K->window,
                                   n_tiles, n_chunks, tpc, R->d_keys, R->d_cell, R->d_kmers, st));
    KMX_HIP(ctx, launch_filter_scan(R->d_cell, (u32)(cells - 1), st));
    KMX_HIP(ctx, launch_query_parts(R->d_cell, P, n_chunks, R->d_pstart, st));
    KMX_HIP(ctx, launch_query_scatter(R->d_keys, (const u64*)K->offsets, n_seqs, n_bases, n_tiles, n_chunks, tpc, R->d_cell, R->d_recs, st));
    KMX_HIP(ctx, launch_cquery_gather(R->d_recs, n_bases, R->d_pstart, P, R->d_rows, nb, K->bitw, N, K->min_class, R->d_hits, R->d_sums, (u32)ctx->n_cu, st));
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev1, st));
  KMX_HIP(ctx, hipMemcpyAsync(&R->h_tot[0], R->d_pstart + P, 4, hipMemcpyDeviceToHost, st));
  KMX_HIP(ctx, hipEventCreateWithFlags(&R->ev_done, hipEventDisableTiming));
  KMX_HIP(ctx, hipEventRecord(R->ev_done, st));
  return KMX_OK;
}

static kmx_cquery_result* cquery_new(kmx_ctx* ctx, const kmx_cquery_task* K, u64 n_bases)
{
  kmx_cquery_result* R = new kmx_cquery_result();
  R->ctx = ctx; R->n_seqs = K->n_seqs; R->n_bases = n_bases; R->n_cols = K->n_cols; R->nb = (u32)cquery_row_bytes(K); R->n_parts = K->nb_parts;
  return R;
}

extern "C" int kmx_cquery_dev(kmx_ctx* ctx, const kmx_cquery_task* task, kmx_cquery_result** out)
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, "kmx_cquery_dev: null argument");
  *out = nullptr;
  int rc = cquery_check(ctx, task, "kmx_cquery_dev");
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  u64 ends[1] = {0};      // the grid's size: the end of the last query
  KMX_HIP(ctx, hipMemcpyAsync(ends, task->offsets + task->n_seqs, 8, hipMemcpyDeviceToHost, ctx->stream));
  KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ends[0] > 0xFFFFFFFFull) return ctx->fail(KMX_E_UNSUPPORTED, "kmx_cquery_dev: 2^32 bases and more in one call (send the queries in batches)");
  kmx_cquery_result* R = cquery_new(ctx, task, ends[0]);
  if ((rc = cquery_queue(ctx, task, R)) != KMX_OK) { (void)hipStreamSynchronize(ctx->stream); cquery_release(R); return rc; }
  *out = R;
  return KMX_OK;
}

extern "C" int kmx_cquery_host(kmx_ctx* ctx, const kmx_cquery_task* task, kmx_cquery_result** out)
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, "kmx_cquery_host: null argument");
  *out = nullptr;
  int rc = cquery_check(ctx, task, "kmx_cquery_host");
  if (rc != KMX_OK) return rc;
  const u64 n_bases = task->offsets[task->n_seqs];
  if (task->offsets[0] != 0) return ctx->fail(KMX_E_INVAL, "kmx_cquery_host: offsets[0] must be 0");
  for (u64 i = 0; i < task->n_seqs; i++) if (task->offsets[i] > task->offsets[i + 1]) return ctx->fail(KMX_E_INVAL, "kmx_cquery_host: offsets must not descend");
  if (n_bases > 0xFFFFFFFFull) return ctx->fail(KMX_E_UNSUPPORTED, "kmx_cquery_host: 2^32 bases and more in one call (send the queries in batches)");
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  kmx_cquery_result* R = cquery_new(ctx, task, n_bases);
  kmx_cquery_task dt = *task;
  std::vector<const uint8_t*> drows(task->nb_parts, nullptr);
  auto fail = [&](int code) { (void)hipStreamSynchronize(ctx->up); (void)hipStreamSynchronize(ctx->stream); cquery_release(R); return code; };
  hipError_t e = hipSuccess;
  auto upload = [&](const void* src, u64 bytes) -> void* {
    void* d = ctx->dalloc(bytes);
    if (!d) return nullptr;
    R->d_in.push_back(d);
    if (bytes && e == hipSuccess) e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->up);
    return d;
  };
  const u64 body_bytes = task->window * cquery_row_bytes(task);
  if (!(dt.bases = (const char*)upload(task->bases, n_bases)) || !(dt.offsets = (const uint64_t*)upload(task->offsets, 8 * (task->n_seqs + 1))) ||
      !(dt.repart = (const uint16_t*)upload(task->repart, 2ull << (2 * task->minim_size))))
    return fail(ctx->fail(KMX_E_NOMEM, "kmx_cquery_host: upload allocation failed"));
  for (u32 p = 0; p < task->nb_parts; p++) {
    if (!task->rows[p]) continue;
    if (!(drows[p] = (const uint8_t*)upload(task->rows[p], body_bytes))) return fail(ctx->fail(KMX_E_NOMEM, "kmx_cquery_host: upload allocation failed"));
  }
  dt.rows = drows.data();
  if (e == hipSuccess) e = hipEventCreateWithFlags(&R->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(R->ev_in, ctx->up);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, R->ev_in, 0);
  if (e != hipSuccess) return fail(ctx->fail(KMX_E_HIP, std::string("kmx_cquery_host: upload: ") + hipGetErrorString(e)));
  if ((rc = cquery_queue(ctx, &dt, R)) != KMX_OK) return fail(rc);
  *out = R;
  return KMX_OK;
}

extern "C" int kmx_cquery_result_wait(kmx_cquery_result* R)
{
  if (!R) return KMX_E_INVAL;
  if (R->waited) return R->status;
  R->waited = true;
  const hipError_t e = hipEventSynchronize(R->ev_done);
  if (e != hipSuccess) return R->status = R->ctx->fail(KMX_E_HIP, std::string("kmx_cquery: ") + hipGetErrorString(e));
  // the call has run: its scratch and uploads go back to the pool; n_kmers and the tables stay (a result kept as the accumulator of
  // later partition groups holds nothing else)
  kmx_ctx* c = R->ctx;
  void* scratch[] = {R->d_keys, R->d_recs, R->d_cell, R->d_pstart, (void*)R->d_rows};
  for (void* p : scratch) c->dfree(p);
  R->d_keys = R->d_recs = nullptr; R->d_cell = R->d_pstart = nullptr; R->d_rows = nullptr;
  for (void* p : R->d_in) c->dfree(p);
  R->d_in.clear();
  c->hfree((void*)R->h_rows); R->h_rows = nullptr;
  return R->status = KMX_OK;
}
extern "C" uint64_t kmx_cquery_result_n_seqs(const kmx_cquery_result* R) { return R ? R->n_seqs : 0; }
static int cquery_copy_out(kmx_cquery_result* R, void* dst, uint64_t dst_entries, const void* src, u64 entries, u32 entry_bytes)
{
  const int rc = kmx_cquery_result_wait(R);
  if (rc != KMX_OK) return rc;
  if (dst_entries < entries) return R->ctx->fail(KMX_E_INVAL, "destination too small");
  if (!entries) return KMX_OK;
  if (!dst) return R->ctx->fail(KMX_E_INVAL, "null destination");
  return kmx_copy_to_host(R->ctx, dst, src, (u64)entry_bytes * entries);
}
extern "C" int kmx_cquery_result_copy_kmers(kmx_cquery_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? cquery_copy_out(R, host_dst, dst_entries, R->d_kmers, R->n_seqs, 4) : KMX_E_INVAL; }
extern "C" int kmx_cquery_result_copy_hits(kmx_cquery_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? cquery_copy_out(R, host_dst, dst_entries, R->d_hits, R->n_seqs * R->n_cols, 4) : KMX_E_INVAL; }
extern "C" int kmx_cquery_result_copy_sums(kmx_cquery_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? cquery_copy_out(R, host_dst, dst_entries, R->d_sums, R->n_seqs * R->n_cols, 8) : KMX_E_INVAL; }
extern "C" uint32_t* kmx_cquery_result_hits_dev(kmx_cquery_result* R) { return R && kmx_cquery_result_wait(R) == KMX_OK ? R->d_hits : nullptr; }
extern "C" uint64_t* kmx_cquery_result_sums_dev(kmx_cquery_result* R) { return R && kmx_cquery_result_wait(R) == KMX_OK ? (uint64_t*)R->d_sums : nullptr; }
extern "C" double kmx_cquery_result_kernel_ms(kmx_cquery_result* R)
{
  if (!R || !R->ev0 || !R->ev1 || kmx_cquery_result_wait(R) != KMX_OK) return -1.0;
  float ms = 0;
  return hipEventElapsedTime(&ms, R->ev0, R->ev1) == hipSuccess ? (double)ms : -1.0;
}
extern "C" uint64_t kmx_cquery_result_algo_bytes(kmx_cquery_result* R)
{ return R && kmx_cquery_result_wait(R) == KMX_OK ? R->n_bases + (u64)R->h_tot[0] * R->nb + 12 * R->n_seqs * R->n_cols : 0; }
extern "C" void kmx_cquery_result_free(kmx_cquery_result* R)
{
  if (!R) return;
  (void)hipSetDevice(R->ctx->device);
  if (R->ev_done) (void)hipEventSynchronize(R->ev_done);
  cquery_release(R);
}
