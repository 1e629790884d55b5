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
#include "seqquery_host.hpp"
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
        if (4u * ws + 4u <= nb) x = reinterpret_cast<const UDword*>(rp)->v;
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

using namespace kmx;

// ---- zquery ------------------------------------------------------------------------------------------------------------------------
// kmx_zquery_dev / kmx_zquery_host: the (k + z)-mers of query sequences against the Bloom matrices of a run.  The shared host path:
// seqquery_host.hpp; h_tot holds the first record of every partition, [n_parts] the valid k-mers of the call.
struct kmx_zquery_result : SeqResult {
  u32 nb = 0, pitch = 0, z = 0;
  bool last = false;
  u32 *d_kmers = nullptr, *d_hits = nullptr;      // (the last call of a series only)
  u8* d_bits = nullptr;                           // the series' table: the result's own (a series' first call) or the caller's
  std::vector<bool> in_call;                      // partition p is part of the call
};

extern "C" uint64_t kmx_zquery_bits_bytes(uint64_t n_bases, uint32_t n_cols)
{ return n_bases * (4ull * ((((u64)n_cols + 7) / 8 + 3) / 4)); }

// the kernels of one call, queued on ctx->stream; every pointer of K a device pointer but K->rows (a host array of device pointers)
static int zquery_queue(kmx_ctx* ctx, const kmx_zquery_task* K, kmx_zquery_result* R)
{
  hipStream_t st = ctx->stream;
  const u64 n_bases = R->n_bases;
  const u32 n_seqs = (u32)R->n_seqs, P = K->nb_parts, N = K->n_cols, nb = R->nb, kw = (K->kmer_size + 31) / 32;
  u32 n_tiles = 0, n_chunks = 1, tpc = 1;
  query_chunks(n_bases, P, &n_tiles, &n_chunks, &tpc);
  const u64 cells = (u64)P * n_chunks + 1, table = (u64)n_seqs * N, bits_bytes = kmx_zquery_bits_bytes(n_bases, N);
  R->in_call.assign(P, false);
  for (u32 p = 0; p < P; p++) R->in_call[p] = K->rows[p] != nullptr;
  u64* d_keys = (u64*)R->tmp(8 * n_bases);
  u64* d_recs = (u64*)R->tmp(8 * n_bases);
  u32* d_cell = (u32*)R->tmp(4 * cells);
  u32* d_pstart = (u32*)R->tmp(4ull * (P + 1));
  u32* d_kcount = (u32*)R->tmp(4ull * n_seqs);      // k_query_keys' k-mers per query (the result counts K-positions)
  u8* bits_own = K->bits ? nullptr : (u8*)R->keep(bits_bytes);
  R->d_bits = K->bits ? K->bits : bits_own;
  u32* hits_own = nullptr;
  if (R->last) {
    R->d_kmers = (u32*)R->keep(4ull * n_seqs);
    if (!K->hits) hits_own = (u32*)R->keep(4 * table);
    R->d_hits = K->hits ? K->hits : hits_own;
  }
  const int rc = seq_queue_head(R, K->rows, nullptr, 4ull * (P + 1));
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_cell, 0, 4 * cells, st));
  KMX_HIP(ctx, hipMemsetAsync(d_pstart, 0, 4ull * (P + 1), st));
  if (n_seqs) KMX_HIP(ctx, hipMemsetAsync(d_kcount, 0, 4ull * n_seqs, st));
  if (bits_own && bits_bytes) KMX_HIP(ctx, hipMemsetAsync(bits_own, 0, bits_bytes, st));
  if (R->last && n_seqs) KMX_HIP(ctx, hipMemsetAsync(R->d_kmers, 0, 4ull * n_seqs, st));
  if (hits_own && table) KMX_HIP(ctx, hipMemsetAsync(hits_own, 0, 4 * table, st));
  if (n_bases) {
    KMX_HIP(ctx, launch_query_keys((int)kw, K->bases, (const u64*)K->offsets, n_seqs, n_bases, (int)K->kmer_size, (int)K->minim_size, K->repart, K->window,
                                   n_tiles, n_chunks, tpc, d_keys, d_cell, d_kcount, st));
    KMX_HIP(ctx, launch_filter_scan(d_cell, (u32)(cells - 1), st));
    KMX_HIP(ctx, launch_query_parts(d_cell, P, n_chunks, d_pstart, st));
    KMX_HIP(ctx, launch_zquery_scatter(d_keys, n_bases, n_tiles, n_chunks, tpc, d_cell, d_recs, st));
    KMX_HIP(ctx, launch_zquery_rows(d_recs, n_bases, d_pstart, P, R->d_rows, nb, N, R->d_bits, (u32)kmx_plan_cus(ctx), st));
    if (R->last)
      KMX_HIP(ctx, launch_zquery_window(d_keys, (const u64*)K->offsets, n_seqs, n_bases, K->z, R->d_bits, nb, N, R->d_kmers, R->d_hits, (u32)kmx_plan_cus(ctx), st));
  }
  return seq_queue_tail(R, d_pstart, P + 1);
}

static int zquery_call(kmx_ctx* ctx, const kmx_zquery_task* task, kmx_zquery_result** out, bool host, const char* who)
{
  u64 n_bases = 0;
  int rc = seq_args(ctx, task, out, who);
  if (rc == KMX_OK) rc = seq_check_bloom(ctx, task, who);      // the query section's limits, then the section's own
  if (rc == KMX_OK && (task->z > 8 || task->z >= task->kmer_size)) rc = ctx->fail(KMX_E_INVAL, std::string(who) + ": z must be in [0, 8] and below kmer_size");
  if (rc == KMX_OK) rc = seq_n_bases(ctx, task->offsets, task->n_seqs, host, who, &n_bases);
  if (rc == KMX_OK && kmx_zquery_bits_bytes(n_bases, task->n_cols) > (1ull << 40))
    rc = ctx->fail(KMX_E_UNSUPPORTED, std::string(who) + ": a bits table of more than 2^40 bytes (send the queries in batches)");
  if (rc != KMX_OK) return rc;
  kmx_zquery_result* R = new kmx_zquery_result();
  R->init(ctx, "kmx_zquery", *task, n_bases); R->nb = (task->n_cols + 7) / 8;
  R->pitch = (u32)kmx_zquery_bits_bytes(1, task->n_cols); R->z = task->z; R->last = task->last != 0;
  kmx_zquery_task dt = *task;
  std::vector<const uint8_t*> drows(task->nb_parts, nullptr);
  if (host) rc = seq_upload(R, &dt, drows, who, [&](u32) { return task->window * R->nb; });
  if (rc == KMX_OK) rc = zquery_queue(ctx, &dt, R);
  return seq_finish(R, rc, host, out);
}
extern "C" int kmx_zquery_dev(kmx_ctx* ctx, const kmx_zquery_task* task, kmx_zquery_result** out) { return zquery_call(ctx, task, out, false, "kmx_zquery_dev"); }
extern "C" int kmx_zquery_host(kmx_ctx* ctx, const kmx_zquery_task* task, kmx_zquery_result** out) { return zquery_call(ctx, task, out, true, "kmx_zquery_host"); }

extern "C" int kmx_zquery_result_wait(kmx_zquery_result* R) { return seq_wait(R); }
extern "C" uint64_t kmx_zquery_result_n_seqs(const kmx_zquery_result* R) { return R ? R->n_seqs : 0; }
static int zquery_copy_out(kmx_zquery_result* R, void* dst, uint64_t dst_entries, const void* src, u64 entries)
{
  const int rc = seq_wait(R);
  if (rc != KMX_OK) return rc;
  if (!R->last) return R->ctx->fail(KMX_E_INVAL, "kmx_zquery: n_kmers and hits belong to the last call of a series");
  return seq_copy_out(R, dst, dst_entries, src, entries, 4);
}
extern "C" int kmx_zquery_result_copy_kmers(kmx_zquery_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? zquery_copy_out(R, host_dst, dst_entries, R->d_kmers, R->n_seqs) : KMX_E_INVAL; }
extern "C" int kmx_zquery_result_copy_hits(kmx_zquery_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? zquery_copy_out(R, host_dst, dst_entries, R->d_hits, R->n_seqs * R->n_cols) : KMX_E_INVAL; }
extern "C" uint32_t* kmx_zquery_result_hits_dev(kmx_zquery_result* R) { return R && R->last && seq_wait(R) == KMX_OK ? R->d_hits : nullptr; }
extern "C" uint8_t* kmx_zquery_result_bits_dev(kmx_zquery_result* R) { return R && seq_wait(R) == KMX_OK ? R->d_bits : nullptr; }
extern "C" double kmx_zquery_result_kernel_ms(kmx_zquery_result* R) { return seq_kernel_ms(R); }
extern "C" uint64_t kmx_zquery_result_algo_bytes(kmx_zquery_result* R)
{
  if (!R || seq_wait(R) != KMX_OK) return 0;
  u64 found = 0;
  for (u32 p = 0; p < R->n_parts; p++) if (R->in_call[p]) found += R->h_tot[p + 1] - R->h_tot[p];
  u64 bytes = R->n_bases + found * ((u64)R->nb + R->pitch);
  if (R->last) {
    std::vector<u32> nk(R->n_seqs);
    if (R->n_seqs && kmx_copy_to_host(R->ctx, nk.data(), R->d_kmers, 4 * R->n_seqs) != KMX_OK) return 0;
    u64 rows = 0;
    for (u32 n : nk) if (n) rows += (u64)n + R->z;
    bytes += rows * R->pitch + 4 * R->n_seqs * R->n_cols;
  }
  return bytes;
}
extern "C" void kmx_zquery_result_free(kmx_zquery_result* R) { seq_free(R); }
