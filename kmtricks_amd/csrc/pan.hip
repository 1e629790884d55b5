// pan.hip -- `kmx pan` on the device: how the recurrences of a matrix's rows are distributed over a list of samples (include/kmx.h,
// section "pan"; what pangrowth and Panacus `hist` / `histgrowth` / `ordered-histgrowth` compute from a k-mer x sample matrix).  No
// reference counterpart in the kmtricks tree.  gfx950, wave64.
//
//   k_pan_score   k_select_score's decomposition: a wave a chunk of rows; a row of 64 units and more (a unit: a count, or a payload
//                 byte) is read by the whole wave, shorter rows by the L lanes of a sub-group, 64 / L rows at a time.  Three butterflies
//                 over the row's lanes: add for rec, min for first, min for gap; the operand of the mins is the column's ordinal in the
//                 list, from a table per INPUT column (PN_NONE: not listed; padded to whole bytes of 8 columns).  Lane i of the wave
//                 ends with row i of the chunk and adds 1 to three histograms: in LDS (u32, atomicAdd) while 3 (M + 1) words fit
//                 PN_LDS_WORDS, flushed once a workgroup, non-zero bins only, with 64-bit global atomics -- the grid is persistent and
//                 strides over the chunks --; beyond that M straight into the table with three global atomics a row.  With SHARED it
//                 also writes rec[row].  The histograms go to a CALL-LOCAL table: the caller's may hold other partitions.
//   k_pan_fold    one workgroup: the call-local table added into the caller's; with SHARED the exclusive scan of the recurrence bins
//                 (the first place of every recurrence class in the order).
//   k_pan_order   SHARED: a counting-sort scatter of (row, rec) into recurrence order.  A wave loops over its distinct rec values
//                 (ballot of the lanes that share the first one's, one atomic add of their number): most rows of a real matrix share
//                 r = 1 or r = M, and one atomic a row on one address is the contended shape.  The order inside a class is whatever
//                 arrives: the results are integer sums.
//   k_pan_shared  SHARED: a workgroup takes a run of PN_RUN consecutive places of the order (read into LDS once) and a block of 256
//                 units: a lane a column (COUNT; the workgroup reads 1 KB of a row at a time) or a payload byte with 8 accumulators
//                 (PA).  It sums in u32 registers while rec stays the same -- rec is uniform over the workgroup, it comes from the
//                 order -- and flushes the non-zero sums to shared[rec][c] with 64-bit atomicAdd when rec changes and at the run's end.
//                 COUNT: a wave's flush is 512 contiguous bytes.  PA: the flush is strided by 8 columns a lane (flushes are few: at most
//                 runs + M + 1 a column; no transpose through LDS).
// No kernel waits on another workgroup: any grid is a correct one.
// Every load of a body byte is inside [rows, rows + n_rows * row_bytes): an address is rows + r * row_bytes + skip + b with r < n_rows
// and b + (bytes loaded) <= row_bytes - skip, both tested by the lane that loads; nothing is loaded in wider pieces than the piece that
// is tested and nothing is rounded to an aligned address.  Every (row, rec) that k_pan_shared takes from the order is tested again
// (row < n_rows, rec <= M) before it becomes an address.  The launch knobs of this file are its own: KMX_PAN_CUS and KMX_PAN_GRID.
#include "matrix_host.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 PN_NONE = 0xFFFFFFFFu;      // the ordinal of a column that is not listed (M <= 2^32 - 1)
constexpr u32 PN_LDS_WORDS = 12288;       // 48 KB: the three histograms live in LDS while 3 (M + 1) <= this, M <= 4095
constexpr u32 PN_WGS_PER_CU = 8;          // k_pan_score's persistent grid: workgroups a CU
constexpr u32 PN_MAX_GRID = 1u << 16;     // workgroups of a launch: the kernels stride over their work
constexpr u32 PN_WAVES_PER_SIMD = 8;      // chunks of long rows are made small enough for this many waves a SIMD
constexpr u32 PN_RUN = 256;               // places of the order a workgroup of k_pan_shared sums before it must flush
constexpr u32 PN_BLOCK = 256;             // units of a row a workgroup of k_pan_shared takes: a lane a unit

static_assert(sizeof(kmx_pan_task) == 64, "kmx_pan_task is 64 bytes");

// ordt: the ordinal of every input column in the list, PN_NONE where it is not listed, 8 * ceil(N / 8) entries.
// L: lanes of a row (a power of two <= 64); RW: rows of a wave's chunk (64 when L < 64; a power of two <= 64 when L == 64).
// loc: the call-local u64 table [3][M + 1]; recv: null without SHARED.  Dynamic LDS: 3 (M + 1) words when use_lds.
template <bool COUNT>
__global__ __launch_bounds__(256)
void k_pan_score(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 M, u32 L, u32 RW, const u32* __restrict__ ordt,
                 u32 a, u32 use_lds, u64* __restrict__ loc, u32* __restrict__ recv)
{
  extern __shared__ u32 s_hist[];
  const u32 lane = threadIdx.x & 63u, u = lane & (L - 1u), sub = lane / L;
  const u32 units = COUNT ? N : (u32)(((u64)N + 7) / 8);
  const u32 passes = L == 64 ? RW : L;
  const u64 n_chunks = ((u64)n_rows + RW - 1) / RW;
  const u64 M1 = (u64)M + 1;
  if (use_lds) {
    for (u32 i = threadIdx.x; i < 3 * (M + 1); i += 256) s_hist[i] = 0;
    __syncthreads();
  }
  for (u64 g = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; g < n_chunks; g += (u64)gridDim.x * 4) {
    const u64 row0 = g * RW;
    u32 rec = 0, fst = M, gap = M;
    for (u32 p = 0; p < passes; p++) {
      const u64 row = row0 + (u64)sub * L + p;
      u32 acc = 0, f = M, h = M;
      if (row < n_rows) {
        const u8* q = rows + row * row_bytes + skip;
        for (u64 un = u; un < units; un += L) {
          if (COUNT) {
            const u32 v = reinterpret_cast<const UDword*>(q + 4 * un)->v;
            const u32 o = ordt[un];
            const bool pres = v >= a;
            acc += (u32)(pres && o != PN_NONE);
            f = min(f, pres ? o : PN_NONE);
            h = min(h, pres ? PN_NONE : o);
          } else {
            const u32 x = q[un];
            const u32* ot = ordt + 8 * un;
#pragma unroll
            for (u32 k = 0; k < 8; k++) {
              const u32 o = ot[k];
              const bool pres = (x >> k) & 1u;
              acc += (u32)(pres && o != PN_NONE);
              f = min(f, pres ? o : PN_NONE);
              h = min(h, pres ? PN_NONE : o);
            }
          }
        }
      }
      for (u32 o = L >> 1; o; o >>= 1) {
        acc += __shfl_xor(acc, (int)o);
        f = min(f, (u32)__shfl_xor(f, (int)o));
        h = min(h, (u32)__shfl_xor(h, (int)o));
      }
      if (u == p) { rec = acc; fst = f; gap = h; }
    }
    // lane i holds row row0 + i
    const u64 mine = row0 + lane;
    if (lane < RW && mine < n_rows) {
      if (recv) recv[mine] = rec;
      if (use_lds) {
        atomicAdd(&s_hist[rec], 1u);
        atomicAdd(&s_hist[M + 1 + fst], 1u);
        atomicAdd(&s_hist[2 * (M + 1) + gap], 1u);
      } else {
        atomicAdd(&loc[rec], 1ull);
        atomicAdd(&loc[M1 + fst], 1ull);
        atomicAdd(&loc[2 * M1 + gap], 1ull);
      }
    }
  }
  if (use_lds) {
    __syncthreads();
    for (u32 i = threadIdx.x; i < 3 * (M + 1); i += 256) { const u32 v = s_hist[i]; if (v) atomicAdd(&loc[i], (u64)v); }
  }
}

// one workgroup.  loc[3][M + 1] -> added into spec; cursor (null without SHARED) [M + 1]: the rows of this call with a smaller rec
__global__ __launch_bounds__(256)
void k_pan_fold(const u64* __restrict__ loc, u32 M, u64* __restrict__ spec, u32* __restrict__ cursor)
{
  __shared__ u32 s[256];
  const u32 tid = threadIdx.x;
  const u64 M1 = (u64)M + 1;
  for (u64 i = tid; i < 3 * M1; i += 256) { const u64 v = loc[i]; if (v) atomicAdd(&spec[i], v); }
  if (!cursor) return;
  u32 carry = 0;
  for (u64 t0 = 0; t0 < M1; t0 += 256) {
    const u64 i = t0 + tid;
    const u32 v = i < M1 ? (u32)loc[i] : 0u;      // (a call has fewer than 2^32 rows)
    s[tid] = v;
    __syncthreads();
    for (u32 off = 1; off < 256; off <<= 1) {
      const u32 t = tid >= off ? s[tid - off] : 0u;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    if (i < M1) cursor[i] = carry + s[tid] - v;
    carry += s[255];
    __syncthreads();
  }
}

// a thread a row; cursor[r]: the next free place of class r (k_pan_fold's scan, moved on here)
__global__ __launch_bounds__(256)
void k_pan_order(const u32* __restrict__ recv, u32 n_rows, u32 M, u32* __restrict__ cursor, uint2* __restrict__ order)
{
  const u32 lane = threadIdx.x & 63u;
  const u64 n_tiles = ((u64)n_rows + 255) / 256;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 row = t * 256 + threadIdx.x;
    const bool have = row < n_rows;
    u32 r = have ? recv[row] : 0u;
    if (r > M) r = M;      // (never: a recurrence is at most M; the cursor has M + 1 entries)
    u64 todo = __ballot(have);
    while (todo) {      // (uniform over the wave)
      const int lead = __ffsll((long long)todo) - 1;
      const u32 rl = (u32)__shfl((int)r, lead);
      const bool in = have && r == rl;
      const u64 same = __ballot(in);
      u32 base = 0;
      if ((int)lane == lead) base = atomicAdd(&cursor[rl], (u32)__popcll(same));
      base = (u32)__shfl((int)base, lead);
      if (in) {
        const u64 at = (u64)base + (u32)__popcll(same & ((1ULL << lane) - 1ULL));
        if (at < n_rows) order[at] = make_uint2((u32)row, r);
      }
      todo &= ~same;
    }
  }
}

// work item w: run w / n_blocks of the order, unit block w % n_blocks.  ordt as for k_pan_score.
template <bool COUNT>
__global__ __launch_bounds__(PN_BLOCK)
void k_pan_shared(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 M, const u32* __restrict__ ordt, u32 a,
                  const uint2* __restrict__ order, u32 n_blocks, u64* __restrict__ shared)
{
  __shared__ uint2 s_ord[PN_RUN];
  const u32 tid = threadIdx.x;
  const u32 units = COUNT ? N : (u32)(((u64)N + 7) / 8);
  const u64 n_runs = ((u64)n_rows + PN_RUN - 1) / PN_RUN, n_work = n_runs * n_blocks;
  for (u64 w = blockIdx.x; w < n_work; w += gridDim.x) {
    const u64 run = w / n_blocks, p0 = run * PN_RUN;
    const u64 un = (w % n_blocks) * PN_BLOCK + tid;
    const u32 len = (u32)std::min<u64>(PN_RUN, n_rows - p0);
    __syncthreads();      // (the run before this one has been read by every lane)
    if (tid < len) {
      uint2 e = order[p0 + tid];
      if (e.x >= n_rows || e.y > M) e = make_uint2(0u, 0u);      // (never: the order is a permutation of the rows; a rec of 0 adds nothing)
      s_ord[tid] = e;
    }
    __syncthreads();
    // which of the lane's columns are listed: COUNT one, PA a mask of 8
    u32 m = 0;
    if (un < units) {
      if (COUNT) m = ordt[un] != PN_NONE;
      else for (u32 k = 0; k < 8; k++) m |= (u32)(ordt[8 * un + k] != PN_NONE) << k;
    }
    if (!m) continue;      // (the lane has no barrier left in this trip: the next trip's first barrier is met by all)
    const u8* q = rows + skip + (COUNT ? 4 * un : un);
    u32 cur = 0, acc[COUNT ? 1 : 8] = {};
    auto flush = [&]() {
      if (COUNT) { if (acc[0]) atomicAdd(&shared[(u64)cur * N + un], (u64)acc[0]); acc[0] = 0; }
      else {
#pragma unroll
        for (u32 k = 0; k < 8; k++) { if (acc[k]) atomicAdd(&shared[(u64)cur * N + 8 * un + k], (u64)acc[k]); acc[k] = 0; }
      }
    };
    for (u32 i = 0; i < len; i += 4) {
      uint2 e[4]; u32 v[4];
#pragma unroll
      for (u32 k = 0; k < 4; k++) {
        e[k] = i + k < len ? s_ord[i + k] : make_uint2(0u, 0u);
        v[k] = 0;
        if (e[k].y) {
          const u8* src = q + (u64)e[k].x * row_bytes;
          if (COUNT) v[k] = reinterpret_cast<const UDword*>(src)->v >= a; else v[k] = (u32)*src & m;
        }
      }
#pragma unroll
      for (u32 k = 0; k < 4; k++) {
        if (!e[k].y) continue;
        if (e[k].y != cur) { flush(); cur = e[k].y; }
        if (COUNT) acc[0] += v[k];
        else {
#pragma unroll
          for (u32 b = 0; b < 8; b++) acc[b] += (v[k] >> b) & 1u;
        }
      }
    }
    flush();
  }
}

static u32 pn_cus(const kmx_ctx* ctx) { return (u32)std::max(kmx_env_cus("KMX_PAN_CUS", ctx), 1); }
static u32 pn_grid(u64 dflt) { return kmx_env_grid("KMX_PAN_GRID", dflt); }

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
struct kmx_pan_result : MatResult {
  u32 n_use = 0;
  bool want_shared = false;
  u64 *d_spec = nullptr, *d_shared = nullptr;
};

static int pan_check(kmx_ctx* ctx, const kmx_pan_task* T, const char* who, u64* row_bytes)
{
  const MatCheck c{ctx, who};
  const u32 N = T->n_cols, M = T->n_use;
  int rc;
  if ((rc = c.n_cols(N, M, "list")) || (rc = c.no_bloom(T->mode, ": a Bloom row is a hash bit, its recurrence is not a k-mer's")) || (rc = c.mode(T->mode)) ||
      (rc = c.key_words(T->key_words)) || (rc = c.min_abund(T->min_abund, T->mode)) || (rc = c.flags(T->flags, KMX_PAN_SHARED))) return rc;
  if (T->shared && !(T->flags & KMX_PAN_SHARED)) return c.no(KMX_E_INVAL, ": a shared table without KMX_PAN_SHARED");
  if ((rc = c.list_fits(M, N, "listed")) || (rc = c.identity(T->cols, M, N, "n_use"))) return rc;
  *row_bytes = MatCheck::row_bytes(T->key_words, T->mode, N);
  if ((rc = c.row_fits(*row_bytes)) || (rc = c.n_rows(T->n_rows))) return rc;
  if ((T->flags & KMX_PAN_SHARED) && ((u64)M + 1) * N >= (1ull << 30)) return c.no(KMX_E_UNSUPPORTED, ": a shared table of 8 GiB and more");
  if ((rc = c.rows(T->n_rows, T->rows))) return rc;
  return c.col_list(T->cols, M, N);
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int pan_queue(kmx_ctx* ctx, const kmx_pan_task* T, kmx_pan_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, M = R->n_use = T->n_use, skip = 8 * T->key_words, n_rows = (u32)R->n_rows;
  const bool count = T->mode == KMX_MODE_COUNT, sh = R->want_shared = (T->flags & KMX_PAN_SHARED) != 0;
  const u32 units = count ? N : (u32)(((u64)N + 7) / 8);
  const u64 M1 = (u64)M + 1, n_ord = ((u64)N + 7) / 8 * 8, spec_bytes = 24 * M1, shared_bytes = 8 * M1 * N;
  u32* h_ordt = (u32*)R->pin(4 * n_ord);      // page-locked: the ordinal table on its way up
  if (!h_ordt) return ctx->fail(KMX_E_NOMEM, "kmx_pan: host allocation failed");
  for (u64 i = 0; i < n_ord; i++) h_ordt[i] = !T->cols && i < N ? (u32)i : PN_NONE;
  if (T->cols) for (u32 j = 0; j < M; j++) h_ordt[T->cols[j]] = j;
  // a table of the call's own starts at zero; one the caller handed in is on neither list
  const bool own_spec = !T->spectrum, own_shared = sh && !T->shared;
  u32* d_ordt = (u32*)R->tmp(4 * n_ord);
  u64* d_loc = (u64*)R->tmp(spec_bytes);
  R->d_spec = own_spec ? (u64*)R->keep(spec_bytes) : (u64*)T->spectrum;
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_pan: device allocation failed");
  u32 *d_cursor = nullptr, *d_recv = nullptr; uint2* d_order = nullptr;
  if (sh) {
    R->d_shared = own_shared ? (u64*)R->keep(shared_bytes) : (u64*)T->shared;
    d_cursor = (u32*)R->tmp(4 * M1);
    if (n_rows) { d_recv = (u32*)R->tmp(4ull * n_rows); d_order = (uint2*)R->tmp(8ull * n_rows); }
    if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_pan: device allocation failed (send the body in runs of rows)");
  }
  KMX_HIP(ctx, hipMemcpyAsync(d_ordt, h_ordt, 4 * n_ord, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R, 4);      // ev: start, behind score + fold, behind the order, end
  if (rc != KMX_OK) return rc;
  if (own_spec) KMX_HIP(ctx, hipMemsetAsync(R->d_spec, 0, spec_bytes, st));
  if (own_shared) KMX_HIP(ctx, hipMemsetAsync(R->d_shared, 0, shared_bytes, st));
  const u32 cus = pn_cus(ctx);
  if (n_rows) {
    KMX_HIP(ctx, hipMemsetAsync(d_loc, 0, spec_bytes, st));
    // rows of 64 units and more get a wave each; their chunks shrink until the chip has PN_WAVES_PER_SIMD waves a SIMD to hide the loads
    const RowPlan p = mat_row_plan(units, n_rows, cus, PN_WAVES_PER_SIMD);
    const u32 grid = (u32)std::min<u64>((p.chunks + 3) / 4, pn_grid(std::min<u64>((u64)cus * PN_WGS_PER_CU, PN_MAX_GRID)));
    const u32 use_lds = 3 * M1 <= PN_LDS_WORDS;
    const size_t lds = use_lds ? (size_t)(12 * M1) : 0;
    if (count) hipLaunchKernelGGL(k_pan_score<true>, dim3(grid), dim3(256), lds, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, p.L, p.RW,
                                  (const u32*)d_ordt, T->min_abund, use_lds, d_loc, d_recv);
    else hipLaunchKernelGGL(k_pan_score<false>, dim3(grid), dim3(256), lds, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, p.L, p.RW,
                            (const u32*)d_ordt, T->min_abund, use_lds, d_loc, d_recv);
    KMX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pan_fold, dim3(1), dim3(256), 0, st, (const u64*)d_loc, M, R->d_spec, sh ? d_cursor : (u32*)nullptr);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[1], st));
  if (n_rows && sh) {
    const u64 tiles = ((u64)n_rows + 255) / 256;
    hipLaunchKernelGGL(k_pan_order, dim3((u32)std::min<u64>(tiles, pn_grid(PN_MAX_GRID))), dim3(256), 0, st, (const u32*)d_recv, n_rows, M, d_cursor, d_order);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[2], st));
  if (n_rows && sh) {
    const u32 n_blocks = (units + PN_BLOCK - 1) / PN_BLOCK;
    const u64 work = (((u64)n_rows + PN_RUN - 1) / PN_RUN) * n_blocks;
    const u32 grid = (u32)std::min<u64>(work, pn_grid(PN_MAX_GRID));
    if (count) hipLaunchKernelGGL(k_pan_shared<true>, dim3(grid), dim3(PN_BLOCK), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, (const u32*)d_ordt,
                                  T->min_abund, (const uint2*)d_order, n_blocks, R->d_shared);
    else hipLaunchKernelGGL(k_pan_shared<false>, dim3(grid), dim3(PN_BLOCK), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, (const u32*)d_ordt,
                            T->min_abund, (const uint2*)d_order, n_blocks, R->d_shared);
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R);
}

extern "C" int kmx_pan_dev(kmx_ctx* ctx, const kmx_pan_task* task, kmx_pan_result** out)
{ return mat_call(ctx, task, out, false, "kmx_pan_dev", "kmx_pan", pan_check, pan_queue); }
extern "C" int kmx_pan_host(kmx_ctx* ctx, const kmx_pan_task* task, kmx_pan_result** out)
{ return mat_call(ctx, task, out, true, "kmx_pan_host", "kmx_pan", pan_check, pan_queue); }

extern "C" int kmx_pan_result_wait(kmx_pan_result* R) { return mat_wait(R); }
extern "C" uint64_t* kmx_pan_result_spectrum_dev(kmx_pan_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_spec : nullptr; }
extern "C" uint64_t* kmx_pan_result_shared_dev(kmx_pan_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_shared : nullptr; }
extern "C" int kmx_pan_result_copy_spectrum(kmx_pan_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_spec, 3 * ((u64)R->n_use + 1), 8) : KMX_E_INVAL; }
extern "C" int kmx_pan_result_copy_shared(kmx_pan_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_shared, ((u64)R->n_use + 1) * R->n_cols, 8, "kmx_pan_result_copy_shared: the call was made without KMX_PAN_SHARED") : KMX_E_INVAL; }
extern "C" double kmx_pan_result_kernel_ms(kmx_pan_result* R) { return mat_kernel_ms(R); }
extern "C" int kmx_pan_result_kernel_parts_ms(kmx_pan_result* R, double* score_ms, double* order_ms, double* shared_ms)
{ return mat_kernel_parts_ms(R, {score_ms, order_ms, shared_ms}, R && R->want_shared ? 7u : 1u); }
extern "C" uint64_t kmx_pan_result_algo_bytes(kmx_pan_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  const u64 M1 = (u64)R->n_use + 1, body = R->n_rows * R->row_bytes;
  return body + 24 * M1 + (R->want_shared ? body + 24ull * R->n_rows + 8 * M1 * R->n_cols : 0);
}
extern "C" void kmx_pan_result_free(kmx_pan_result* R) { mat_free(R); }
