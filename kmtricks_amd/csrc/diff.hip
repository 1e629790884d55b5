// diff.hip -- `kmx diff` on the device: which rows of a matrix are over- or under-represented in the case samples against the control
// samples (include/kmx.h, section "diff"; what kmdiff asks of a kmtricks matrix).  No reference counterpart in the kmtricks tree.
// gfx950, wave64.
//
//   k_colsums      the per-sample totals: a workgroup takes a tile of rows and LU units of a row (COUNT: a lane a column, a wave's load
//                  is 256 contiguous bytes a row, a u64 accumulator; PA: a lane a byte with eight accumulators, the last byte masked to
//                  the columns below N when it is loaded); rows shorter than the workgroup are taken 256 / LU at a time and meet in
//                  LDS; one 64-bit atomic add per column per workgroup.
//   k_diff_score   a wave a chunk of rows.  A row of 64 units and more (a unit: a count, or a payload byte) is read by the whole wave,
//                  shorter rows by the L lanes of a sub-group (L = the power of two at or above the units), 64 / L rows at a time.
//                  The masked sums and recurrences of a row are a butterfly over its lanes; lane i of the wave keeps the numbers of
//                  the chunk's row i, so that at the end every lane computes `over` and `stat` of one row and writes its keep word
//                  and, for a kept row, its record.  The kept rows of a tile of 256 are counted with one atomic add a wave.
//   k_diff_place   the records of the kept rows, gathered to their final place (rank in the tile + the tile's base).
// The tile bases are k_filter_scan's and the kept rows are moved by k_filter_move (filter.hip), both unchanged: orb == irb, the keep
// words in the place of the hits, no new column.
// Every load of a body byte is inside [rows, rows + n_rows * row_bytes) by construction: an address is rows + r * row_bytes + skip + b
// with r < n_rows and b + (bytes loaded) <= row_bytes - skip, both tested by the lane that loads; nothing is loaded in wider pieces
// than the piece that is tested (a byte for PA, a count's dword for COUNT) and nothing is rounded to an aligned address.
#include "matrix_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace kmx {

constexpr u32 DF_TILE = 256;              // rows of a placement tile: k_filter_move's (filter_tiles)
constexpr u32 DF_MAX_GRID = 1u << 18;     // workgroups of a launch: the kernels stride over their work
constexpr u32 DF_WAVES_PER_SIMD = 8;      // chunks of long rows are made small enough for this many waves a SIMD
constexpr u32 CS_WGS_PER_CU = 8;          // workgroups k_colsums aims at


struct DiffRec { u64 sum_ctrl, sum_case; double stat; u32 rec_ctrl, rec_case, row, over; };      // kmx_diff_rec
static_assert(sizeof(DiffRec) == 40 && sizeof(kmx_diff_rec) == 40, "a record is 40 bytes");

template <bool COUNT>
__global__ __launch_bounds__(256)
void k_colsums(const u8* __restrict__ rows, u64 n_rows, u64 row_bytes, u32 skip, u32 N, u32 LU, u64 tile_rows, u64* __restrict__ sums)
{
  constexpr u32 PER = COUNT ? 1 : 8;      // columns of a unit
  __shared__ u64 s_acc[256 * PER];
  const u32 tid = threadIdx.x, u = tid & (LU - 1u), sub = tid / LU, RP = 256u / LU;
  const u32 units = COUNT ? N : (N + 7) / 8;
  const u32 unit = blockIdx.x * LU + u;      // (blockIdx.x * LU < units <= 2^32 - 1)
  for (u32 i = tid; i < LU * PER; i += 256) s_acc[i] = 0;
  __syncthreads();
  const u64 r0 = (u64)blockIdx.y * tile_rows, r1 = min(n_rows, r0 + tile_rows);
  if (unit < units) {
    const u8* p = rows + skip + (COUNT ? 4ull * unit : (u64)unit);
    if (COUNT) {
      u64 acc = 0;
      for (u64 r = r0 + sub; r < r1; r += RP) acc += reinterpret_cast<const UDword*>(p + r * row_bytes)->v;
      if (acc) atomicAdd(&s_acc[u], acc);
    } else {
      const u32 keep = 8ull * unit + 8 <= N ? 0xFFu : (1u << (N - 8 * unit)) - 1u;      // the padding bits of the last byte
      u32 a[8];      // (a tile is shorter than 2^32 rows)
#pragma unroll
      for (int j = 0; j < 8; j++) a[j] = 0;
      for (u64 r = r0 + sub; r < r1; r += RP) {
        const u32 x = p[r * row_bytes] & keep;
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] += (x >> j) & 1u;
      }
#pragma unroll
      for (int j = 0; j < 8; j++) if (a[j]) atomicAdd(&s_acc[8 * u + j], (u64)a[j]);
    }
  }
  __syncthreads();
  for (u32 i = tid; i < LU * PER; i += 256) {
    const u64 col = (u64)blockIdx.x * LU * PER + i, v = s_acc[i];
    if (col < N && v) atomicAdd(&sums[col], v);
  }
}

// the Poisson likelihood-ratio statistic of include/kmx.h, in IEEE double in the order written there: no contraction into fma
__device__ __forceinline__ double diff_stat(u64 c0, u64 c1, u64 T0, u64 T1)
{
#pragma clang fp contract(off)
  const u64 c = c0 + c1;
  if (c == 0) return 0.0;
  const double dT = (double)(T0 + T1), dc = (double)c;
  double t1 = 0.0, t0 = 0.0;
  if (c1) t1 = (double)c1 * log(((double)c1 * dT) / (dc * (double)T1));
  if (c0) t0 = (double)c0 * log(((double)c0 * dT) / (dc * (double)T0));
  const double s = 2.0 * (t1 + t0);
  return s > 0.0 ? s : 0.0;
}

// 1: c1 * T0 > c0 * T1, 2: below, 0: equal -- in 128-bit integers
__device__ __forceinline__ u32 diff_over(u64 c0, u64 c1, u64 T0, u64 T1)
{
  const u64 ah = __umul64hi(c1, T0), al = c1 * T0, bh = __umul64hi(c0, T1), bl = c0 * T1;
  if (ah != bh) return ah > bh ? 1u : 2u;
  if (al != bl) return al > bl ? 1u : 2u;
  return 0u;
}

// grp: COUNT -- group[N]; PA -- the control byte masks [nb], then the case byte masks [nb] (padding bits 0 in both).
// L: lanes of a row (a power of two <= 64); RW: rows of a wave's chunk (64 when L < 64; a power of two <= 64 when L == 64).
template <bool COUNT>
__global__ __launch_bounds__(256)
void k_diff_score(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 L, u32 RW, const u8* __restrict__ grp,
                  u64 T0, u64 T1, double thr, u32 min_rec, u32* __restrict__ keep, DiffRec* __restrict__ recs, u32* __restrict__ tile_cnt)
{
  const u32 lane = threadIdx.x & 63u, u = lane & (L - 1u), sub = lane / L;
  const u32 units = COUNT ? N : (N + 7) / 8;
  const u32 passes = L == 64 ? RW : L;
  const u64 n_chunks = ((u64)n_rows + RW - 1) / RW;
  // what the lane's first units belong to, read once: COUNT 2 bits a unit for 16 units, PA the two masks of one byte
  u32 gp = 0;
  if (COUNT) {
    for (u32 i = 0; i < 16; i++) { const u64 un = (u64)u + (u64)L * i; if (un < units) gp |= (u32)grp[un] << (2 * i); }
  } else if (u < units) gp = (u32)grp[u] | ((u32)grp[(u64)units + u] << 8);
  for (u64 g = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; g < n_chunks; g += (u64)gridDim.x * 4) {
    const u64 row0 = g * RW;
    u64 c0 = 0, c1 = 0, rr = 0;      // rr: the recurrences, control in the low and case in the high half
    for (u32 p = 0; p < passes; p++) {
      const u64 row = row0 + (u64)sub * L + p;
      u64 a0 = 0, a1 = 0, ar = 0;
      if (row < n_rows) {
        const u8* q = rows + row * row_bytes + skip;
        u32 i = 0;
        for (u64 un = u; un < units; un += L, i++) {
          if (COUNT) {
            const u32 v = reinterpret_cast<const UDword*>(q + 4 * un)->v;
            const u32 gr = i < 16 ? (gp >> (2 * i)) & 3u : (u32)grp[un];
            const u64 nz = v != 0;
            if (gr == 0) { a0 += v; ar += nz; }
            else if (gr == 1) { a1 += v; ar += nz << 32; }
          } else {
            const u32 x = q[un];
            const u32 m = i == 0 ? gp : (u32)grp[un] | ((u32)grp[(u64)units + un] << 8);
            const u64 b0 = (u32)__popc(x & m & 0xFFu), b1 = (u32)__popc(x & (m >> 8));
            a0 += b0; a1 += b1; ar += b0 | (b1 << 32);
          }
        }
      }
      for (u32 o = L >> 1; o; o >>= 1) {
        a0 += __shfl_xor(a0, (int)o); a1 += __shfl_xor(a1, (int)o); ar += __shfl_xor(ar, (int)o);
      }
      if (u == p) { c0 = a0; c1 = a1; rr = ar; }
    }
    // lane i holds row row0 + i
    const u64 mine = row0 + lane;
    const bool have = lane < RW && mine < n_rows;
    bool kept = false;
    if (have) {
      const u32 q0 = (u32)rr, q1 = (u32)(rr >> 32);
      const double stat = diff_stat(c0, c1, T0, T1);
      kept = q0 + q1 >= min_rec && stat >= thr;      // (q0 + q1 <= N < 2^30)
      keep[mine] = kept ? 1u : 0u;
      if (kept) {
        DiffRec rec;
        rec.sum_ctrl = c0; rec.sum_case = c1; rec.stat = stat; rec.rec_ctrl = q0; rec.rec_case = q1; rec.row = (u32)mine;
        rec.over = diff_over(c0, c1, T0, T1);
        recs[mine] = rec;
      }
    }
    const u32 nk = (u32)__popcll(__ballot(kept));
    if (lane == 0 && nk) atomicAdd(&tile_cnt[row0 / DF_TILE], nk);      // (a chunk lies in one tile: RW divides DF_TILE)
  }
}

__global__ __launch_bounds__(DF_TILE)
void k_diff_place(const u32* __restrict__ keep, const DiffRec* __restrict__ recs, u32 n_rows, const u32* __restrict__ tile_base,
                  DiffRec* __restrict__ out)
{
  __shared__ u32 s_w[DF_TILE / 64];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 n_tiles = (u32)(((u64)n_rows + DF_TILE - 1) / DF_TILE);
  for (u32 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 row = (u64)t * DF_TILE + tid;
    const bool k = row < n_rows && keep[row] != 0;
    const u64 bal = __ballot(k);
    if (lane == 0) s_w[wave] = (u32)__popcll(bal);
    __syncthreads();
    u32 rank = (u32)__popcll(bal & ((1ULL << lane) - 1ULL));
    for (u32 w = 0; w < wave; w++) rank += s_w[w];
    if (k) out[(u64)tile_base[t] + rank] = recs[row];
    __syncthreads();
  }
}

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
static int diff_check_body(const MatCheck& c, u32 key_words, u32 mode, u32 n_cols, const void* rows, u64 n_rows, u64* row_bytes)
{
  int rc;
  if ((rc = c.n_cols(n_cols)) || (rc = c.no_bloom(mode, "")) || (rc = c.mode(mode)) || (rc = c.key_words(key_words))) return rc;
  *row_bytes = MatCheck::row_bytes(key_words, mode, n_cols);
  if ((rc = c.row_fits(*row_bytes)) || (rc = c.n_rows(n_rows))) return rc;
  return c.rows(n_rows, rows);
}

// ---- column sums ----
struct kmx_colsums_result : MatResult {
  u64* d_sums = nullptr;
};

static int colsums_check(kmx_ctx* ctx, const kmx_colsums_task* T, const char* who, u64* row_bytes)
{ return diff_check_body(MatCheck{ctx, who}, T->key_words, T->mode, T->n_cols, T->rows, T->n_rows, row_bytes); }

static int colsums_queue(kmx_ctx* ctx, const kmx_colsums_task* T, kmx_colsums_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, skip = 8 * T->key_words;
  const bool count = T->mode == KMX_MODE_COUNT;
  R->d_sums = (u64*)T->sums;
  const bool own = !R->d_sums;
  if (own && !(R->d_sums = (u64*)R->keep(8ull * N))) return ctx->fail(KMX_E_NOMEM, "kmx_colsums: device allocation failed");
  int rc = mat_queue_head(R);
  if (rc != KMX_OK) return rc;
  if (own) KMX_HIP(ctx, hipMemsetAsync(R->d_sums, 0, 8ull * N, st));
  if (T->n_rows) {
    const u32 units = count ? N : (N + 7) / 8, LU = pow2_at_or_above(units, 256), ub = (units + LU - 1) / LU;
    u64 tiles = std::max<u64>(1, (u64)std::max(kmx_plan_cus(ctx), 1) * CS_WGS_PER_CU / ub);
    tiles = std::min<u64>(std::min<u64>(tiles, (T->n_rows + 63) / 64), 65535);
    const u64 tile_rows = (T->n_rows + tiles - 1) / tiles;
    tiles = (T->n_rows + tile_rows - 1) / tile_rows;
    const dim3 grid(ub, (u32)tiles);
    if (count) hipLaunchKernelGGL(k_colsums<true>, grid, dim3(256), 0, st, (const u8*)T->rows, (u64)T->n_rows, R->row_bytes, skip, N, LU, tile_rows, R->d_sums);
    else hipLaunchKernelGGL(k_colsums<false>, grid, dim3(256), 0, st, (const u8*)T->rows, (u64)T->n_rows, R->row_bytes, skip, N, LU, tile_rows, R->d_sums);
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R);
}

extern "C" int kmx_colsums_dev(kmx_ctx* ctx, const kmx_colsums_task* task, kmx_colsums_result** out)
{ return mat_call(ctx, task, out, false, "kmx_colsums_dev", "kmx_colsums", colsums_check, colsums_queue); }
extern "C" int kmx_colsums_host(kmx_ctx* ctx, const kmx_colsums_task* task, kmx_colsums_result** out)
{ return mat_call(ctx, task, out, true, "kmx_colsums_host", "kmx_colsums", colsums_check, colsums_queue); }

extern "C" int kmx_colsums_result_wait(kmx_colsums_result* R) { return mat_wait(R); }
extern "C" uint64_t* kmx_colsums_result_sums_dev(kmx_colsums_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_sums : nullptr; }
extern "C" int kmx_colsums_result_copy_sums(kmx_colsums_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_sums, R->n_cols, 8) : KMX_E_INVAL; }
extern "C" double kmx_colsums_result_kernel_ms(kmx_colsums_result* R) { return mat_kernel_ms(R); }
extern "C" uint64_t kmx_colsums_result_algo_bytes(kmx_colsums_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  return R->n_rows * R->row_bytes + 8ull * R->n_cols;
}
extern "C" void kmx_colsums_result_free(kmx_colsums_result* R) { mat_free(R); }

// ---- the test ----
struct kmx_diff_result : MatResult {
  DiffRec* d_recs = nullptr;
  u8* d_out = nullptr;
};

static int diff_check(kmx_ctx* ctx, const kmx_diff_task* T, const char* who, u64* row_bytes)
{
  const MatCheck c{ctx, who};
  const int rc = diff_check_body(c, T->key_words, T->mode, T->n_cols, T->rows, T->n_rows, row_bytes);
  if (rc != KMX_OK) return rc;
  if (!T->group) return c.no(KMX_E_INVAL, ": null group table");
  u64 n[3] = {0, 0, 0};
  for (u32 i = 0; i < T->n_cols; i++) {
    if (T->group[i] > 2) return c.no(KMX_E_INVAL, ": a group is 0 (control), 1 (case) or 2 (ignored)");
    n[T->group[i]]++;
  }
  if (!n[0] || !n[1]) return c.no(KMX_E_INVAL, ": at least one control and one case column are needed");
  if (T->total_ctrl == 0 || T->total_case == 0) return c.no(KMX_E_INVAL, ": total_ctrl and total_case must be above 0");
  if (T->total_ctrl + T->total_case < T->total_ctrl) return c.no(KMX_E_INVAL, ": total_ctrl + total_case must be below 2^64");
  if (std::isnan(T->threshold) || T->threshold < 0.0) return c.no(KMX_E_INVAL, ": the threshold is a number at or above 0");
  return KMX_OK;
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int diff_queue(kmx_ctx* ctx, const kmx_diff_task* T, kmx_diff_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, skip = 8 * T->key_words, n_rows = (u32)R->n_rows, tiles = filter_tiles(n_rows);
  const bool count = T->mode == KMX_MODE_COUNT;
  const u32 units = count ? N : (N + 7) / 8;
  const u64 grp_bytes = count ? N : 2ull * units;
  u8* h_grp;      // page-locked: the group table (COUNT) or the two byte masks (PA) on their way up
  if (!(R->h_tot = (u32*)R->pin(64)) || !(h_grp = (u8*)R->pin(grp_bytes))) return ctx->fail(KMX_E_NOMEM, "kmx_diff: host allocation failed");
  R->h_tot[0] = 0;
  if (count) memcpy(h_grp, T->group, N);
  else {      // per-group byte masks: bit i & 7 of byte i >> 3; the padding bits stay 0
    memset(h_grp, 0, grp_bytes);
    for (u32 i = 0; i < N; i++) if (T->group[i] < 2) h_grp[(T->group[i] ? units : 0) + (i >> 3)] |= (u8)(1u << (i & 7));
  }
  u32* d_keep = (u32*)R->tmp(4ull * n_rows);
  u32* d_tiles = (u32*)R->keep(4ull * ((u64)tiles + 1));
  DiffRec* d_recs_all = (DiffRec*)R->tmp(sizeof(DiffRec) * (u64)n_rows);
  R->d_recs = (DiffRec*)R->keep(sizeof(DiffRec) * (u64)n_rows);      // every row kept
  R->d_out = (u8*)R->keep((u64)n_rows * R->row_bytes + 16);
  u8* d_grp = (u8*)R->tmp(grp_bytes);
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_diff: device allocation failed (send the body in runs of rows)");
  KMX_HIP(ctx, hipMemcpyAsync(d_grp, h_grp, grp_bytes, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_tiles, 0, 4ull * ((u64)tiles + 1), st));
  if (n_rows) {
    // rows of 64 units and more get a wave each; their chunks shrink until the chip has DF_WAVES_PER_SIMD waves a SIMD to hide the loads
    const RowPlan p = mat_row_plan(units, n_rows, (u32)std::max(kmx_plan_cus(ctx), 1), DF_WAVES_PER_SIMD);
    const u32 grid = (u32)std::min<u64>((p.chunks + 3) / 4, kmx_grid_cap(DF_MAX_GRID));
    if (count) hipLaunchKernelGGL(k_diff_score<true>, dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, p.L, p.RW, (const u8*)d_grp,
                                  (u64)T->total_ctrl, (u64)T->total_case, T->threshold, T->min_rec, d_keep, d_recs_all, d_tiles);
    else hipLaunchKernelGGL(k_diff_score<false>, dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, p.L, p.RW, (const u8*)d_grp,
                            (u64)T->total_ctrl, (u64)T->total_case, T->threshold, T->min_rec, d_keep, d_recs_all, d_tiles);
    KMX_HIP(ctx, hipGetLastError());
  }
  KMX_HIP(ctx, launch_filter_scan(d_tiles, tiles, st));
  if (n_rows) {
    KMX_HIP(ctx, launch_filter_move((const u8*)T->rows, n_rows, R->row_bytes, R->row_bytes, d_keep, d_keep, d_tiles, R->d_out, st));
    hipLaunchKernelGGL(k_diff_place, dim3(std::min(tiles, kmx_grid_cap(DF_MAX_GRID))), dim3(DF_TILE), 0, st, (const u32*)d_keep, (const DiffRec*)d_recs_all, n_rows,
                       (const u32*)d_tiles, R->d_recs);
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R, d_tiles + tiles);
}

extern "C" int kmx_diff_dev(kmx_ctx* ctx, const kmx_diff_task* task, kmx_diff_result** out)
{ return mat_call(ctx, task, out, false, "kmx_diff_dev", "kmx_diff", diff_check, diff_queue); }
extern "C" int kmx_diff_host(kmx_ctx* ctx, const kmx_diff_task* task, kmx_diff_result** out)
{ return mat_call(ctx, task, out, true, "kmx_diff_host", "kmx_diff", diff_check, diff_queue); }

extern "C" int kmx_diff_result_wait(kmx_diff_result* R) { return mat_wait(R); }
extern "C" uint64_t kmx_diff_result_rows(kmx_diff_result* R) { return mat_wait(R) == KMX_OK ? R->h_tot[0] : 0; }
extern "C" uint64_t kmx_diff_result_row_bytes(const kmx_diff_result* R) { return R ? R->row_bytes : 0; }
extern "C" uint64_t kmx_diff_result_body_bytes(kmx_diff_result* R) { return R ? kmx_diff_result_rows(R) * R->row_bytes : 0; }
extern "C" const void* kmx_diff_result_body_dev(kmx_diff_result* R) { return mat_wait(R) == KMX_OK ? R->d_out : nullptr; }
extern "C" const kmx_diff_rec* kmx_diff_result_recs_dev(kmx_diff_result* R) { return mat_wait(R) == KMX_OK ? (const kmx_diff_rec*)R->d_recs : nullptr; }
extern "C" int kmx_diff_result_copy_body(kmx_diff_result* R, void* host_dst, uint64_t dst_bytes)
{ return R ? mat_copy_out(R, host_dst, dst_bytes, R->d_out, kmx_diff_result_body_bytes(R), 1) : KMX_E_INVAL; }
extern "C" int kmx_diff_result_copy_recs(kmx_diff_result* R, kmx_diff_rec* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_recs, kmx_diff_result_rows(R), sizeof(DiffRec)) : KMX_E_INVAL; }
extern "C" double kmx_diff_result_kernel_ms(kmx_diff_result* R) { return mat_kernel_ms(R); }
extern "C" uint64_t kmx_diff_result_algo_bytes(kmx_diff_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  return R->n_rows * R->row_bytes + (u64)R->h_tot[0] * (R->row_bytes + sizeof(DiffRec));
}
extern "C" void kmx_diff_result_free(kmx_diff_result* R) { mat_free(R); }
