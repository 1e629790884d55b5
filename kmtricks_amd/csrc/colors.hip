// colors.hip -- `kmx colors` on the device: the distinct sample sets of a matrix's rows (include/kmx.h, section "colors"; the colour
// classes of a coloured de Bruijn graph, the exclusive regions of the N-way Venn diagram).  No reference counterpart in the kmtricks
// tree.  gfx950, wave64.
//
//   k_col_pack    a wave a chunk of rows, L lanes a row, a lane an ORDINAL of the list (not an input column: the pattern is wanted in
//                 list order, so the column comes from a table per ordinal, the identity included -- one road for COUNT and PA, listed
//                 or not).  The ballot of the lanes' presence bits IS the pattern word: lists of 64 ordinals and more give the wave a
//                 row and a word a trip; shorter lists give L lanes a row, 64 / L rows a ballot.  Writes pat[row][W] (lane k keeps
//                 word k of a block of 64 and the block leaves in one coalesced store) and sig[row], a 64-bit mix of the W words.
//   k_col_claim   a thread a row.  First the wave groups its rows: the first pending lane leads, the lanes whose signature AND words
//                 equal the leader's retire with it.  Then every leader probes the table (open addressing, linear, T a power of two
//                 >= 2 n_rows u32 slots of row indices, start sig & (T - 1)) for its group: atomicCAS(slot, EMPTY, row); EMPTY: the
//                 row owns the slot and is the class's representative; else the signature and then all W words of the row found are
//                 compared -- equal: that row is the representative; unequal: the next slot.  One atomicMin (the class's first row) and
//                 one atomicAdd (its size) a group, on arrays indexed by the REPRESENTATIVE row; rep[row] for every row.  At most T
//                 probes, then a status word is raised and the call returns KMX_E_INTERNAL.  Nothing waits: a CAS's answer is final.
//                 Everything compared (pat, sig) was written by the launch before, so there is no fence and no acquire.
//   k_col_flag    a row is its class's first when minrow[rep[row]] == row: the flags counted per tile of 256 rows;
//   (scan)        launch_filter_scan over the tiles' counts (the scan of filter / select / diff), the total C behind them;
//   k_col_number  the first rows' ranks inside their tile from a ballot: rank[row], first[c], size[c];
//   k_col_ids     ids[row] = rank[minrow[rep[row]]];  k_col_gather  patterns[c] = pat[first[c]], an element a lane.
// No kernel waits on another workgroup: any grid is a correct one.
// Every load of a body byte is inside [rows, rows + n_rows * row_bytes): an address is rows + r * row_bytes + skip + b with r < n_rows
// and b + (bytes loaded) <= row_bytes - skip, both tested by the lane that loads (c < N); nothing is rounded to an aligned address.
// Every row index taken from the table, rep, minrow or first is tested < n_rows before it becomes an address.  The launch knobs of
// this file are its own: KMX_COLORS_CUS, KMX_COLORS_GRID and KMX_COLORS_HASH_BITS.
#include "matrix_host.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 CL_EMPTY = 0xFFFFFFFFu;     // a free slot of the table; "no row" everywhere else (n_rows <= 2^32 - 256)
constexpr u32 CL_TILE = 256;              // rows of a tile: a thread a row
constexpr u32 CL_WGS_PER_CU = 8;          // k_col_pack's grid: workgroups a CU
constexpr u32 CL_MAX_GRID = 1u << 16;     // workgroups of a launch: the kernels stride over their work
constexpr u32 CL_WAVES_PER_SIMD = 8;      // chunks of long lists are made small enough for this many waves a SIMD
constexpr u32 CL_AHEAD = 4;              // k_col_pack: loads a lane has on their way before the ballots that need them
constexpr u64 CL_SEED = 0x9E3779B97F4A7C15ull;

static_assert(sizeof(kmx_colors_task) == 48, "kmx_colors_task is 48 bytes");

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 cl_mix(u64 h, u64 w) { h = (h ^ w) * 0xFF51AFD7ED558CCDull; return h ^ (h >> 32); }
__device__ __forceinline__ u64 cl_fin(u64 h) { h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; return h ^ (h >> 29); }
__device__ __forceinline__ u64 cl_shfl64(u64 v, int src)
{
  const u32 lo = (u32)__shfl((int)(u32)v, src), hi = (u32)__shfl((int)(u32)(v >> 32), src);
  return (u64)hi << 32 | lo;
}

// what a lane loads for column c < N: its count, or the payload byte that holds its bit; and whether that makes the column present
// (a value of 0 is "absent" in both modes: a >= 1)
template <bool COUNT> __device__ __forceinline__ u32 cl_unit(const u8* q, u32 c) { return COUNT ? reinterpret_cast<const UDword*>(q + 4ull * c)->v : (u32)q[c >> 3]; }
template <bool COUNT> __device__ __forceinline__ bool cl_present(u32 v, u32 c, u32 a) { return COUNT ? v >= a : (bool)((v >> (c & 7u)) & 1u); }

// colt: the input column of every ordinal, M entries.  L: lanes of a row (a power of two <= 64, >= M when below 64); RW: rows of a wave's
// chunk (64 when L < 64).  keep: the signature bits that stay; the others are SET (KMX_COLORS_HASH_BITS; all ones: nothing changes).
template <bool COUNT>
__global__ __launch_bounds__(256)
void k_col_pack(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 M, u32 L, u32 RW, const u32* __restrict__ colt,
                u32 a, u64 keep, u64* __restrict__ pat, u64* __restrict__ sig)
{
  const u32 lane = threadIdx.x & 63u, u = lane & (L - 1u), sub = lane / L;
  const u32 W = (u32)(((u64)M + 63) / 64);
  const u64 n_chunks = ((u64)n_rows + RW - 1) / RW;
  for (u64 g = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; g < n_chunks; g += (u64)gridDim.x * 4) {
    const u64 row0 = g * RW;
    if (L == 64) {      // the wave a row, a word a trip; CL_AHEAD trips' loads are on their way before the first ballot
      for (u32 p = 0; p < RW; p++) {
        const u64 row = row0 + p;
        if (row >= n_rows) break;      // (uniform over the wave)
        const u8* q = rows + row * row_bytes + skip;
        u64 h = CL_SEED, mine = 0;
        for (u32 w0 = 0; w0 < W; w0 += CL_AHEAD) {
          u32 c[CL_AHEAD], v[CL_AHEAD];
#pragma unroll
          for (u32 k = 0; k < CL_AHEAD; k++) { const u64 j = (u64)(w0 + k) * 64 + lane; c[k] = j < M ? colt[j] : N; }      // (N: no column)
#pragma unroll
          for (u32 k = 0; k < CL_AHEAD; k++) v[k] = c[k] < N ? cl_unit<COUNT>(q, c[k]) : 0u;
#pragma unroll
          for (u32 k = 0; k < CL_AHEAD; k++) {
            const u32 w = w0 + k;
            if (w < W) {      // (uniform)
              const u64 b = __ballot(cl_present<COUNT>(v[k], c[k], a));
              h = cl_mix(h, b);
              if (lane == (w & 63u)) mine = b;
              if ((w & 63u) == 63u || w + 1 == W) {      // a block of up to 64 words leaves
                if (lane <= (w & 63u)) pat[row * W + (w & ~63u) + lane] = mine;
              }
            }
          }
        }
        if (lane == 0) sig[row] = (cl_fin(h) & keep) | ~keep;
      }
    } else {            // M <= L < 64: one word a row, 64 / L rows a ballot; lane i ends with row i of the chunk
      u64 word = 0;
      const u32 c = u < M ? colt[u] : N;
      for (u32 p0 = 0; p0 < L; p0 += CL_AHEAD) {
        u32 v[CL_AHEAD];
#pragma unroll
        for (u32 k = 0; k < CL_AHEAD; k++) {
          const u64 row = row0 + (u64)sub * L + p0 + k;
          v[k] = p0 + k < L && row < n_rows && c < N ? cl_unit<COUNT>(rows + row * row_bytes + skip, c) : 0u;
        }
#pragma unroll
        for (u32 k = 0; k < CL_AHEAD; k++) {
          if (p0 + k < L) {      // (uniform)
            const u64 b = __ballot(cl_present<COUNT>(v[k], c, a));
            if (u == p0 + k) word = (b >> (sub * L)) & ((1ull << L) - 1ull);
          }
        }
      }
      const u64 mine = row0 + lane;
      if (mine < n_rows) { pat[mine] = word; sig[mine] = (cl_fin(cl_mix(CL_SEED, word)) & keep) | ~keep; }
    }
  }
}

// tmask: T - 1.  minrow (all ones) and cnt (zero) are indexed by the representative row; rep[row]: the row's representative, CL_EMPTY
// when the probe bound was reached (then *status is raised)
__global__ __launch_bounds__(CL_TILE)
void k_col_claim(const u64* __restrict__ pat, const u64* __restrict__ sig, u32 n_rows, u32 W, u32* __restrict__ table, u64 tmask,
                 u32* __restrict__ minrow, u32* __restrict__ cnt, u32* __restrict__ rep, u32* __restrict__ status)
{
  const u32 lane = threadIdx.x & 63u;
  const u64 n_tiles = ((u64)n_rows + CL_TILE - 1) / CL_TILE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 row = t * CL_TILE + threadIdx.x;
    const bool have = row < n_rows;
    const u64 s = have ? sig[row] : 0ull;
    const u64* mp = pat + (have ? row : 0ull) * W;
    // the wave's groups: lead_of the lane that claims for this one, n_in the lanes of a leader's group
    u32 lead_of = lane, n_in = 0;
    u64 todo = __ballot(have);
    while (todo) {      // (uniform over the wave; the leader retires every trip)
      const int lead = __ffsll((long long)todo) - 1;
      const u64 sl = cl_shfl64(s, lead);
      const u32 rl = (u32)__shfl((int)(u32)row, lead);      // (< n_rows: the leader has a row)
      bool in = ((todo >> lane) & 1ull) && s == sl;
      if (in && (int)lane != lead) {
        const u64* lp = pat + (u64)rl * W;
        for (u32 w = 0; w < W; w++) if (mp[w] != lp[w]) { in = false; break; }
      }
      const u64 same = __ballot(in);
      if (in) { lead_of = (u32)lead; n_in = (u32)__popcll(same); }
      todo &= ~same;
    }
    u32 owner = CL_EMPTY;
    if (have && lead_of == lane) {
      u64 slot = s & tmask;
      for (u64 probes = 0; probes <= tmask; probes++) {
        const u32 prev = atomicCAS(&table[slot], CL_EMPTY, (u32)row);
        if (prev == CL_EMPTY) { owner = (u32)row; break; }
        if (prev < n_rows && sig[prev] == s) {
          const u64* op = pat + (u64)prev * W;
          bool eq = true;
          for (u32 w = 0; w < W; w++) if (op[w] != mp[w]) { eq = false; break; }
          if (eq) { owner = prev; break; }
        }
        slot = (slot + 1) & tmask;
      }
      if (owner == CL_EMPTY) atomicOr(status, 1u);
      else { atomicMin(&minrow[owner], (u32)row); atomicAdd(&cnt[owner], n_in); }      // (the leader is its group's lowest row)
    }
    owner = (u32)__shfl((int)owner, (int)lead_of);
    if (have) rep[row] = owner;
  }
}

__global__ __launch_bounds__(CL_TILE)
void k_col_flag(const u32* __restrict__ rep, const u32* __restrict__ minrow, u32 n_rows, u32* __restrict__ tile_cnt)
{
  const u64 n_tiles = ((u64)n_rows + CL_TILE - 1) / CL_TILE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 row = t * CL_TILE + threadIdx.x;
    const u32 o = row < n_rows ? rep[row] : CL_EMPTY;
    const int c = __syncthreads_count(o < n_rows && minrow[o] == (u32)row);
    if (threadIdx.x == 0) tile_cnt[t] = (u32)c;
  }
}

// tile_base: the scanned counts.  A first row's class is its rank among the first rows: class c's first row comes before class c + 1's
__global__ __launch_bounds__(CL_TILE)
void k_col_number(const u32* __restrict__ rep, const u32* __restrict__ minrow, const u32* __restrict__ cnt, u32 n_rows,
                  const u32* __restrict__ tile_base, u32* __restrict__ rank, u32* __restrict__ first, u32* __restrict__ size)
{
  __shared__ u32 s_w[CL_TILE / 64];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u64 n_tiles = ((u64)n_rows + CL_TILE - 1) / CL_TILE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 row = t * CL_TILE + threadIdx.x;
    const u32 o = row < n_rows ? rep[row] : CL_EMPTY;
    const bool flag = o < n_rows && minrow[o] == (u32)row;
    const u64 bal = __ballot(flag);
    if (lane == 0) s_w[wave] = (u32)__popcll(bal);
    __syncthreads();
    u32 r = (u32)__popcll(bal & ((1ULL << lane) - 1ULL));
    for (u32 w = 0; w < wave; w++) r += s_w[w];
    if (flag) {
      const u64 c = (u64)tile_base[t] + r;
      if (c < n_rows) { rank[row] = (u32)c; first[c] = (u32)row; size[c] = cnt[o]; }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(CL_TILE)
void k_col_ids(const u32* __restrict__ rep, const u32* __restrict__ minrow, const u32* __restrict__ rank, u32 n_rows, u32* __restrict__ ids)
{
  for (u64 row = (u64)blockIdx.x * CL_TILE + threadIdx.x; row < n_rows; row += (u64)gridDim.x * CL_TILE) {
    const u32 o = rep[row];
    const u32 m = o < n_rows ? minrow[o] : CL_EMPTY;
    ids[row] = m < n_rows ? rank[m] : CL_EMPTY;
  }
}

// n_classes: the scan's total, on the device
__global__ __launch_bounds__(CL_TILE)
void k_col_gather(const u64* __restrict__ pat, const u32* __restrict__ first, const u32* __restrict__ n_classes, u32 n_rows, u32 W,
                  u64* __restrict__ patterns)
{
  const u64 total = (u64)min(*n_classes, n_rows) * W;
  for (u64 i = (u64)blockIdx.x * CL_TILE + threadIdx.x; i < total; i += (u64)gridDim.x * CL_TILE) {
    const u32 f = first[i / W];
    if (f < n_rows) patterns[i] = pat[(u64)f * W + i % W];
  }
}
// ---- end of the kernels -------------------------------------------------------------------------------------------------------------

static u32 cl_cus(const kmx_ctx* ctx) { return (u32)std::max(kmx_env_cus("KMX_COLORS_CUS", ctx), 1); }
static u32 cl_grid(u64 dflt) { return kmx_env_grid("KMX_COLORS_GRID", dflt); }
// KMX_COLORS_HASH_BITS=b, 0 <= b <= 63: the low b bits of every signature stay, all the others are set
static u64 cl_keep()
{
  const long b = kmx_env_int("KMX_COLORS_HASH_BITS");
  return b >= 0 && b <= 63 ? (1ull << b) - 1ull : ~0ull;
}
static u64 cl_table_slots(u64 n_rows) { u64 t = 2; while (t < 2 * n_rows) t <<= 1; return t; }
static u64 cl_tiles(u64 n_rows) { return (n_rows + CL_TILE - 1) / CL_TILE; }
// what a call takes from the pool: scratch (given back when the call has run) and what the result keeps
static u64 cl_scratch_bytes(u64 n_rows, u64 M)
{
  const u64 W = (M + 63) / 64;
  return n_rows * (8 * W + 8 + 16) + 4 * cl_table_slots(n_rows) + 4 * (cl_tiles(n_rows) + 1) + 4 * M + 8;
}
static u64 cl_result_bytes(u64 n_rows, u64 M) { return n_rows * (12 + 8 * ((M + 63) / 64)); }

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
struct kmx_colors_result : MatResult {      // h_tot: C and the status word on their way down
  u32 n_use = 0, W = 0;
  u64* d_patterns = nullptr;
  u32 *d_ids = nullptr, *d_first = nullptr, *d_size = nullptr;
};

static int colors_check(kmx_ctx* ctx, const kmx_colors_task* T, const char* who, u64* row_bytes)
{
  const MatCheck c{ctx, who};
  const u32 N = T->n_cols, M = T->n_use;
  int rc;
  if ((rc = c.n_cols(N, M, "list")) || (rc = c.no_bloom(T->mode, ": a Bloom row is a hash bit, its sample set is not a k-mer's")) || (rc = c.mode(T->mode)) ||
      (rc = c.key_words(T->key_words)) || (rc = c.min_abund(T->min_abund, T->mode)) || (rc = c.flags(T->flags, 0)) || (rc = c.list_fits(M, N, "listed")) ||
      (rc = c.identity(T->cols, M, N, "n_use"))) return rc;
  *row_bytes = MatCheck::row_bytes(T->key_words, T->mode, N);
  if ((rc = c.row_fits(*row_bytes)) || (rc = c.n_rows(T->n_rows)) || (rc = c.col_list(T->cols, M, N))) return rc;
  // the pool cannot give more than the device has
  size_t fr = 0, tot = 0;
  if (hipSetDevice(ctx->device) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) return c.no(KMX_E_HIP, ": the device's memory size is not known");
  if (cl_scratch_bytes(T->n_rows, M) + cl_result_bytes(T->n_rows, M) > (u64)tot)
    return c.no(KMX_E_UNSUPPORTED, ": scratch and result beyond the device's memory (send the body in runs of rows)");
  return c.rows(T->n_rows, T->rows);
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int colors_queue(kmx_ctx* ctx, const kmx_colors_task* T, kmx_colors_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, M = R->n_use = T->n_use, skip = 8 * T->key_words, n_rows = (u32)R->n_rows, W = R->W = (u32)(((u64)M + 63) / 64);
  const bool count = T->mode == KMX_MODE_COUNT;
  const u64 n = n_rows, slots = cl_table_slots(n), tiles = cl_tiles(n);
  u32* h_colt;      // page-locked: the column table on its way up
  if (!(h_colt = (u32*)R->pin(4ull * M)) || !(R->h_tot = (u32*)R->pin(8))) return ctx->fail(KMX_E_NOMEM, "kmx_colors: host allocation failed");
  for (u32 j = 0; j < M; j++) h_colt[j] = T->cols ? T->cols[j] : j;
  R->h_tot[0] = 0; R->h_tot[1] = 0;
  u32* d_colt = (u32*)R->tmp(4ull * M);
  u32* d_tiles = (u32*)R->tmp(4 * (tiles + 1));
  u32* d_status = (u32*)R->tmp(4);
  u64 *d_pat = nullptr, *d_sig = nullptr;
  u32 *d_table = nullptr, *d_minrow = nullptr, *d_cnt = nullptr, *d_rep = nullptr, *d_rank = nullptr;
  if (n_rows) {
    d_pat = (u64*)R->tmp(8 * n * W); d_sig = (u64*)R->tmp(8 * n); d_table = (u32*)R->tmp(4 * slots);
    d_minrow = (u32*)R->tmp(4 * n); d_cnt = (u32*)R->tmp(4 * n); d_rep = (u32*)R->tmp(4 * n); d_rank = (u32*)R->tmp(4 * n);
    R->d_ids = (u32*)R->keep(4 * n); R->d_first = (u32*)R->keep(4 * n); R->d_size = (u32*)R->keep(4 * n); R->d_patterns = (u64*)R->keep(8 * n * W);
  }
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_colors: device allocation failed (send the body in runs of rows)");
  KMX_HIP(ctx, hipMemcpyAsync(d_colt, h_colt, 4ull * M, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R, 4);      // ev: start, behind the pack, behind the claim, end
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_tiles, 0, 4 * (tiles + 1), st));
  KMX_HIP(ctx, hipMemsetAsync(d_status, 0, 4, st));
  const u32 cus = cl_cus(ctx);
  const u32 tile_grid = (u32)std::min<u64>(std::max<u64>(tiles, 1), cl_grid(CL_MAX_GRID));
  if (n_rows) {
    // lists of 64 ordinals and more get a wave a row; their chunks shrink until the chip has CL_WAVES_PER_SIMD waves a SIMD to hide the loads
    const RowPlan p = mat_row_plan(M, n, cus, CL_WAVES_PER_SIMD);
    const u32 grid = (u32)std::min<u64>((p.chunks + 3) / 4, cl_grid(std::min<u64>((u64)cus * CL_WGS_PER_CU, CL_MAX_GRID)));
    const u64 keep = cl_keep();
    if (count) hipLaunchKernelGGL(k_col_pack<true>, dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, p.L, p.RW,
                                  (const u32*)d_colt, T->min_abund, keep, d_pat, d_sig);
    else hipLaunchKernelGGL(k_col_pack<false>, dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, p.L, p.RW,
                            (const u32*)d_colt, T->min_abund, keep, d_pat, d_sig);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[1], st));
  if (n_rows) {
    KMX_HIP(ctx, hipMemsetAsync(d_table, 0xFF, 4 * slots, st));
    KMX_HIP(ctx, hipMemsetAsync(d_minrow, 0xFF, 4 * n, st));
    KMX_HIP(ctx, hipMemsetAsync(d_cnt, 0, 4 * n, st));
    hipLaunchKernelGGL(k_col_claim, dim3(tile_grid), dim3(CL_TILE), 0, st, (const u64*)d_pat, (const u64*)d_sig, n_rows, W, d_table, slots - 1,
                       d_minrow, d_cnt, d_rep, d_status);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[2], st));
  if (n_rows) {
    hipLaunchKernelGGL(k_col_flag, dim3(tile_grid), dim3(CL_TILE), 0, st, (const u32*)d_rep, (const u32*)d_minrow, n_rows, d_tiles);
    KMX_HIP(ctx, hipGetLastError());
    KMX_HIP(ctx, launch_filter_scan(d_tiles, (u32)tiles, st));
    hipLaunchKernelGGL(k_col_number, dim3(tile_grid), dim3(CL_TILE), 0, st, (const u32*)d_rep, (const u32*)d_minrow, (const u32*)d_cnt, n_rows,
                       (const u32*)d_tiles, d_rank, R->d_first, R->d_size);
    KMX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_col_ids, dim3(tile_grid), dim3(CL_TILE), 0, st, (const u32*)d_rep, (const u32*)d_minrow, (const u32*)d_rank, n_rows, R->d_ids);
    KMX_HIP(ctx, hipGetLastError());
    const u32 ggrid = (u32)std::min<u64>(std::max<u64>((n * W + CL_TILE - 1) / CL_TILE, 1), cl_grid(CL_MAX_GRID));
    hipLaunchKernelGGL(k_col_gather, dim3(ggrid), dim3(CL_TILE), 0, st, (const u64*)d_pat, (const u32*)R->d_first, (const u32*)(d_tiles + tiles), n_rows, W,
                       R->d_patterns);
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R, d_tiles + tiles, d_status);
}

extern "C" int kmx_colors_dev(kmx_ctx* ctx, const kmx_colors_task* task, kmx_colors_result** out)
{ return mat_call(ctx, task, out, false, "kmx_colors_dev", "kmx_colors", colors_check, colors_queue); }
extern "C" int kmx_colors_host(kmx_ctx* ctx, const kmx_colors_task* task, kmx_colors_result** out)
{ return mat_call(ctx, task, out, true, "kmx_colors_host", "kmx_colors", colors_check, colors_queue); }

extern "C" int kmx_colors_result_wait(kmx_colors_result* R)
{
  if (!R || R->waited) return mat_wait(R);
  const int rc = mat_wait(R);
  if (rc != KMX_OK) return rc;
  if (R->h_tot[1] || R->h_tot[0] > R->n_rows)
    return R->status = R->ctx->fail(KMX_E_INTERNAL, "kmx_colors: a row found no slot within the table's probe bound");
  return KMX_OK;
}
extern "C" uint64_t kmx_colors_result_n_classes(kmx_colors_result* R) { return kmx_colors_result_wait(R) == KMX_OK ? R->h_tot[0] : 0; }
extern "C" const uint32_t* kmx_colors_result_ids_dev(kmx_colors_result* R) { return kmx_colors_result_wait(R) == KMX_OK ? R->d_ids : nullptr; }
// (kmx_colors_result_wait first: behind it mat_copy_out's own wait returns its status)
static int colors_copy_out(kmx_colors_result* R, void* dst, uint64_t dst_entries, const void* src, u64 entries, u32 entry_bytes)
{
  const int rc = kmx_colors_result_wait(R);
  return rc != KMX_OK ? rc : mat_copy_out(R, dst, dst_entries, src, entries, entry_bytes);
}
extern "C" int kmx_colors_result_copy_ids(kmx_colors_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? colors_copy_out(R, host_dst, dst_entries, R->d_ids, R->n_rows, 4) : KMX_E_INVAL; }
extern "C" int kmx_colors_result_copy_first(kmx_colors_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? colors_copy_out(R, host_dst, dst_entries, R->d_first, kmx_colors_result_n_classes(R), 4) : KMX_E_INVAL; }
extern "C" int kmx_colors_result_copy_sizes(kmx_colors_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? colors_copy_out(R, host_dst, dst_entries, R->d_size, kmx_colors_result_n_classes(R), 4) : KMX_E_INVAL; }
extern "C" int kmx_colors_result_copy_patterns(kmx_colors_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? colors_copy_out(R, host_dst, dst_entries, R->d_patterns, kmx_colors_result_n_classes(R) * R->W, 8) : KMX_E_INVAL; }
extern "C" double kmx_colors_result_kernel_ms(kmx_colors_result* R) { return R && R->ev[0] && kmx_colors_result_wait(R) == KMX_OK ? mat_kernel_ms(R) : -1.0; }
extern "C" int kmx_colors_result_kernel_parts_ms(kmx_colors_result* R, double* pack_ms, double* claim_ms, double* number_ms)
{
  if (R && R->ev[0]) (void)kmx_colors_result_wait(R);      // (without profiling nothing is waited for)
  return mat_kernel_parts_ms(R, {pack_ms, claim_ms, number_ms});
}
extern "C" uint64_t kmx_colors_result_algo_bytes(kmx_colors_result* R)
{
  if (kmx_colors_result_wait(R) != KMX_OK) return 0;
  const u64 n = R->n_rows, C = R->h_tot[0], W = R->W;
  return n * R->row_bytes + 2 * n * (8 * W + 8) + 4 * n + C * (8 + 8 * W);
}
extern "C" void kmx_colors_result_free(kmx_colors_result* R) { mat_free(R); }
