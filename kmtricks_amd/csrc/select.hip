// select.hip -- `kmx select` on the device: a smaller matrix out of a larger one -- the rows whose recurrence over a list of columns lies
// in [min_rec, max_rec], rebuilt with those columns alone, in the list's order, as counts or as presence/absence bits (include/kmx.h,
// section "select"; what MUSET's `kmat_tools filter` does on text).  No reference counterpart in the kmtricks tree.  gfx950, wave64.
//
//   k_select_score   a wave a chunk of rows, k_diff_score's decomposition: a row of 64 units and more (a unit: a count, or a payload
//                    byte) is read by the whole wave, shorter rows by the L lanes of a sub-group, 64 / L rows at a time; the recurrence
//                    is a butterfly over the row's lanes.  The selection comes as a table per INPUT column (COUNT: a flag byte a column;
//                    PA: a mask a payload byte, so rec = popc(x & mask)).  Lane i of the wave ends with row i of the chunk and writes
//                    its keep word and its recurrence; the kept rows of a tile of 256 are counted with one atomic add a wave.
//   k_select_move_*  the kept rows of a tile are contiguous in the output.  That stretch is cut in output units and a lane owns a unit:
//                    its place gives the kept row (rank) and the place in the row, it gathers what belongs there and stores it, so
//                    the stores of a wave are 64 consecutive units whatever the row size, and no lane idles on short rows.
//                      cc  COUNT -> COUNT   a unit is a dword (an output row is 8 kw + 4 M bytes and the buffer is aligned: every
//                                           output dword is); a key dword is copied, a count is gathered from column cols[j]
//                      pa  COUNT -> PA      a unit is a byte (an output row of 8 kw + ceil(M / 8) bytes starts anywhere): a key byte
//                          PA -> PA         is copied; a payload byte is put together from the 8 columns cols[8 j ... 8 j + 7] --
//                                           8 counts compared with a, or 8 bits picked out of their bytes
//                    S workgroups share a tile (each works out the tile's ranks for itself: 256 keep words) and stride over its units.
//   k_select_place   the (row, rec) records of the kept rows, gathered to their rank.
// The tile bases are k_filter_scan's.  With cols = NULL, the same mode, no ZERO_BELOW and no padding bits (COUNT, or PA with N a multiple
// of 8) an output row IS the input row and k_filter_move moves it whole, as for diff; every other call takes the movers here.
// Every load of a body byte is inside [rows, rows + n_rows * row_bytes): an address is rows + r * row_bytes + skip + b with r < n_rows
// and b + (bytes loaded) <= row_bytes - skip (or rows + r * row_bytes + b inside the key), both tested by the lane that loads; nothing
// is loaded in wider pieces than the piece that is tested and nothing is rounded to an aligned address.  No store lies outside the kept
// rows.
#include "matrix_host.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 SL_TILE = 256;              // rows of a placement tile: k_filter_move's (filter_tiles)
constexpr u32 SL_MAX_GRID = 1u << 18;     // workgroups of a launch: the kernels stride over their work
constexpr u32 SL_WAVES_PER_SIMD = 8;      // chunks of long rows are made small enough for this many waves a SIMD
constexpr u32 SL_LOADS_PER_WG = 8192;     // gathered loads a mover's workgroup aims at: a tile is shared by tile loads / this many
constexpr u32 SL_NONE = 0xFFFFFFFFu;      // the padding of the column list: no column (N <= 2^32 - 1)


struct SelRec { u32 row, rec; };      // kmx_select_rec
static_assert(sizeof(SelRec) == 8 && sizeof(kmx_select_rec) == 8, "a record is 8 bytes");

// sel: COUNT -- a flag byte per input column; PA -- a mask per payload byte (unselected and padding bits 0).
// L: lanes of a row (a power of two <= 64); RW: rows of a wave's chunk (64 when L < 64; a power of two <= 64 when L == 64).
template <bool COUNT>
__global__ __launch_bounds__(256)
void k_select_score(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 L, u32 RW, const u8* __restrict__ sel,
                    u32 a, u32 min_rec, u32 max_rec, u32* __restrict__ keep, u32* __restrict__ recv, u32* __restrict__ tile_cnt)
{
  const u32 lane = threadIdx.x & 63u, u = lane & (L - 1u), sub = lane / L;
  const u32 units = COUNT ? N : (u32)(((u64)N + 7) / 8);
  const u32 passes = L == 64 ? RW : L;
  const u64 n_chunks = ((u64)n_rows + RW - 1) / RW;
  // what the lane's first units are selected by, read once: COUNT a bit a unit for 32 units, PA the mask of one byte
  u32 gp = 0;
  if (COUNT) {
    for (u32 i = 0; i < 32; i++) { const u64 un = (u64)u + (u64)L * i; if (un < units && sel[un]) gp |= 1u << i; }
  } else if (u < units) gp = sel[u];
  for (u64 g = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; g < n_chunks; g += (u64)gridDim.x * 4) {
    const u64 row0 = g * RW;
    u32 rec = 0;
    for (u32 p = 0; p < passes; p++) {
      const u64 row = row0 + (u64)sub * L + p;
      u32 acc = 0;
      if (row < n_rows) {
        const u8* q = rows + row * row_bytes + skip;
        u32 i = 0;
        for (u64 un = u; un < units; un += L, i++) {
          if (COUNT) {
            const u32 v = reinterpret_cast<const UDword*>(q + 4 * un)->v;
            const u32 f = i < 32 ? (gp >> i) & 1u : (u32)(sel[un] != 0);
            acc += f & (u32)(v >= a);
          } else {
            const u32 x = q[un];
            const u32 m = i == 0 ? gp : (u32)sel[un];
            acc += (u32)__popc(x & m);
          }
        }
      }
      for (u32 o = L >> 1; o; o >>= 1) acc += __shfl_xor(acc, (int)o);
      if (u == p) rec = acc;
    }
    // lane i holds row row0 + i
    const u64 mine = row0 + lane;
    const bool have = lane < RW && mine < n_rows;
    const bool kept = have && rec >= min_rec && rec <= max_rec;
    if (have) { keep[mine] = kept ? 1u : 0u; recv[mine] = rec; }
    const u32 nk = (u32)__popcll(__ballot(kept));
    if (lane == 0 && nk) atomicAdd(&tile_cnt[row0 / SL_TILE], nk);      // (a chunk lies in one tile: RW divides SL_TILE)
  }
}

// the kept rows of tile t: s_src[rank] = the row's place in the tile; -> their number.  Every thread of the workgroup calls it.
__device__ __forceinline__ u32 sl_tile_ranks(const u32* __restrict__ keep, u32 n_rows, u32 t, u32* s_w, u32* s_src)
{
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u64 row = (u64)t * SL_TILE + tid;
  const bool k = row < n_rows && keep[row] != 0;
  const u64 bal = __ballot(k);
  if (lane == 0) s_w[wave] = (u32)__popcll(bal);
  __syncthreads();
  u32 rank = (u32)__popcll(bal & ((1ULL << lane) - 1ULL)), nk = 0;
  for (u32 w = 0; w < SL_TILE / 64; w++) { if (w < wave) rank += s_w[w]; nk += s_w[w]; }
  if (k) s_src[rank] = tid;
  __syncthreads();
  return nk;
}

// COUNT -> COUNT.  kd: dwords of a key; cols[M]; zb: counts below it leave as 0 (0: none does).  A lane an output dword.
__global__ __launch_bounds__(SL_TILE)
void k_select_move_cc(const u8* __restrict__ rows, u32 n_rows, u64 irb, u32 N, u32 kd, u32 M, const u32* __restrict__ cols, u32 zb,
                      const u32* __restrict__ keep, const u32* __restrict__ tile_base, u32 S, u32* __restrict__ out)
{
  __shared__ u32 s_w[SL_TILE / 64];
  __shared__ u32 s_src[SL_TILE];
  const u32 tid = threadIdx.x;
  const u32 odw = kd + M;      // dwords of an output row (a row is below 4 GiB)
  const u64 n_groups = (((u64)n_rows + SL_TILE - 1) / SL_TILE) * S;
  for (u64 g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const u32 t = (u32)(g / S), s = (u32)(g % S);
    const u32 nk = sl_tile_ranks(keep, n_rows, t, s_w, s_src);
    if (nk) {
      u32* dst = out + (u64)tile_base[t] * odw;
      const u8* tile_rows = rows + (u64)t * SL_TILE * irb;
      const u64 total = (u64)nk * odw;
      const bool small = total <= 0xFFFFFFFFull;
      for (u64 e = (u64)s * SL_TILE + tid; e < total; e += (u64)S * SL_TILE) {
        u32 r, c;
        if (small) { r = (u32)e / odw; c = (u32)e - r * odw; } else { r = (u32)(e / odw); c = (u32)(e - (u64)r * odw); }
        const u8* src = tile_rows + (u64)s_src[r] * irb;      // (s_src[r] is a row below n_rows: sl_tile_ranks)
        u32 v = 0;
        if (c < kd) v = reinterpret_cast<const UDword*>(src + 4ull * c)->v;
        else {
          const u32 col = cols[c - kd];
          if (col < N) { v = reinterpret_cast<const UDword*>(src + 4ull * kd + 4ull * col)->v; if (v < zb) v = 0; }
        }
        dst[e] = v;
      }
    }
    __syncthreads();
  }
}

// -> PA.  kb: bytes of a key; ob = ceil(M / 8); cols[8 * ob], the entries from M on SL_NONE.  A lane an output byte.
template <bool COUNT>
__global__ __launch_bounds__(SL_TILE)
void k_select_move_pa(const u8* __restrict__ rows, u32 n_rows, u64 irb, u32 N, u32 kb, u32 ob, const u32* __restrict__ cols, u32 a,
                      const u32* __restrict__ keep, const u32* __restrict__ tile_base, u32 S, u8* __restrict__ out)
{
  __shared__ u32 s_w[SL_TILE / 64];
  __shared__ u32 s_src[SL_TILE];
  const u32 tid = threadIdx.x;
  const u32 orb = kb + ob;      // bytes of an output row (below 4 GiB)
  const u64 n_groups = (((u64)n_rows + SL_TILE - 1) / SL_TILE) * S;
  for (u64 g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const u32 t = (u32)(g / S), s = (u32)(g % S);
    const u32 nk = sl_tile_ranks(keep, n_rows, t, s_w, s_src);
    if (nk) {
      u8* dst = out + (u64)tile_base[t] * orb;
      const u8* tile_rows = rows + (u64)t * SL_TILE * irb;
      const u64 total = (u64)nk * orb;
      const bool small = total <= 0xFFFFFFFFull;
      for (u64 e = (u64)s * SL_TILE + tid; e < total; e += (u64)S * SL_TILE) {
        u32 r, c;
        if (small) { r = (u32)e / orb; c = (u32)e - r * orb; } else { r = (u32)(e / orb); c = (u32)(e - (u64)r * orb); }
        const u8* src = tile_rows + (u64)s_src[r] * irb;      // (s_src[r] is a row below n_rows: sl_tile_ranks)
        u32 x = 0;
        if (c < kb) x = src[c];
        else {
          const u32* cj = cols + 8ull * (c - kb);
          const u8* pay = src + kb;
#pragma unroll
          for (u32 k = 0; k < 8; k++) {
            const u32 col = cj[k];
            if (col < N) {
              if (COUNT) x |= (u32)(reinterpret_cast<const UDword*>(pay + 4ull * col)->v >= a) << k;
              else x |= (((u32)pay[col >> 3] >> (col & 7u)) & 1u) << k;
            }
          }
        }
        dst[e] = (u8)x;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(SL_TILE)
void k_select_place(const u32* __restrict__ keep, const u32* __restrict__ recv, u32 n_rows, const u32* __restrict__ tile_base,
                    SelRec* __restrict__ out)
{
  __shared__ u32 s_w[SL_TILE / 64];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 n_tiles = (u32)(((u64)n_rows + SL_TILE - 1) / SL_TILE);
  for (u32 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 row = (u64)t * SL_TILE + tid;
    const bool k = row < n_rows && keep[row] != 0;
    const u64 bal = __ballot(k);
    if (lane == 0) s_w[wave] = (u32)__popcll(bal);
    __syncthreads();
    u32 rank = (u32)__popcll(bal & ((1ULL << lane) - 1ULL));
    for (u32 w = 0; w < wave; w++) rank += s_w[w];
    if (k) { SelRec q; q.row = (u32)row; q.rec = recv[row]; out[(u64)tile_base[t] + rank] = q; }
    __syncthreads();
  }
}

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
struct kmx_select_result : MatResult {
  u64 orb = 0;                          // bytes of an output row (row_bytes: of an input row)
  SelRec* d_recs = nullptr;
  u8* d_out = nullptr;
};

static int select_check(kmx_ctx* ctx, const kmx_select_task* T, const char* who, u64* irb)
{
  const MatCheck c{ctx, who};
  const u32 N = T->n_cols, M = T->n_out;
  int rc;
  if ((rc = c.n_cols(N, M, "selection")) || (rc = c.no_bloom(T->mode, ": a Bloom row's identity is its position")) || (rc = c.mode(T->mode))) return rc;
  if (T->out_mode != KMX_MODE_COUNT && T->out_mode != KMX_MODE_PA) return c.no(KMX_E_INVAL, ": out_mode must be KMX_MODE_COUNT or KMX_MODE_PA");
  if (T->mode == KMX_MODE_PA && T->out_mode == KMX_MODE_COUNT) return c.no(KMX_E_INVAL, ": counts cannot be made out of presence/absence rows");
  if ((rc = c.key_words(T->key_words)) || (rc = c.min_abund(T->min_abund, T->mode)) || (rc = c.flags(T->flags, KMX_SELECT_ZERO_BELOW))) return rc;
  if ((T->flags & KMX_SELECT_ZERO_BELOW) && T->out_mode != KMX_MODE_COUNT) return c.no(KMX_E_INVAL, ": KMX_SELECT_ZERO_BELOW needs a COUNT output");
  if ((rc = c.list_fits(M, N, "output")) || (rc = c.identity(T->cols, M, N, "n_out"))) return rc;
  *irb = MatCheck::row_bytes(T->key_words, T->mode, N);
  if ((rc = c.row_fits(*irb)) || (rc = c.n_rows(T->n_rows)) || (rc = c.rows(T->n_rows, T->rows))) return rc;
  return c.col_list(T->cols, M, N);
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int select_queue(kmx_ctx* ctx, const kmx_select_task* T, kmx_select_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, M = T->n_out, kw = T->key_words, skip = 8 * kw, n_rows = (u32)R->n_rows, tiles = filter_tiles(n_rows);
  const bool count = T->mode == KMX_MODE_COUNT, out_count = T->out_mode == KMX_MODE_COUNT, zb = (T->flags & KMX_SELECT_ZERO_BELOW) != 0;
  const u32 units = count ? N : (u32)(((u64)N + 7) / 8);
  R->orb = MatCheck::row_bytes(kw, T->out_mode, M);
  // an output row is the input row: k_filter_move takes it whole (PA: only without padding bits, which must leave as 0)
  const bool whole = !T->cols && T->mode == T->out_mode && !zb && (count || N % 8 == 0);
  const u64 sel_bytes = ((u64)units + 3) & ~3ull, n_list = whole ? 0 : ((u64)M + 7) & ~7ull;
  u8* h_tab;      // page-locked: the selection table, then the column list, on their way up
  if (!(R->h_tot = (u32*)R->pin(64)) || !(h_tab = (u8*)R->pin(sel_bytes + 4 * n_list + 4))) return ctx->fail(KMX_E_NOMEM, "kmx_select: host allocation failed");
  R->h_tot[0] = 0;
  // per input column: is it selected?  (PA: as a mask per payload byte -- bit i & 7 of byte i >> 3; the padding bits stay 0)
  u32* h_cols = reinterpret_cast<u32*>(h_tab + sel_bytes);
  if (!T->cols) {
    if (count) memset(h_tab, 1, N);
    else { memset(h_tab, 0xFF, units); if (N % 8) h_tab[units - 1] = (u8)((1u << (N % 8)) - 1u); }
  } else {
    memset(h_tab, 0, sel_bytes);
    for (u32 j = 0; j < M; j++) { const u32 c = T->cols[j]; if (count) h_tab[c] = 1; else h_tab[c >> 3] |= (u8)(1u << (c & 7)); }
  }
  for (u64 j = 0; j < n_list; j++) h_cols[j] = j < M ? (T->cols ? T->cols[j] : (u32)j) : SL_NONE;
  u32* d_keep = (u32*)R->tmp(4ull * n_rows);
  u32* d_recv = (u32*)R->tmp(4ull * n_rows);
  u32* d_tiles = (u32*)R->keep(4ull * ((u64)tiles + 1));
  R->d_recs = (SelRec*)R->keep(sizeof(SelRec) * (u64)n_rows);      // every row kept
  R->d_out = (u8*)R->keep((u64)n_rows * R->orb + 16);
  u8* d_sel = (u8*)R->tmp(sel_bytes + 4 * n_list + 4);             // the table, and behind it (at a multiple of 4) the list
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_select: device allocation failed (send the body in runs of rows)");
  const u32* d_cols = reinterpret_cast<const u32*>(d_sel + sel_bytes);
  KMX_HIP(ctx, hipMemcpyAsync(d_sel, h_tab, sel_bytes + 4 * n_list, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_tiles, 0, 4ull * ((u64)tiles + 1), st));
  const u32 max_rec = T->max_rec >= M ? 0xFFFFFFFFu : T->max_rec;
  if (n_rows) {
    // rows of 64 units and more get a wave each; their chunks shrink until the chip has SL_WAVES_PER_SIMD waves a SIMD to hide the loads
    const RowPlan p = mat_row_plan(units, n_rows, (u32)std::max(kmx_plan_cus(ctx), 1), SL_WAVES_PER_SIMD);
    const u32 grid = (u32)std::min<u64>((p.chunks + 3) / 4, kmx_grid_cap(SL_MAX_GRID));
    if (count) hipLaunchKernelGGL(k_select_score<true>, dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, p.L, p.RW, (const u8*)d_sel,
                                  T->min_abund, T->min_rec, max_rec, d_keep, d_recv, d_tiles);
    else hipLaunchKernelGGL(k_select_score<false>, dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, p.L, p.RW, (const u8*)d_sel,
                            T->min_abund, T->min_rec, max_rec, d_keep, d_recv, d_tiles);
    KMX_HIP(ctx, hipGetLastError());
  }
  KMX_HIP(ctx, launch_filter_scan(d_tiles, tiles, st));
  if (n_rows) {
    if (whole) KMX_HIP(ctx, launch_filter_move((const u8*)T->rows, n_rows, R->row_bytes, R->row_bytes, d_keep, d_keep, d_tiles, R->d_out, st));
    else {
      // gathered loads of a tile with every row kept: the key's units, then one a count (-> COUNT) or eight a payload byte (-> PA)
      const u64 loads = (u64)SL_TILE * (out_count ? 2ull * kw + M : 8ull * kw + 8ull * (((u64)M + 7) / 8));
      const u32 S = (u32)std::min<u64>(std::max<u64>((loads + SL_LOADS_PER_WG - 1) / SL_LOADS_PER_WG, 1), 1024);
      const u32 grid = (u32)std::min<u64>((u64)tiles * S, kmx_grid_cap(SL_MAX_GRID));
      const u32 ob = (u32)(((u64)M + 7) / 8);
      if (out_count) hipLaunchKernelGGL(k_select_move_cc, dim3(grid), dim3(SL_TILE), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, N, 2 * kw, M, d_cols,
                                        zb ? T->min_abund : 0u, (const u32*)d_keep, (const u32*)d_tiles, S, (u32*)R->d_out);
      else if (count) hipLaunchKernelGGL(k_select_move_pa<true>, dim3(grid), dim3(SL_TILE), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, N, skip, ob, d_cols,
                                         T->min_abund, (const u32*)d_keep, (const u32*)d_tiles, S, R->d_out);
      else hipLaunchKernelGGL(k_select_move_pa<false>, dim3(grid), dim3(SL_TILE), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, N, skip, ob, d_cols,
                              T->min_abund, (const u32*)d_keep, (const u32*)d_tiles, S, R->d_out);
      KMX_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_select_place, dim3(std::min(tiles, kmx_grid_cap(SL_MAX_GRID))), dim3(SL_TILE), 0, st, (const u32*)d_keep, (const u32*)d_recv, n_rows,
                       (const u32*)d_tiles, R->d_recs);
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R, d_tiles + tiles);
}

extern "C" int kmx_select_dev(kmx_ctx* ctx, const kmx_select_task* task, kmx_select_result** out)
{ return mat_call(ctx, task, out, false, "kmx_select_dev", "kmx_select", select_check, select_queue); }
extern "C" int kmx_select_host(kmx_ctx* ctx, const kmx_select_task* task, kmx_select_result** out)
{ return mat_call(ctx, task, out, true, "kmx_select_host", "kmx_select", select_check, select_queue); }

extern "C" int kmx_select_result_wait(kmx_select_result* R) { return mat_wait(R); }
extern "C" uint64_t kmx_select_result_rows(kmx_select_result* R) { return mat_wait(R) == KMX_OK ? R->h_tot[0] : 0; }
extern "C" uint64_t kmx_select_result_row_bytes(const kmx_select_result* R) { return R ? R->orb : 0; }
extern "C" uint64_t kmx_select_result_body_bytes(kmx_select_result* R) { return R ? kmx_select_result_rows(R) * R->orb : 0; }
extern "C" const void* kmx_select_result_body_dev(kmx_select_result* R) { return mat_wait(R) == KMX_OK ? R->d_out : nullptr; }
extern "C" const kmx_select_rec* kmx_select_result_recs_dev(kmx_select_result* R) { return mat_wait(R) == KMX_OK ? (const kmx_select_rec*)R->d_recs : nullptr; }
extern "C" int kmx_select_result_copy_body(kmx_select_result* R, void* host_dst, uint64_t dst_bytes)
{ return R ? mat_copy_out(R, host_dst, dst_bytes, R->d_out, kmx_select_result_body_bytes(R), 1) : KMX_E_INVAL; }
extern "C" int kmx_select_result_copy_recs(kmx_select_result* R, kmx_select_rec* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_recs, kmx_select_result_rows(R), sizeof(SelRec)) : KMX_E_INVAL; }
extern "C" double kmx_select_result_kernel_ms(kmx_select_result* R) { return mat_kernel_ms(R); }
extern "C" uint64_t kmx_select_result_algo_bytes(kmx_select_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  return R->n_rows * R->row_bytes + (u64)R->h_tot[0] * (R->orb + sizeof(SelRec));
}
extern "C" void kmx_select_result_free(kmx_select_result* R) { mat_free(R); }
