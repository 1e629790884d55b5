// assoc.hip -- `kmx assoc` on the device: the structure-corrected association test of a matrix's rows (include/kmx.h, section "assoc"; the
// score test that kmdiff, EIGENSTRAT and a k-mer GWAS run once the covariates are projected out of the phenotype and of the row).  Per row
// the recurrence and V exact i64 sums of fixed-point regressors over the present listed samples, then a scalar formula in IEEE double.
// No reference counterpart in the kmtricks tree.  gfx950, wave64.
//
//   k_assoc_score  a lane a row.  A workgroup is ONE wave and takes groups of 64 rows.  A group's rows are read one after the other, a
//                  lane a unit (a count, or a payload byte): 64 units of a row are a coalesced load, and a __ballot turns them into the
//                  64-bit presence mask of the row's 64 columns (PA: eight masks, one per bit of the byte: 512 columns).  Lane r keeps
//                  the masks of row r -- k_gram_slab's transposition.  The wave then walks the block's columns with the column index
//                  wave-uniform: vt[c][0 ... VP) comes in scalar loads, and per lane acc_j += bit ? vt[c][j] : 0.  No cross-lane
//                  reduction: at the end lane r holds rec and the V sums of row r and the 64 formulas run side by side, as in
//                  k_diff_score.  The kept rows of a tile of 256 are counted with one atomic add a wave.
//                  vt holds the entries BIASED by 2^31 (u32 = entry + 2^31) and padded with the bias to VP >= V vectors and to a
//                  multiple of 8 columns: a masked biased entry is added as an unsigned 32-bit number into a u64 (an and, an add, an
//                  add-with-carry), and s_j = acc_j - rec * 2^31.  No partial sum is narrower than 64 bits; acc_j <= N * (2^32 - 1)
//                  cannot wrap.  VP is a template parameter (1, 2, 4, 8, 12, 16, 24, 32): the accumulators stay in registers.
//   k_assoc_place  the records of the kept rows, gathered to their final place (rank in the tile + the tile's base): k_diff_place for
//                  32-byte records.
// The tile bases are k_filter_scan's and the kept rows are moved by k_filter_move (filter.hip), both unchanged, as diff.hip uses them.
// No kernel waits on another workgroup.  Every load of a body byte is inside [rows, rows + n_rows * row_bytes): an address is rows +
// r * row_bytes + skip + b with r < n_rows and b + (bytes loaded) <= row_bytes - skip, both tested by the lane that loads; nothing is
// loaded in wider pieces than the piece that is tested (a byte for PA, a count's dword for COUNT) and nothing is rounded to an aligned
// address.  The launch knobs of this file are its own: KMX_ASSOC_CUS and KMX_ASSOC_GRID.
#include "matrix_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace kmx {

constexpr u32 AS_TILE = 256;              // rows of a placement tile: k_filter_move's (filter_tiles)
constexpr u32 AS_GROUP = 64;              // rows of a wave's group: a lane a row
constexpr u32 AS_WGS_PER_CU = 32;         // one-wave workgroups k_assoc_score aims at: eight a SIMD
constexpr u32 AS_MAX_GRID = 1u << 18;     // workgroups of a launch: the kernels stride over their work
constexpr int AS_VC = 8;                  // vectors of one walk over a block's columns (COUNT) ...
constexpr int AS_VC_PA = 4;               // ... and over a block's payload bytes, eight columns a step (PA)
constexpr u32 AS_LOADS_PA = 4;            // ... PA: every row is eight ballots
constexpr u32 AS_LOADS = 8;               // rows whose loads a lane has in flight before the first ballot

typedef long long i64;

struct AssocPrm { double sc, gain, vmin, thr; u32 min_rec, max_rec; };      // the scalars of a call, in device memory
struct AssocRec { double stat, beta; i64 s0; u32 rec, row; };      // kmx_assoc_rec
static_assert(sizeof(AssocRec) == 32 && sizeof(kmx_assoc_rec) == 32, "a record is 32 bytes");
static_assert(sizeof(kmx_assoc_task) == 96, "kmx_assoc_task is 96 bytes");

// the statistic of include/kmx.h, in IEEE double in the order written there: no contraction into fma.  acc: the biased sums.  The
// vectors from V on are the table's padding: their s_j is 0, a = +0, a * a = +0 and h + (+0) is h bit for bit (h is never -0: it
// starts at +0 and only squares are added), so the loop runs to VP without a test.
template <int VP>
__device__ __forceinline__ void assoc_formula(const u64 (&acc)[VP], u32 rec, double sc, double gain, double vmin, i64* s0, double* stat, double* beta)
{
#pragma clang fp contract(off)
  const u64 bias = (u64)rec << 31;
  *s0 = (i64)(acc[0] - bias);
  const double u = (double)*s0 * sc;
  double h = 0.0;
#pragma unroll
  for (int j = 1; j < VP; j++) { const double a = (double)(i64)(acc[j] - bias) * sc; h = h + a * a; }
  const double v = (double)rec - h;
  if (v > vmin) { *beta = u / v; *stat = (gain * (u * u)) / v; }
  else { *beta = 0.0; *stat = 0.0; }
}

// lst: a byte a unit -- COUNT: 1 where the column is listed; PA: the listed columns of the payload byte (no padding bit).
// vt: [N rounded up to 8][VP] biased entries; the rows of unlisted columns and the vectors from V on hold the bias (the value 0).
template <bool COUNT, int VP>
__global__ __launch_bounds__(64)
void k_assoc_score(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, const u8* __restrict__ lst,
                   const u32* __restrict__ vt, u32 a, const AssocPrm* __restrict__ prm,
                   u32* __restrict__ keep, AssocRec* __restrict__ recs, u32* __restrict__ tile_cnt)
{
  const u32 lane = threadIdx.x;
  const u32 units = COUNT ? N : (u32)(((u64)N + 7) / 8);
  const u32 n_blocks = (u32)(((u64)units + 63) / 64);
  const u64 n_groups = ((u64)n_rows + AS_GROUP - 1) / AS_GROUP;
  for (u64 g = blockIdx.x; g < n_groups; g += gridDim.x) {      // (uniform over the wave)
    const u64 row0 = g * AS_GROUP;
    const u32 nr = (u32)min((u64)AS_GROUP, (u64)n_rows - row0);
    u64 acc[VP];
#pragma unroll
    for (int j = 0; j < VP; j++) acc[j] = 0;
    u32 rec = 0;
    for (u32 b = 0; b < n_blocks; b++) {
      const u64 un = (u64)b * 64 + lane;
      const u32 m = un < units ? (u32)lst[un] : 0u;      // 0: nothing of this lane's unit is listed, or there is no such unit
      const u8* p = rows + row0 * row_bytes + skip + (COUNT ? 4 * un : un);
      if (COUNT) {      // a block: 64 columns
        u64 mine = 0;
        for (u32 r0 = 0; r0 < nr; r0 += AS_LOADS) {
          u32 x[AS_LOADS];
#pragma unroll
          for (u32 k = 0; k < AS_LOADS; k++) {
            x[k] = 0;      // (below a: a >= 1)
            if (m && r0 + k < nr) x[k] = reinterpret_cast<const UDword*>(p + (u64)(r0 + k) * row_bytes)->v;
          }
#pragma unroll
          for (u32 k = 0; k < AS_LOADS; k++) {      // (every lane of the wave goes round)
            const u64 bal = __ballot(x[k] >= a);
            if (lane == r0 + k) mine = bal;
          }
        }
        rec += (u32)__popcll(mine);
        const u32 cn = min(64u, N - b * 64);
#pragma unroll
        for (int j0 = 0; j0 < VP; j0 += AS_VC) {      // AS_VC vectors a walk: the entries of a column stay in few scalar registers
          const u32* t = vt + (u64)b * 64 * VP + j0;
          for (u32 i = 0; i < cn; i++, t += VP) {      // column b * 64 + i: uniform over the wave
            const u32 msk = 0u - (u32)((mine >> i) & 1ull);
#pragma unroll
            for (int j = 0; j < AS_VC; j++) if (j0 + j < VP) acc[j0 + j] += (u64)(t[j] & msk);
          }
        }
      } else {          // a block: 64 payload bytes, 512 columns
        u64 mine[8];
#pragma unroll
        for (int j = 0; j < 8; j++) mine[j] = 0;
        for (u32 r0 = 0; r0 < nr; r0 += AS_LOADS_PA) {
          u32 x[AS_LOADS_PA];
#pragma unroll
          for (u32 k = 0; k < AS_LOADS_PA; k++) {
            x[k] = 0;
            if (m && r0 + k < nr) x[k] = (u32)p[(u64)(r0 + k) * row_bytes] & m;
          }
#pragma unroll
          for (u32 k = 0; k < AS_LOADS_PA; k++) {      // (every lane of the wave goes round)
#pragma unroll
            for (int j = 0; j < 8; j++) {
              const u64 bal = __ballot(((x[k] >> j) & 1u) != 0);
              if (lane == r0 + k) mine[j] = bal;
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) rec += (u32)__popcll(mine[j]);
        const u32 bn = min(64u, units - b * 64);      // payload bytes of the block; vt has a row for each of their 8 columns
#pragma unroll
        for (int j0 = 0; j0 < VP; j0 += AS_VC_PA) {
          const u32* t = vt + (u64)b * 512 * VP + j0;
          for (u32 l = 0; l < bn; l++) {      // byte b * 64 + l, columns 8 * that + c: uniform over the wave
#pragma unroll
            for (int c = 0; c < 8; c++, t += VP) {
              const u32 msk = 0u - (u32)((mine[c] >> l) & 1ull);
#pragma unroll
              for (int j = 0; j < AS_VC_PA; j++) if (j0 + j < VP) acc[j0 + j] += (u64)(t[j] & msk);
            }
          }
        }
      }
    }
    // lane i holds row row0 + i
    const u64 mine_row = row0 + lane;
    bool kept = false;
    if (lane < nr) {
      // the call's scalars are fetched here, once a group, and not kept in registers across the walk
      const AssocPrm* q_prm = prm;
      asm volatile("" : "+s"(q_prm));
      const AssocPrm P = *q_prm;
      i64 s0; double stat, beta;
      assoc_formula<VP>(acc, rec, P.sc, P.gain, P.vmin, &s0, &stat, &beta);
      kept = rec >= P.min_rec && rec <= P.max_rec && stat >= P.thr;
      keep[mine_row] = kept ? 1u : 0u;
      if (kept) {
        AssocRec q;
        q.stat = stat; q.beta = beta; q.s0 = s0; q.rec = rec; q.row = (u32)mine_row;
        recs[mine_row] = q;
      }
    }
    const u32 nk = (u32)__popcll(__ballot(kept));
    if (lane == 0 && nk) atomicAdd(&tile_cnt[row0 / AS_TILE], nk);      // (a group lies in one tile: AS_GROUP divides AS_TILE)
  }
}

__global__ __launch_bounds__(AS_TILE)
void k_assoc_place(const u32* __restrict__ keep, const AssocRec* __restrict__ recs, u32 n_rows, const u32* __restrict__ tile_base,
                   AssocRec* __restrict__ out)
{
  __shared__ u32 s_w[AS_TILE / 64];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 n_tiles = (u32)(((u64)n_rows + AS_TILE - 1) / AS_TILE);
  for (u32 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 row = (u64)t * AS_TILE + tid;
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

// the vectors a kernel is built for: the smallest of these at or above V
static u32 as_vp(u32 V)
{
  const u32 steps[] = {1, 2, 4, 8, 12, 16, 24, 32};
  for (u32 s : steps) if (V <= s) return s;
  return 32;
}
static u32 as_cus(const kmx_ctx* ctx) { return (u32)std::max(kmx_env_cus("KMX_ASSOC_CUS", ctx), 1); }
static u32 as_grid(u64 dflt) { return kmx_env_grid("KMX_ASSOC_GRID", dflt); }

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
struct kmx_assoc_result : MatResult {
  u32 n_vec = 0;
  AssocRec* d_recs = nullptr;
  u8* d_out = nullptr;
};

static int assoc_check(kmx_ctx* ctx, const kmx_assoc_task* T, const char* who, u64* row_bytes)
{
  const MatCheck c{ctx, who};
  const u32 N = T->n_cols, M = T->n_use, V = T->n_vec;
  int rc;
  if ((rc = c.n_cols(N, M, "list")) || (rc = c.no_bloom(T->mode, ": a Bloom row is a hash bit, its presence pattern is not a k-mer's")) || (rc = c.mode(T->mode)) ||
      (rc = c.key_words(T->key_words)) || (rc = c.min_abund(T->min_abund, T->mode)) || (rc = c.flags(T->flags, 0))) return rc;
  if (V == 0 || V > 32) return c.no(KMX_E_INVAL, ": n_vec must be 1 ... 32");
  if (!T->vecs) return c.no(KMX_E_INVAL, ": null vecs");
  if (T->frac_bits > 62) return c.no(KMX_E_INVAL, ": frac_bits must be 0 ... 62");
  if (!std::isfinite(T->gain) || !(T->gain > 0.0)) return c.no(KMX_E_INVAL, ": the gain is a finite number above 0");
  if (std::isnan(T->vmin) || T->vmin < 0.0) return c.no(KMX_E_INVAL, ": vmin is a number at or above 0");
  if (std::isnan(T->threshold) || T->threshold < 0.0) return c.no(KMX_E_INVAL, ": the threshold is a number at or above 0");
  if ((rc = c.list_fits(M, N, "listed")) || (rc = c.identity(T->cols, M, N, "n_use"))) return rc;
  *row_bytes = MatCheck::row_bytes(T->key_words, T->mode, N);
  if ((rc = c.row_fits(*row_bytes)) || (rc = c.n_rows(T->n_rows)) || (rc = c.rows(T->n_rows, T->rows)) || (rc = c.col_list(T->cols, M, N))) return rc;
  // (double)s_j must be exact whichever samples are present: the sum of a vector's magnitudes stays below 2^53
  for (u32 j = 0; j < V; j++) {
    u64 sum = 0;      // (M < 2^32 entries below 2^31 + 1: no wrap)
    for (u64 m = 0; m < M; m++) { const i64 e = T->vecs[m * V + j]; sum += (u64)(e < 0 ? -e : e); }
    if (sum >= (1ull << 53)) return c.no(KMX_E_INVAL, ": the magnitudes of vector " + std::to_string(j) + " sum to 2^53 or more: its sums would not be exact in a double");
  }
  return KMX_OK;
}

// what a score launch takes besides its grid
struct AssocArgs { const u8* rows; u32 n_rows; u64 row_bytes; u32 skip, n_cols; const u8* lst; const u32* vt; u32 min_abund; const AssocPrm* prm; u32* keep; AssocRec* recs_all; u32* tiles; };

template <bool COUNT, int VP>
static void assoc_launch_score(u32 grid, hipStream_t st, const AssocArgs& a)
{
  hipLaunchKernelGGL((k_assoc_score<COUNT, VP>), dim3(grid), dim3(64), 0, st, a.rows, a.n_rows, a.row_bytes, a.skip, a.n_cols, a.lst, a.vt,
                     a.min_abund, a.prm, a.keep, a.recs_all, a.tiles);
}
template <bool COUNT>
static void assoc_launch_vp(u32 VP, u32 grid, hipStream_t st, const AssocArgs& a)
{
  switch (VP) {
    case 1: assoc_launch_score<COUNT, 1>(grid, st, a); break;
    case 2: assoc_launch_score<COUNT, 2>(grid, st, a); break;
    case 4: assoc_launch_score<COUNT, 4>(grid, st, a); break;
    case 8: assoc_launch_score<COUNT, 8>(grid, st, a); break;
    case 12: assoc_launch_score<COUNT, 12>(grid, st, a); break;
    case 16: assoc_launch_score<COUNT, 16>(grid, st, a); break;
    case 24: assoc_launch_score<COUNT, 24>(grid, st, a); break;
    default: assoc_launch_score<COUNT, 32>(grid, st, a); break;
  }
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int assoc_queue(kmx_ctx* ctx, const kmx_assoc_task* T, kmx_assoc_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, M = T->n_use, V = R->n_vec = T->n_vec, VP = as_vp(V), skip = 8 * T->key_words, n_rows = (u32)R->n_rows, tiles = filter_tiles(n_rows);
  const bool count = T->mode == KMX_MODE_COUNT;
  const u32 units = count ? N : (u32)(((u64)N + 7) / 8);
  const u64 NR = ((u64)N + 7) / 8 * 8;      // the table's rows: PA walks whole payload bytes
  const u64 vt_bytes = 4 * NR * VP, par_bytes = sizeof(AssocPrm) + vt_bytes + units;      // the scalars, the table, the list
  u8* h_par;      // page-locked: the call's scalars, the biased vector table, the list a byte a unit, on their way up
  if (!(R->h_tot = (u32*)R->pin(64)) || !(h_par = (u8*)R->pin(par_bytes))) return ctx->fail(KMX_E_NOMEM, "kmx_assoc: host allocation failed");
  R->h_tot[0] = 0;
  AssocPrm* h_prm = reinterpret_cast<AssocPrm*>(h_par);
  u32* h_vt = reinterpret_cast<u32*>(h_par + sizeof(AssocPrm));
  u8* h_lst = h_par + sizeof(AssocPrm) + vt_bytes;
  h_prm->sc = std::ldexp(1.0, -(int)T->frac_bits); h_prm->gain = T->gain; h_prm->vmin = T->vmin; h_prm->thr = T->threshold;
  h_prm->min_rec = T->min_rec; h_prm->max_rec = T->max_rec;
  for (u64 i = 0; i < NR * VP; i++) h_vt[i] = 0x80000000u;      // the value 0
  memset(h_lst, 0, units);
  for (u32 m = 0; m < M; m++) {
    const u32 c = T->cols ? T->cols[m] : m;
    for (u32 j = 0; j < V; j++) h_vt[(u64)c * VP + j] = (u32)T->vecs[(u64)m * V + j] ^ 0x80000000u;
    if (count) h_lst[c] = 1; else h_lst[c >> 3] |= (u8)(1u << (c & 7));
  }
  u32* d_keep = (u32*)R->tmp(4ull * n_rows);
  u32* d_tiles = (u32*)R->keep(4ull * ((u64)tiles + 1));
  AssocRec* d_recs_all = (AssocRec*)R->tmp(sizeof(AssocRec) * (u64)n_rows);
  R->d_recs = (AssocRec*)R->keep(sizeof(AssocRec) * (u64)n_rows);      // every row kept
  R->d_out = (u8*)R->keep((u64)n_rows * R->row_bytes + 16);
  u8* d_par = (u8*)R->tmp(par_bytes);
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_assoc: device allocation failed (send the body in runs of rows)");
  KMX_HIP(ctx, hipMemcpyAsync(d_par, h_par, par_bytes, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_tiles, 0, 4ull * ((u64)tiles + 1), st));
  const u32 cap = as_grid(AS_MAX_GRID);
  if (n_rows) {
    const u64 groups = ((u64)n_rows + AS_GROUP - 1) / AS_GROUP;
    const u32 grid = (u32)std::min<u64>(groups, std::min<u64>((u64)as_cus(ctx) * AS_WGS_PER_CU, cap));
    const AssocArgs a{(const u8*)T->rows, n_rows, R->row_bytes, skip, N, d_par + sizeof(AssocPrm) + vt_bytes, reinterpret_cast<const u32*>(d_par + sizeof(AssocPrm)),
                      T->min_abund, reinterpret_cast<const AssocPrm*>(d_par), d_keep, d_recs_all, d_tiles};
    if (count) assoc_launch_vp<true>(VP, grid, st, a);
    else assoc_launch_vp<false>(VP, grid, st, a);
    KMX_HIP(ctx, hipGetLastError());
  }
  KMX_HIP(ctx, launch_filter_scan(d_tiles, tiles, st));
  if (n_rows) {
    KMX_HIP(ctx, launch_filter_move((const u8*)T->rows, n_rows, R->row_bytes, R->row_bytes, d_keep, d_keep, d_tiles, R->d_out, st));
    hipLaunchKernelGGL(k_assoc_place, dim3(std::min(tiles, cap)), dim3(AS_TILE), 0, st, (const u32*)d_keep, (const AssocRec*)d_recs_all, n_rows,
                       (const u32*)d_tiles, R->d_recs);
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R, d_tiles + tiles);
}

extern "C" int kmx_assoc_dev(kmx_ctx* ctx, const kmx_assoc_task* task, kmx_assoc_result** out)
{ return mat_call(ctx, task, out, false, "kmx_assoc_dev", "kmx_assoc", assoc_check, assoc_queue); }
extern "C" int kmx_assoc_host(kmx_ctx* ctx, const kmx_assoc_task* task, kmx_assoc_result** out)
{ return mat_call(ctx, task, out, true, "kmx_assoc_host", "kmx_assoc", assoc_check, assoc_queue); }

extern "C" int kmx_assoc_result_wait(kmx_assoc_result* R) { return mat_wait(R); }
extern "C" uint64_t kmx_assoc_result_rows(kmx_assoc_result* R) { return mat_wait(R) == KMX_OK ? R->h_tot[0] : 0; }
extern "C" uint64_t kmx_assoc_result_row_bytes(const kmx_assoc_result* R) { return R ? R->row_bytes : 0; }
extern "C" uint64_t kmx_assoc_result_body_bytes(kmx_assoc_result* R) { return R ? kmx_assoc_result_rows(R) * R->row_bytes : 0; }
extern "C" const void* kmx_assoc_result_body_dev(kmx_assoc_result* R) { return mat_wait(R) == KMX_OK ? R->d_out : nullptr; }
extern "C" const kmx_assoc_rec* kmx_assoc_result_recs_dev(kmx_assoc_result* R) { return mat_wait(R) == KMX_OK ? (const kmx_assoc_rec*)R->d_recs : nullptr; }
extern "C" int kmx_assoc_result_copy_body(kmx_assoc_result* R, void* host_dst, uint64_t dst_bytes)
{ return R ? mat_copy_out(R, host_dst, dst_bytes, R->d_out, kmx_assoc_result_body_bytes(R), 1) : KMX_E_INVAL; }
extern "C" int kmx_assoc_result_copy_recs(kmx_assoc_result* R, kmx_assoc_rec* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_recs, kmx_assoc_result_rows(R), sizeof(AssocRec)) : KMX_E_INVAL; }
extern "C" double kmx_assoc_result_kernel_ms(kmx_assoc_result* R) { return mat_kernel_ms(R); }
extern "C" uint64_t kmx_assoc_result_algo_bytes(kmx_assoc_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  return R->n_rows * R->row_bytes + (u64)R->h_tot[0] * (R->row_bytes + sizeof(AssocRec)) + 4ull * R->n_cols * R->n_vec;
}
extern "C" void kmx_assoc_result_free(kmx_assoc_result* R) { mat_free(R); }
