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
#include "kmx_host.hpp"

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
struct __attribute__((packed, aligned(1))) ADword { u32 v; };      // a dword at any address: one global_load_dword

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
            if (m && r0 + k < nr) x[k] = reinterpret_cast<const ADword*>(p + (u64)(r0 + k) * row_bytes)->v;
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
// KMX_ASSOC_CUS=c: the CU count the launches plan for, 1 <= c <= the device's (it may only lower the count)
static u32 as_cus(int n_cu)
{
  const long c = kmx_env_int("KMX_ASSOC_CUS"), n = std::max(n_cu, 1);
  return (u32)(c >= 1 && c <= n ? c : n);
}
// KMX_ASSOC_GRID=g: the cap on the workgroups of a launch (every kernel here strides over its work), 1 <= g <= the built-in cap
static u32 as_grid(u64 dflt)
{
  const long g = kmx_env_int("KMX_ASSOC_GRID");
  return (u32)(g >= 1 && (u64)g <= dflt ? (u64)g : dflt);
}

}  // namespace kmx

using namespace kmx;

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
struct kmx_assoc_result {
  kmx_ctx* ctx = nullptr;
  u32 n_rows = 0, n_cols = 0, n_vec = 0;
  u64 row_bytes = 0;
  u32 *d_keep = nullptr, *d_tiles = nullptr;
  AssocRec *d_recs_all = nullptr, *d_recs = nullptr;
  u8 *d_par = nullptr, *d_out = nullptr;
  u8* h_par = nullptr;                  // page-locked: the call's scalars, the biased vector table, the list a byte a unit, on their way up
  u32* h_tot = nullptr;                 // page-locked: kept rows
  void* d_in = nullptr;                 // kmx_assoc_host: the upload
  hipEvent_t ev_in = nullptr, ev_done = nullptr, ev0 = nullptr, ev1 = nullptr;
  bool waited = false; int status = KMX_OK;
};

static int assoc_check(kmx_ctx* ctx, const kmx_assoc_task* T, const char* who, u64* row_bytes)
{
  const std::string w(who);
  const u32 N = T->n_cols, M = T->n_use, V = T->n_vec;
  if (N == 0 || M == 0) return ctx->fail(KMX_E_INVAL, w + ": a matrix has at least one column, and so has the list");
  if (T->mode == KMX_MODE_BF || T->mode == KMX_MODE_BFC || T->mode == KMX_MODE_BFT)
    return ctx->fail(KMX_E_UNSUPPORTED, w + ": Bloom filter bodies are not supported: a Bloom row is a hash bit, its presence pattern is not a k-mer's (KMX_MODE_COUNT and KMX_MODE_PA only)");
  if (T->mode != KMX_MODE_COUNT && T->mode != KMX_MODE_PA) return ctx->fail(KMX_E_INVAL, w + ": mode must be KMX_MODE_COUNT or KMX_MODE_PA");
  if (T->key_words < 1 || T->key_words > 4) return ctx->fail(KMX_E_INVAL, w + ": key_words must be 1 ... 4");
  if (T->min_abund == 0) return ctx->fail(KMX_E_INVAL, w + ": min_abund must be at least 1");
  if (T->min_abund > 1 && T->mode == KMX_MODE_PA) return ctx->fail(KMX_E_INVAL, w + ": min_abund above 1 needs counts");
  if (T->flags) return ctx->fail(KMX_E_INVAL, w + ": unknown flag bits");
  if (V == 0 || V > 32) return ctx->fail(KMX_E_INVAL, w + ": n_vec must be 1 ... 32");
  if (!T->vecs) return ctx->fail(KMX_E_INVAL, w + ": null vecs");
  if (T->frac_bits > 62) return ctx->fail(KMX_E_INVAL, w + ": frac_bits must be 0 ... 62");
  if (!std::isfinite(T->gain) || !(T->gain > 0.0)) return ctx->fail(KMX_E_INVAL, w + ": the gain is a finite number above 0");
  if (std::isnan(T->vmin) || T->vmin < 0.0) return ctx->fail(KMX_E_INVAL, w + ": vmin is a number at or above 0");
  if (std::isnan(T->threshold) || T->threshold < 0.0) return ctx->fail(KMX_E_INVAL, w + ": the threshold is a number at or above 0");
  if (M > N) return ctx->fail(KMX_E_INVAL, w + ": more listed columns than input columns");
  if (!T->cols && M != N) return ctx->fail(KMX_E_INVAL, w + ": cols = NULL is the identity and needs n_use = n_cols");
  *row_bytes = 8ull * T->key_words + (T->mode == KMX_MODE_COUNT ? 4ull * N : ((u64)N + 7) / 8);
  if (*row_bytes > 0xFFFFFFFFull) return ctx->fail(KMX_E_UNSUPPORTED, w + ": rows of 4 GiB and more");
  if (T->n_rows > 0xFFFFFF00ull) return ctx->fail(KMX_E_UNSUPPORTED, w + ": more than 2^32 - 256 rows in one call (send the body in runs of rows)");
  if (T->n_rows && !T->rows) return ctx->fail(KMX_E_INVAL, w + ": null rows");
  if (T->cols) {
    std::vector<u32> s(T->cols, T->cols + M);
    std::sort(s.begin(), s.end());
    if (s.back() >= N) return ctx->fail(KMX_E_INVAL, w + ": a column index at or above n_cols");
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) return ctx->fail(KMX_E_INVAL, w + ": a column is listed twice");
  }
  // (double)s_j must be exact whichever samples are present: the sum of a vector's magnitudes stays below 2^53
  for (u32 j = 0; j < V; j++) {
    u64 sum = 0;      // (M < 2^32 entries below 2^31 + 1: no wrap)
    for (u64 m = 0; m < M; m++) { const i64 e = T->vecs[m * V + j]; sum += (u64)(e < 0 ? -e : e); }
    if (sum >= (1ull << 53)) return ctx->fail(KMX_E_INVAL, w + ": the magnitudes of vector " + std::to_string(j) + " sum to 2^53 or more: its sums would not be exact in a double");
  }
  return KMX_OK;
}

static void assoc_release(kmx_assoc_result* R)
{
  kmx_ctx* c = R->ctx;
  void* blocks[] = {R->d_keep, R->d_tiles, R->d_recs_all, R->d_recs, R->d_par, R->d_out, R->d_in};
  for (void* p : blocks) c->dfree(p);
  c->hfree(R->h_par); c->hfree(R->h_tot);
  for (hipEvent_t e : {R->ev_in, R->ev_done, R->ev0, R->ev1}) if (e) (void)hipEventDestroy(e);
  delete R;
}

template <bool COUNT, int VP>
static void assoc_launch_score(u32 grid, hipStream_t st, const kmx_assoc_task* T, const kmx_assoc_result* R, u32 skip, const u8* d_lst, const u32* d_vt, const AssocPrm* prm)
{
  hipLaunchKernelGGL((k_assoc_score<COUNT, VP>), dim3(grid), dim3(64), 0, st, (const u8*)T->rows, R->n_rows, R->row_bytes, skip, T->n_cols, d_lst, d_vt,
                     T->min_abund, prm, R->d_keep, R->d_recs_all, R->d_tiles);
}
template <bool COUNT>
static void assoc_launch_vp(u32 VP, u32 grid, hipStream_t st, const kmx_assoc_task* T, const kmx_assoc_result* R, u32 skip, const u8* d_lst, const u32* d_vt, const AssocPrm* prm)
{
  switch (VP) {
    case 1: assoc_launch_score<COUNT, 1>(grid, st, T, R, skip, d_lst, d_vt, prm); break;
    case 2: assoc_launch_score<COUNT, 2>(grid, st, T, R, skip, d_lst, d_vt, prm); break;
    case 4: assoc_launch_score<COUNT, 4>(grid, st, T, R, skip, d_lst, d_vt, prm); break;
    case 8: assoc_launch_score<COUNT, 8>(grid, st, T, R, skip, d_lst, d_vt, prm); break;
    case 12: assoc_launch_score<COUNT, 12>(grid, st, T, R, skip, d_lst, d_vt, prm); break;
    case 16: assoc_launch_score<COUNT, 16>(grid, st, T, R, skip, d_lst, d_vt, prm); break;
    case 24: assoc_launch_score<COUNT, 24>(grid, st, T, R, skip, d_lst, d_vt, prm); break;
    default: assoc_launch_score<COUNT, 32>(grid, st, T, R, skip, d_lst, d_vt, prm); break;
  }
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int assoc_queue(kmx_ctx* ctx, const kmx_assoc_task* T, kmx_assoc_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, M = T->n_use, V = T->n_vec, VP = as_vp(V), skip = 8 * T->key_words, n_rows = R->n_rows, tiles = filter_tiles(n_rows);
  const bool count = T->mode == KMX_MODE_COUNT;
  const u32 units = count ? N : (u32)(((u64)N + 7) / 8);
  const u64 NR = ((u64)N + 7) / 8 * 8;      // the table's rows: PA walks whole payload bytes
  const u64 vt_bytes = 4 * NR * VP, par_bytes = sizeof(AssocPrm) + vt_bytes + units;      // the scalars, the table, the list
  if (!(R->h_tot = (u32*)ctx->halloc(64)) || !(R->h_par = (u8*)ctx->halloc(par_bytes))) return ctx->fail(KMX_E_NOMEM, "kmx_assoc: host allocation failed");
  R->h_tot[0] = 0;
  AssocPrm* h_prm = reinterpret_cast<AssocPrm*>(R->h_par);
  u32* h_vt = reinterpret_cast<u32*>(R->h_par + sizeof(AssocPrm));
  u8* h_lst = R->h_par + sizeof(AssocPrm) + vt_bytes;
  h_prm->sc = std::ldexp(1.0, -(int)T->frac_bits); h_prm->gain = T->gain; h_prm->vmin = T->vmin; h_prm->thr = T->threshold;
  h_prm->min_rec = T->min_rec; h_prm->max_rec = T->max_rec;
  for (u64 i = 0; i < NR * VP; i++) h_vt[i] = 0x80000000u;      // the value 0
  memset(h_lst, 0, units);
  for (u32 m = 0; m < M; m++) {
    const u32 c = T->cols ? T->cols[m] : m;
    for (u32 j = 0; j < V; j++) h_vt[(u64)c * VP + j] = (u32)T->vecs[(u64)m * V + j] ^ 0x80000000u;
    if (count) h_lst[c] = 1; else h_lst[c >> 3] |= (u8)(1u << (c & 7));
  }
  R->d_keep = (u32*)ctx->dalloc(4ull * n_rows);
  R->d_tiles = (u32*)ctx->dalloc(4ull * ((u64)tiles + 1));
  R->d_recs_all = (AssocRec*)ctx->dalloc(sizeof(AssocRec) * (u64)n_rows);
  R->d_recs = (AssocRec*)ctx->dalloc(sizeof(AssocRec) * (u64)n_rows);      // every row kept
  R->d_out = (u8*)ctx->dalloc((u64)n_rows * R->row_bytes + 16);
  R->d_par = (u8*)ctx->dalloc(par_bytes);
  if (!R->d_keep || !R->d_tiles || !R->d_recs_all || !R->d_recs || !R->d_out || !R->d_par)
    return ctx->fail(KMX_E_NOMEM, "kmx_assoc: device allocation failed (send the body in runs of rows)");
  KMX_HIP(ctx, hipMemcpyAsync(R->d_par, R->h_par, par_bytes, hipMemcpyHostToDevice, st));
  if (ctx->profiling) {
    KMX_HIP(ctx, hipEventCreate(&R->ev0)); KMX_HIP(ctx, hipEventCreate(&R->ev1));
    KMX_HIP(ctx, hipEventRecord(R->ev0, st));
  }
  KMX_HIP(ctx, hipMemsetAsync(R->d_tiles, 0, 4ull * ((u64)tiles + 1), st));
  const u32 cap = as_grid(AS_MAX_GRID);
  if (n_rows) {
    const u64 groups = ((u64)n_rows + AS_GROUP - 1) / AS_GROUP;
    const u32 grid = (u32)std::min<u64>(groups, std::min<u64>((u64)as_cus(ctx->n_cu) * AS_WGS_PER_CU, cap));
    const AssocPrm* prm = reinterpret_cast<const AssocPrm*>(R->d_par);
    const u32* d_vt = reinterpret_cast<const u32*>(R->d_par + sizeof(AssocPrm));
    const u8* d_lst = R->d_par + sizeof(AssocPrm) + vt_bytes;
    if (count) assoc_launch_vp<true>(VP, grid, st, T, R, skip, d_lst, d_vt, prm);
    else assoc_launch_vp<false>(VP, grid, st, T, R, skip, d_lst, d_vt, prm);
    KMX_HIP(ctx, hipGetLastError());
  }
  KMX_HIP(ctx, launch_filter_scan(R->d_tiles, tiles, st));
  if (n_rows) {
    KMX_HIP(ctx, launch_filter_move((const u8*)T->rows, n_rows, R->row_bytes, R->row_bytes, R->d_keep, R->d_keep, R->d_tiles, R->d_out, st));
    hipLaunchKernelGGL(k_assoc_place, dim3(std::min(tiles, cap)), dim3(AS_TILE), 0, st, (const u32*)R->d_keep, (const AssocRec*)R->d_recs_all, n_rows,
                       (const u32*)R->d_tiles, R->d_recs);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev1, st));
  KMX_HIP(ctx, hipMemcpyAsync(&R->h_tot[0], R->d_tiles + tiles, 4, hipMemcpyDeviceToHost, st));
  KMX_HIP(ctx, hipEventCreateWithFlags(&R->ev_done, hipEventDisableTiming));
  KMX_HIP(ctx, hipEventRecord(R->ev_done, st));
  return KMX_OK;
}

static int assoc_call(kmx_ctx* ctx, const kmx_assoc_task* task, kmx_assoc_result** out, bool host, const char* who)
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, std::string(who) + ": null argument");
  *out = nullptr;
  u64 row_bytes = 0;
  int rc = assoc_check(ctx, task, who, &row_bytes);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  kmx_assoc_result* R = new kmx_assoc_result();
  R->ctx = ctx; R->n_rows = (u32)task->n_rows; R->row_bytes = row_bytes; R->n_cols = task->n_cols; R->n_vec = task->n_vec;
  kmx_assoc_task dt = *task;
  auto fail = [&](int code) { if (host) (void)hipStreamSynchronize(ctx->up); (void)hipStreamSynchronize(ctx->stream); assoc_release(R); return code; };
  const u64 bytes = task->n_rows * row_bytes;
  if (host && bytes) {
    if (!(R->d_in = ctx->dalloc(bytes))) return fail(ctx->fail(KMX_E_NOMEM, std::string(who) + ": upload allocation failed (send the body in runs of rows)"));
    hipError_t e = hipMemcpyAsync(R->d_in, task->rows, bytes, hipMemcpyHostToDevice, ctx->up);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&R->ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(R->ev_in, ctx->up);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, R->ev_in, 0);
    if (e != hipSuccess) return fail(ctx->fail(KMX_E_HIP, std::string(who) + ": upload: " + hipGetErrorString(e)));
    dt.rows = R->d_in;
  }
  if ((rc = assoc_queue(ctx, &dt, R)) != KMX_OK) return fail(rc);
  *out = R;
  return KMX_OK;
}

extern "C" int kmx_assoc_dev(kmx_ctx* ctx, const kmx_assoc_task* task, kmx_assoc_result** out) { return assoc_call(ctx, task, out, false, "kmx_assoc_dev"); }
extern "C" int kmx_assoc_host(kmx_ctx* ctx, const kmx_assoc_task* task, kmx_assoc_result** out) { return assoc_call(ctx, task, out, true, "kmx_assoc_host"); }

extern "C" int kmx_assoc_result_wait(kmx_assoc_result* R)
{
  if (!R) return KMX_E_INVAL;
  if (R->waited) return R->status;
  R->waited = true;
  const hipError_t e = hipEventSynchronize(R->ev_done);
  if (e != hipSuccess) return R->status = R->ctx->fail(KMX_E_HIP, std::string("kmx_assoc: ") + hipGetErrorString(e));
  // the call has run: the scratch and the upload go back to the pool; the kept rows and their records stay
  kmx_ctx* c = R->ctx;
  c->dfree(R->d_keep); R->d_keep = nullptr;
  c->dfree(R->d_recs_all); R->d_recs_all = nullptr;
  c->dfree(R->d_par); R->d_par = nullptr;
  c->dfree(R->d_in); R->d_in = nullptr;
  return R->status = KMX_OK;
}
extern "C" uint64_t kmx_assoc_result_rows(kmx_assoc_result* R) { return R && kmx_assoc_result_wait(R) == KMX_OK ? R->h_tot[0] : 0; }
extern "C" uint64_t kmx_assoc_result_row_bytes(const kmx_assoc_result* R) { return R ? R->row_bytes : 0; }
extern "C" uint64_t kmx_assoc_result_body_bytes(kmx_assoc_result* R) { return R ? kmx_assoc_result_rows(R) * R->row_bytes : 0; }
extern "C" const void* kmx_assoc_result_body_dev(kmx_assoc_result* R) { return R && kmx_assoc_result_wait(R) == KMX_OK ? R->d_out : nullptr; }
extern "C" const kmx_assoc_rec* kmx_assoc_result_recs_dev(kmx_assoc_result* R) { return R && kmx_assoc_result_wait(R) == KMX_OK ? (const kmx_assoc_rec*)R->d_recs : nullptr; }
static int assoc_copy_out(kmx_assoc_result* R, void* dst, uint64_t dst_bytes, const void* src, u64 bytes)
{
  if (dst_bytes < bytes) return R->ctx->fail(KMX_E_INVAL, "destination too small");
  if (!bytes) return KMX_OK;
  if (!dst) return R->ctx->fail(KMX_E_INVAL, "null destination");
  return kmx_copy_to_host(R->ctx, dst, src, bytes);
}
extern "C" int kmx_assoc_result_copy_body(kmx_assoc_result* R, void* host_dst, uint64_t dst_bytes)
{
  if (!R) return KMX_E_INVAL;
  const int rc = kmx_assoc_result_wait(R);
  return rc != KMX_OK ? rc : assoc_copy_out(R, host_dst, dst_bytes, R->d_out, kmx_assoc_result_body_bytes(R));
}
extern "C" int kmx_assoc_result_copy_recs(kmx_assoc_result* R, kmx_assoc_rec* host_dst, uint64_t dst_entries)
{
  if (!R) return KMX_E_INVAL;
  const int rc = kmx_assoc_result_wait(R);
  if (rc != KMX_OK) return rc;
  if (dst_entries < R->h_tot[0]) return R->ctx->fail(KMX_E_INVAL, "destination too small");
  return assoc_copy_out(R, host_dst, ~0ull, R->d_recs, sizeof(AssocRec) * (u64)R->h_tot[0]);
}
extern "C" double kmx_assoc_result_kernel_ms(kmx_assoc_result* R)
{
  if (!R || !R->ev0 || !R->ev1 || kmx_assoc_result_wait(R) != KMX_OK) return -1.0;
  float ms = 0;
  return hipEventElapsedTime(&ms, R->ev0, R->ev1) == hipSuccess ? (double)ms : -1.0;
}
extern "C" uint64_t kmx_assoc_result_algo_bytes(kmx_assoc_result* R)
{
  if (!R || kmx_assoc_result_wait(R) != KMX_OK) return 0;
  return (u64)R->n_rows * R->row_bytes + (u64)R->h_tot[0] * (R->row_bytes + sizeof(AssocRec)) + 4ull * R->n_cols * R->n_vec;
}
extern "C" void kmx_assoc_result_free(kmx_assoc_result* R)
{
  if (!R) return;
  (void)hipSetDevice(R->ctx->device);
  if (R->ev_done) (void)hipEventSynchronize(R->ev_done);
  assoc_release(R);
}
