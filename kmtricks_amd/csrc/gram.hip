// gram.hip -- `kmx pca` on the device: the recurrence-weighted co-presence table of a matrix's samples (include/kmx.h, section "gram";
// the integer part of the EIGENSTRAT / smartpca Gram matrix).  T[i][j] = the sum over the rows that hold listed samples i and j of
// weights[rec]: dist.hip's shared table with a weight a row.  A weight a row breaks the popcount; a weight a 64-row WORD does not: the
// rows are put in recurrence order, every class of a weight other than 0 starting on a word, and the pair kernel is k_dist_pairs with
// one multiply a word.  No reference counterpart in the kmtricks tree.  gfx950, wave64.
//
//   k_gram_score   k_pan_score's decomposition, the recurrence only: a wave a chunk of rows; a row of 64 units and more (a unit: a count,
//                  or a payload byte) is read by the whole wave, shorter rows by the L lanes of a sub-group.  The list is a byte a unit:
//                  COUNT 1 where the column is listed, PA the mask of the byte's listed columns (the padding bits of the last byte
//                  are not listed: masked at load).  Writes rec[row] and the class histogram (u32: a call has fewer than 2^32 rows), in
//                  LDS while M + 1 words fit GR_LDS_WORDS, flushed once a workgroup.
//   k_gram_fold    one workgroup: the exclusive scan of ceil(n_R / 64) over the classes of a weight other than 0 -- the first WORD of
//                  every class; cursor[R] = 64 x that, the class's next free place; meta[0] = Wu, the words the order takes.
//   k_gram_order   k_pan_order's scatter, row -> place: a wave loops over its distinct classes (ballot, one atomic a class).  Rows of
//                  a class of weight 0 get no place.  The places a class leaves free in its last word stay GR_NONE (cleared before).
//   k_gram_slab    dist's sample-major bit slab in PLACE order: a wave a tile of one word x 64 columns (COUNT) or 64 payload bytes (PA);
//                  lane r holds the row of place 64 w + r, the wave reads the 64 rows one after the other through it.  Every row taken
//                  from the order is tested (row < n_rows) before it becomes an address; a free place is a zero bit; so is an unlisted
//                  column.  The tile of column block 0 also writes the word's weight, ww[w] = weights[rec[row of place 64 w]] (a class
//                  fills its words from the first place on; rec tested <= M).
//   k_gram_pairs   k_dist_pairs' panels and 16 x 16 thread tiling; popcount(a & b) into u32 sums while the word's weight stays the
//                  same, folded into u64 accumulators (sum x weight) when it changes -- almost never inside a panel -- and at the run's
//                  end; the flush is dist's.  It strides over (block pair, run) items: any grid is a correct one.
// No kernel waits on another workgroup.  Every load of a body byte is inside [rows, rows + n_rows * row_bytes): an address is rows +
// r * row_bytes + skip + b with r < n_rows and b + (bytes loaded) <= row_bytes - skip, both tested by the lane that loads; nothing is
// loaded in wider pieces than the piece that is tested and nothing is rounded to an aligned address.  The launch knobs of this file are
// its own: KMX_GRAM_CUS and KMX_GRAM_GRID.
#include "matrix_host.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 GR_NONE = 0xFFFFFFFFu;      // a free place of the order (n_rows <= 2^32 - 256: no row has this number)
constexpr u32 GR_LDS_WORDS = 12288;       // 48 KB: the class histogram lives in LDS while M + 1 <= this
constexpr u32 GR_WGS_PER_CU = 8;          // k_gram_score's persistent grid, and the workgroups k_gram_pairs' runs aim at: a CU
constexpr u32 GR_MAX_GRID = 1u << 16;     // workgroups of a launch: the kernels stride over their work
constexpr u32 GR_WAVES_PER_SIMD = 8;      // chunks of long rows are made small enough for this many waves a SIMD
constexpr u32 GP_CH = 32;                 // slab words (64 places each) of a panel in LDS: 2 x 16 KB
constexpr u64 GP_RUN_MIN = 64;            // words of the shortest run a workgroup of k_gram_pairs takes (4096 places) ...
constexpr u64 GP_RUN_MAX = 1ull << 24;    // ... and of the longest: see k_gram_pairs

static_assert(sizeof(kmx_gram_task) == 64, "kmx_gram_task is 64 bytes");

// lst: a byte a unit -- COUNT: 1 where the column is listed; PA: the listed columns of the payload byte.
// L: lanes of a row (a power of two <= 64); RW: rows of a wave's chunk (64 when L < 64; a power of two <= 64 when L == 64).
// hist: the call's class histogram [M + 1], zeroed.  Dynamic LDS: M + 1 words when use_lds.
template <bool COUNT>
__global__ __launch_bounds__(256)
void k_gram_score(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 M, u32 L, u32 RW, const u8* __restrict__ lst,
                  u32 a, u32 use_lds, u32* __restrict__ hist, u32* __restrict__ recv)
{
  extern __shared__ u32 s_hist[];
  const u32 lane = threadIdx.x & 63u, u = lane & (L - 1u), sub = lane / L;
  const u32 units = COUNT ? N : (u32)(((u64)N + 7) / 8);
  const u32 passes = L == 64 ? RW : L;
  const u64 n_chunks = ((u64)n_rows + RW - 1) / RW;
  if (use_lds) {
    for (u32 i = threadIdx.x; i < M + 1; i += 256) s_hist[i] = 0;
    __syncthreads();
  }
  for (u64 g = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; g < n_chunks; g += (u64)gridDim.x * 4) {
    const u64 row0 = g * RW;
    u32 rec = 0;
    for (u32 p = 0; p < passes; p++) {
      const u64 row = row0 + (u64)sub * L + p;
      u32 acc = 0;
      if (row < n_rows) {
        const u8* q = rows + row * row_bytes + skip;
        for (u64 un = u; un < units; un += L) {
          const u32 m = lst[un];
          if (COUNT) { if (m) acc += (u32)(reinterpret_cast<const UDword*>(q + 4 * un)->v >= a); }
          else if (m) acc += (u32)__popc((u32)q[un] & m);
        }
      }
      for (u32 o = L >> 1; o; o >>= 1) acc += __shfl_xor(acc, (int)o);
      if (u == p) rec = acc;
    }
    // lane i holds row row0 + i
    const u64 mine = row0 + lane;
    if (lane < RW && mine < n_rows) {
      if (rec > M) rec = M;      // (never: M columns are listed)
      recv[mine] = rec;
      if (use_lds) atomicAdd(&s_hist[rec], 1u); else atomicAdd(&hist[rec], 1u);
    }
  }
  if (use_lds) {
    __syncthreads();
    for (u32 i = threadIdx.x; i < M + 1; i += 256) { const u32 v = s_hist[i]; if (v) atomicAdd(&hist[i], v); }
  }
}

// one workgroup.  cursor[R]: the first place of class R (64 x its first word); meta[0]: the words of the order, at most w_max
__global__ __launch_bounds__(256)
void k_gram_fold(const u32* __restrict__ hist, const u32* __restrict__ wt, u32 M, u64 w_max, u64* __restrict__ cursor, u32* __restrict__ meta)
{
  __shared__ u32 s[256];
  const u32 tid = threadIdx.x;
  const u64 M1 = (u64)M + 1;
  u32 carry = 0;      // (words: at most 2^26 + 2^15)
  for (u64 t0 = 0; t0 < M1; t0 += 256) {
    const u64 i = t0 + tid;
    const u32 v = i < M1 && wt[i] ? (u32)(((u64)hist[i] + 63) / 64) : 0u;
    s[tid] = v;
    __syncthreads();
    for (u32 off = 1; off < 256; off <<= 1) {
      const u32 t = tid >= off ? s[tid - off] : 0u;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    if (i < M1) cursor[i] = 64ull * (carry + s[tid] - v);
    carry += s[255];
    __syncthreads();
  }
  if (tid == 0) meta[0] = (u32)min((u64)carry, w_max);      // (never more: the sum of ceil(n_R / 64) is at most n_rows / 64 + classes)
}

// a thread a row; cursor[r]: the next free place of class r, moved on here.  order: n_places entries, GR_NONE
__global__ __launch_bounds__(256)
void k_gram_order(const u32* __restrict__ recv, u32 n_rows, u32 M, const u32* __restrict__ wt, u64* __restrict__ cursor, u64 n_places,
                  u32* __restrict__ order)
{
  const u32 lane = threadIdx.x & 63u;
  const u64 n_tiles = ((u64)n_rows + 255) / 256;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 row = t * 256 + threadIdx.x;
    bool have = row < n_rows;
    u32 r = have ? recv[row] : 0u;
    if (r > M) r = M;      // (never: a recurrence is at most M; the cursor has M + 1 entries)
    have = have && wt[r] != 0;
    u64 todo = __ballot(have);
    while (todo) {      // (uniform over the wave)
      const int lead = __ffsll((long long)todo) - 1;
      const u32 rl = (u32)__shfl((int)r, lead);
      const bool in = have && r == rl;
      const u64 same = __ballot(in);
      u32 blo = 0, bhi = 0;
      if ((int)lane == lead) {
        const u64 b = atomicAdd(reinterpret_cast<unsigned long long*>(&cursor[rl]), (unsigned long long)__popcll(same));
        blo = (u32)b; bhi = (u32)(b >> 32);
      }
      blo = (u32)__shfl((int)blo, lead); bhi = (u32)__shfl((int)bhi, lead);
      if (in) {
        const u64 at = ((u64)blo | ((u64)bhi << 32)) + (u32)__popcll(same & ((1ULL << lane) - 1ULL));
        if (at < n_places) order[at] = (u32)row;
      }
      todo &= ~same;
    }
  }
}

// tile t: word t / ct_n of the order, column block (COUNT) or block of 64 payload bytes (PA) t % ct_n.  W: the words the slab, the
// order and ww are laid out for (the host's bound); meta[0] <= W of them are in use.
template <bool COUNT>
__global__ __launch_bounds__(256)
void k_gram_slab(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 NB, u32 M, u64 W, u32 ct_n, const u8* __restrict__ lst,
                 u32 a, const u32* __restrict__ order, const u32* __restrict__ recv, const u32* __restrict__ wt, const u32* __restrict__ meta,
                 u64* __restrict__ slab, u32* __restrict__ ww)
{
  const u32 lane = threadIdx.x & 63u;
  const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (u64)gridDim.x * 4;
  const u64 n_tiles = min((u64)meta[0], W) * ct_n;
  for (u64 t = wave; t < n_tiles; t += n_waves) {
    const u64 w = t / ct_n;
    const u32 ct = (u32)(t % ct_n);
    u32 mine = order[w * 64 + lane];      // (w < W: the order has 64 W entries)
    if (mine >= n_rows) mine = GR_NONE;   // a free place; never a row that is not there
    if (ct == 0 && lane == 0) {
      const u32 r = mine != GR_NONE ? recv[mine] : 0u;
      ww[w] = mine != GR_NONE && r <= M ? wt[r] : 0u;
    }
    const u64 live = __ballot(mine != GR_NONE);
    const u32 nr = live ? 64u - (u32)__clzll((long long)live) : 0u;      // places behind the last row of the word are free
    if (COUNT) {      // a tile: 64 places x the 64 columns of block ct
      const u32 c = ct * 64 + lane;
      u32 lo = 0, hi = 0;
      const bool ok = c < N && lst[c];
      const u8* p = rows + skip + 4ull * c;
      for (u32 r = 0; r < nr; r++) {      // (every lane of the wave goes round: place r is read from lane r)
        const u32 row = (u32)__builtin_amdgcn_readlane((int)mine, (int)r);
        u32 bit = 0;
        if (ok && row != GR_NONE) bit = (u32)(reinterpret_cast<const UDword*>(p + (u64)row * row_bytes)->v >= a);
        if (r < 32) lo |= bit << r; else hi |= bit << (r - 32);
      }
      slab[((u64)ct * W + w) * 64 + lane] = (u64)lo | ((u64)hi << 32);
    } else {          // a tile: 64 places x 64 payload bytes (the 8 column blocks from 8 ct on)
      const u32 nb = (N + 7) / 8, bi = ct * 64 + lane;
      const u32 m = bi < nb ? (u32)lst[bi] : 0u;      // the listed columns of the byte: no padding bit is
      u32 lo[8], hi[8];
#pragma unroll
      for (int j = 0; j < 8; j++) { lo[j] = 0; hi[j] = 0; }
      const u8* p = rows + skip + bi;
      for (u32 r = 0; r < nr; r++) {      // (every lane of the wave goes round: place r is read from lane r)
        const u32 row = (u32)__builtin_amdgcn_readlane((int)mine, (int)r);
        u32 x = 0;
        if (m && row != GR_NONE) x = (u32)p[(u64)row * row_bytes] & m;
        if (r < 32) {
#pragma unroll
          for (int j = 0; j < 8; j++) lo[j] |= ((x >> j) & 1u) << r;
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) hi[j] |= ((x >> j) & 1u) << (r - 32);
        }
      }
      const u32 cb = ct * 8 + (lane >> 3);      // the lane's 8 columns are samples 8 (lane & 7) ... + 7 of block cb
      if (cb < NB) {
        uint4* q = reinterpret_cast<uint4*>(slab + ((u64)cb * W + w) * 64 + 8 * (lane & 7u));
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = make_uint4(lo[2 * j], hi[2 * j], lo[2 * j + 1], hi[2 * j + 1]);
      }
    }
  }
}

// block pair bp of the upper triangle, rows first: (0,0) (0,1) ... (0,NB-1) (1,1) ...
__device__ __forceinline__ void gram_pair_of(u64 bp, u32 NB, u32& I, u32& J)
{
  u32 i = 0;
  while (i + 1 < NB && bp >= NB - i) { bp -= NB - i; i++; }
  I = i; J = i + (u32)min(bp, (u64)(NB - 1 - i));
}

// item it: block pair it / runs, run it % runs of run_words words.  No overflow: a run is at most GP_RUN_MAX = 2^24 words of 64 places, so
// a popcount sum is at most 2^30; times a weight below 2^32 that is below 2^62, and a thread folds a sum once a change of weight and
// once at the run's end.  The u64 accumulators and the table's cells are sums modulo 2^64 (include/kmx.h: the caller keeps the sum of
// the weights of all rows below 2^64).
__global__ __launch_bounds__(256)
void k_gram_pairs(const u64* __restrict__ slab, const u32* __restrict__ ww, const u32* __restrict__ meta, u64 W, u32 N, u32 NB, u32 runs,
                  u64 run_words, u64 n_items, u64* __restrict__ table)
{
  __shared__ uint4 A[GP_CH * 32];      // [word][64 samples] u64
  __shared__ uint4 B[GP_CH * 32];
  __shared__ u32 s_w[GP_CH];
  const u64 wu = min((u64)meta[0], W);
  const u32 tid = threadIdx.x, ti = tid >> 4, tj = tid & 15u;
  for (u64 it = blockIdx.x; it < n_items; it += gridDim.x) {      // (uniform over the workgroup)
    u32 I, J;
    gram_pair_of(it / runs, NB, I, J);
    const u64 w0 = (it % runs) * run_words, w1 = min(wu, w0 + run_words);
    if (w0 >= w1) continue;
    const bool diag = I == J;
    u64 acc[4][4];
    u32 pc[4][4];
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
      for (int y = 0; y < 4; y++) { acc[x][y] = 0; pc[x][y] = 0; }
    u32 cw = 0;      // the weight the sums in pc were taken under
    const uint4* Bp = diag ? A : B;
    for (u64 wc = w0; wc < w1; wc += GP_CH) {
      const u32 cn = (u32)min((u64)GP_CH, w1 - wc);
      const uint4* sa = reinterpret_cast<const uint4*>(slab + ((u64)I * W + wc) * 64);
      const uint4* sb = reinterpret_cast<const uint4*>(slab + ((u64)J * W + wc) * 64);
      __syncthreads();      // the chunk before this one has been read
      for (u32 i = tid; i < cn * 32; i += 256) {
        A[i] = sa[i];
        if (!diag) B[i] = sb[i];
      }
      if (tid < cn) s_w[tid] = ww[wc + tid];
      __syncthreads();
      for (u32 k = 0; k < cn; k++) {
        const u32 wk = s_w[k];
        if (wk != cw) {      // (uniform over the workgroup)
#pragma unroll
          for (int x = 0; x < 4; x++)
#pragma unroll
            for (int y = 0; y < 4; y++) { acc[x][y] += (u64)pc[x][y] * cw; pc[x][y] = 0; }
          cw = wk;
        }
        const uint4 a01 = A[k * 32 + ti * 2], a23 = A[k * 32 + ti * 2 + 1], b01 = Bp[k * 32 + tj * 2], b23 = Bp[k * 32 + tj * 2 + 1];
        const u64 a[4] = {(u64)a01.x | ((u64)a01.y << 32), (u64)a01.z | ((u64)a01.w << 32), (u64)a23.x | ((u64)a23.y << 32), (u64)a23.z | ((u64)a23.w << 32)};
        const u64 b[4] = {(u64)b01.x | ((u64)b01.y << 32), (u64)b01.z | ((u64)b01.w << 32), (u64)b23.x | ((u64)b23.y << 32), (u64)b23.z | ((u64)b23.w << 32)};
#pragma unroll
        for (int x = 0; x < 4; x++)
#pragma unroll
          for (int y = 0; y < 4; y++) pc[x][y] += (u32)__popcll(a[x] & b[y]);
      }
    }
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
      for (int y = 0; y < 4; y++) {
        const u64 v = acc[x][y] + (u64)pc[x][y] * cw;
        const u32 i = I * 64 + ti * 4 + x, j = J * 64 + tj * 4 + y;
        if (i < N && j < N && v) {
          atomicAdd(reinterpret_cast<unsigned long long*>(&table[(u64)i * N + j]), (unsigned long long)v);
          if (!diag) atomicAdd(reinterpret_cast<unsigned long long*>(&table[(u64)j * N + i]), (unsigned long long)v);
        }
      }
  }
}

static u32 gr_cus(const kmx_ctx* ctx) { return (u32)std::max(kmx_env_cus("KMX_GRAM_CUS", ctx), 1); }
static u32 gr_grid(u64 dflt) { return kmx_env_grid("KMX_GRAM_GRID", dflt); }
// runs per block pair (dist's rule): enough workgroups to fill the chip, no run below GP_RUN_MIN words or above GP_RUN_MAX, a run a
// multiple of a panel
static void gr_runs(u64 words, u64 pairs, u32 cus, u32* runs, u64* run_len)
{
  u64 r = std::max<u64>(1, (u64)cus * GR_WGS_PER_CU / pairs);
  r = std::min(r, (words + GP_RUN_MIN - 1) / GP_RUN_MIN);
  r = std::max<u64>(std::max<u64>(r, (words + GP_RUN_MAX - 1) / GP_RUN_MAX), 1);
  u64 len = (words + r - 1) / r;
  len = (len + GP_CH - 1) / GP_CH * GP_CH;
  *run_len = len;
  *runs = (u32)((words + len - 1) / len);
}

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
struct kmx_gram_result : MatResult {
  u64* d_table = nullptr;
  u32* h_par = nullptr;                 // page-locked: [0] the words of the order on their way down; the weights and the list on their way up
};

static int gram_check(kmx_ctx* ctx, const kmx_gram_task* T, const char* who, u64* row_bytes)
{
  const MatCheck c{ctx, who};
  const u32 N = T->n_cols, M = T->n_use;
  int rc;
  if ((rc = c.n_cols(N, M, "list")) || (rc = c.no_bloom(T->mode, ": a Bloom row is a hash bit, its recurrence is not a k-mer's")) || (rc = c.mode(T->mode)) ||
      (rc = c.key_words(T->key_words)) || (rc = c.min_abund(T->min_abund, T->mode)) || (rc = c.flags(T->flags, 0))) return rc;
  if (!T->weights) return c.no(KMX_E_INVAL, ": null weights");
  if ((rc = c.list_fits(M, N, "listed")) || (rc = c.identity(T->cols, M, N, "n_use"))) return rc;
  *row_bytes = MatCheck::row_bytes(T->key_words, T->mode, N);
  if ((rc = c.row_fits(*row_bytes))) return rc;
  if (N > 32768) return c.no(KMX_E_UNSUPPORTED, ": more than 32768 samples (a table would be 8 GiB and more)");
  if ((rc = c.n_rows(T->n_rows)) || (rc = c.rows(T->n_rows, T->rows))) return rc;
  return c.col_list(T->cols, M, N);
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int gram_queue(kmx_ctx* ctx, const kmx_gram_task* T, kmx_gram_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, M = T->n_use, NB = (N + 63) / 64, skip = 8 * T->key_words, n_rows = (u32)R->n_rows;
  const bool count = T->mode == KMX_MODE_COUNT;
  const u32 units = count ? N : (u32)(((u64)N + 7) / 8);
  const u64 M1 = (u64)M + 1, table = (u64)N * N, pairs = (u64)NB * (NB + 1) / 2;
  const u64 W = (u64)n_rows / 64 + std::min<u64>(M1, n_rows);      // the words of the order at the most
  // page-locked: word 0 comes back (the words in use), then the weights, then the list a byte a unit
  const u64 par_words = 1 + M1 + (units + 3) / 4;
  if (!(R->h_par = (u32*)R->pin(4 * par_words))) return ctx->fail(KMX_E_NOMEM, "kmx_gram: host allocation failed");
  R->h_par[0] = 0;
  memcpy(R->h_par + 1, T->weights, 4 * M1);
  u8* h_lst = reinterpret_cast<u8*>(R->h_par + 1 + M1);
  memset(h_lst, 0, 4 * ((units + 3) / 4));
  for (u32 j = 0; j < M; j++) {
    const u32 c = T->cols ? T->cols[j] : j;
    if (count) h_lst[c] = 1; else h_lst[c >> 3] |= (u8)(1u << (c & 7));
  }
  // a table of the call's own starts at zero; one the caller handed in is on neither list
  const bool own = !T->table;
  u32* d_par = (u32*)R->tmp(4 * par_words);
  R->d_table = own ? (u64*)R->keep(8 * table) : (u64*)T->table;
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_gram: device allocation failed");
  u64 *d_cursor = nullptr, *d_slab = nullptr;
  u32 *d_hist = nullptr, *d_meta = nullptr, *d_recv = nullptr, *d_order = nullptr, *d_ww = nullptr;
  if (n_rows) {
    d_hist = (u32*)R->tmp(4 * M1);
    d_cursor = (u64*)R->tmp(8 * M1);
    d_meta = (u32*)R->tmp(16);
    d_recv = (u32*)R->tmp(4ull * n_rows);
    d_order = (u32*)R->tmp(4 * 64 * W);
    d_ww = (u32*)R->tmp(4 * W);
    d_slab = (u64*)R->tmp(8 * 64 * NB * W);
    if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_gram: device allocation failed (send the body in runs of rows)");
  }
  const u32* d_wt = d_par + 1;
  const u8* d_lst = reinterpret_cast<const u8*>(d_par + 1 + M1);
  KMX_HIP(ctx, hipMemcpyAsync(d_par, R->h_par, 4 * par_words, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R, 5);      // ev: start, behind score + fold, behind the order, behind the slab, end
  if (rc != KMX_OK) return rc;
  if (own) KMX_HIP(ctx, hipMemsetAsync(R->d_table, 0, 8 * table, st));
  const u32 cus = gr_cus(ctx);
  const u32 cap = gr_grid(GR_MAX_GRID);
  if (n_rows) {
    KMX_HIP(ctx, hipMemsetAsync(d_hist, 0, 4 * M1, st));
    KMX_HIP(ctx, hipMemsetAsync(d_order, 0xFF, 4 * 64 * W, st));
    // rows of 64 units and more get a wave each; their chunks shrink until the chip has GR_WAVES_PER_SIMD waves a SIMD to hide the loads
    const RowPlan p = mat_row_plan(units, n_rows, cus, GR_WAVES_PER_SIMD);
    const u32 grid = (u32)std::min<u64>((p.chunks + 3) / 4, std::min<u64>((u64)cus * GR_WGS_PER_CU, cap));
    const u32 use_lds = M1 <= GR_LDS_WORDS;
    const size_t lds = use_lds ? (size_t)(4 * M1) : 0;
    if (count) hipLaunchKernelGGL(k_gram_score<true>, dim3(grid), dim3(256), lds, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, p.L, p.RW, d_lst,
                                  T->min_abund, use_lds, d_hist, d_recv);
    else hipLaunchKernelGGL(k_gram_score<false>, dim3(grid), dim3(256), lds, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, p.L, p.RW, d_lst,
                            T->min_abund, use_lds, d_hist, d_recv);
    KMX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_gram_fold, dim3(1), dim3(256), 0, st, (const u32*)d_hist, d_wt, M, W, d_cursor, d_meta);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[1], st));
  if (n_rows) {
    const u64 tiles = ((u64)n_rows + 255) / 256;
    hipLaunchKernelGGL(k_gram_order, dim3((u32)std::min<u64>(tiles, cap)), dim3(256), 0, st, (const u32*)d_recv, n_rows, M, d_wt, d_cursor, 64 * W, d_order);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[2], st));
  if (n_rows) {
    const u32 ct_n = count ? NB : (NB + 7) / 8;
    const u64 n_tiles = W * ct_n;
    const u32 grid = (u32)std::min<u64>((n_tiles + 3) / 4, cap);
    if (count) hipLaunchKernelGGL(k_gram_slab<true>, dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, NB, M, W, ct_n, d_lst, T->min_abund,
                                  (const u32*)d_order, (const u32*)d_recv, d_wt, (const u32*)d_meta, d_slab, d_ww);
    else hipLaunchKernelGGL(k_gram_slab<false>, dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, NB, M, W, ct_n, d_lst, T->min_abund,
                            (const u32*)d_order, (const u32*)d_recv, d_wt, (const u32*)d_meta, d_slab, d_ww);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[3], st));
  if (n_rows) {
    u32 runs = 1; u64 run_len = GP_CH;
    gr_runs(W, pairs, cus, &runs, &run_len);
    const u64 items = pairs * runs;
    hipLaunchKernelGGL(k_gram_pairs, dim3((u32)std::min<u64>(items, cap)), dim3(256), 0, st, (const u64*)d_slab, (const u32*)d_ww, (const u32*)d_meta, W, N, NB,
                       runs, run_len, items, R->d_table);
    KMX_HIP(ctx, hipGetLastError());
    KMX_HIP(ctx, hipMemcpyAsync(R->h_par, d_meta, 4, hipMemcpyDeviceToHost, st));      // (for algo_bytes; nothing on the device waits for it)
  }
  return mat_queue_tail(R);
}

extern "C" int kmx_gram_dev(kmx_ctx* ctx, const kmx_gram_task* task, kmx_gram_result** out)
{ return mat_call(ctx, task, out, false, "kmx_gram_dev", "kmx_gram", gram_check, gram_queue); }
extern "C" int kmx_gram_host(kmx_ctx* ctx, const kmx_gram_task* task, kmx_gram_result** out)
{ return mat_call(ctx, task, out, true, "kmx_gram_host", "kmx_gram", gram_check, gram_queue); }

extern "C" int kmx_gram_result_wait(kmx_gram_result* R) { return mat_wait(R); }
extern "C" uint64_t* kmx_gram_result_table_dev(kmx_gram_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_table : nullptr; }
extern "C" int kmx_gram_result_copy_table(kmx_gram_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_table, (u64)R->n_cols * R->n_cols, 8) : KMX_E_INVAL; }
extern "C" double kmx_gram_result_kernel_ms(kmx_gram_result* R) { return mat_kernel_ms(R); }
extern "C" int kmx_gram_result_kernel_parts_ms(kmx_gram_result* R, double* score_ms, double* order_ms, double* slab_ms, double* pairs_ms)
{ return mat_kernel_parts_ms(R, {score_ms, order_ms, slab_ms, pairs_ms}); }
extern "C" uint64_t kmx_gram_result_algo_bytes(kmx_gram_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  const u64 NB = ((u64)R->n_cols + 63) / 64, wu = R->n_rows ? R->h_par[0] : 0;
  return 2 * R->n_rows * R->row_bytes + 16ull * R->n_rows + 2 * 8 * 64 * NB * wu + 8ull * R->n_cols * R->n_cols;
}
extern "C" void kmx_gram_result_free(kmx_gram_result* R) { mat_free(R); }
