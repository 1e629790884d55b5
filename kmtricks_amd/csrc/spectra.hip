// spectra.hip -- `kmx spectra` on the device: per listed sample the rows of a matrix by count, per pair of samples the rows by the two
// counts (include/kmx.h, section "spectra"; what KAT `hist` / `comp` and Merqury's spectra-cn tabulate).  No reference counterpart in
// the kmtricks tree.  gfx950, wave64.  Exact integer tallies; the tables are added to with 64-bit global atomics, so the caller's table
// is the only one there is (no call-local copy).
//
//   k_spectra_hist_count  HIST, COUNT.  A work item is a block of SP_BLOCK = 64 input columns and a run of rows; a workgroup (8 waves)
//                 strides over the items of a persistent grid.  A lane is a column: a wave reads 256 contiguous bytes of a row, the
//                 eight waves take the run's rows in turn, eight rows in flight each (32 KiB a CU with two workgroups).  Zeros --
//                 nearly every cell of a real matrix -- are counted in a register of the lane and added once an item, and so is the
//                 volume of the last bin (u64).  The bins 1 ... C1 are u32 in LDS, laid out [bin][column of the block]: a wave's 64
//                 increments fall into 64 different banks whatever the data (a run has fewer than 2^32 rows: no bin overflows).  They
//                 are flushed once an item, non-zero bins only, a wave's lanes on consecutive bins of one column so that its 64-bit
//                 adds fall on contiguous words of the table.  That holds while C1 <= SP_HIST_LDS_CAP = 255 (255 * 64 * 4 = 65 280
//                 bytes: two workgroups a CU of 160 KiB; a smaller C1 admits more, up to 8); beyond it, up to 65535, a non-zero count
//                 is one 64-bit global atomic on hist[j][bin].
//   k_spectra_hist_pa     HIST, PA.  The same items, in runs of SP_MIN_RUN_PA = 4096 rows at the least (a row gives a workgroup 64
//                 bytes); a lane is a payload byte with eight u32 registers of ones, which the eight waves add up in LDS; thread
//                 (bit, byte) then adds the run's rows - the ones to bin 0 and the ones to bin 1 -- with C1 = 1 to the volume too.
//                 No bins: a bit has two values.
//   k_spectra_joint       JOINT.  The pairs go in groups of G consecutive pairs, G = min(SP_GROUP = 16, SP_JOINT_LDS_WORDS / (C2 + 1)^2)
//                 while a pair's (C2 + 1)^2 u32 table fits SP_JOINT_LDS_WORDS = 12288 words (C2 <= SP_JOINT_LDS_CAP = 109); the group's
//                 tables live in LDS and are flushed once an item, non-zero cells only.  Beyond that C2 a group is 16 pairs and a cell is
//                 one 64-bit global atomic.  A work item is a group and a run of rows, taken in tiles; a thread takes (row of the tile,
//                 pair of the group).  THE ROAD, one for the call: with U the largest number of distinct columns of a group, the
//                 columns are GATHERED when SP_GATHER_FACTOR * 128 * U <= row_bytes (SP_GATHER_FACTOR = 2: a gathered count costs a
//                 128-byte line of its row, so the lines touched are at most half the row) -- a tile is 256 rows, a wave's lanes are 64
//                 consecutive rows of one pair and load the two counts straight from the body (L2 holds a line for the pairs that
//                 share a column); otherwise the rows are STREAMED: a tile is the floor(SP_STAGE_BYTES / row_bytes) rows (256 at the
//                 most) that fit 16 KiB of LDS, copied there as one contiguous piece of the body, dword a lane, and the counts are read
//                 from LDS.  (U <= 32, so streamed rows are shorter than 8 KiB: a tile has two rows and more.)
//                 THE HOT CELL: nearly every row of a real pair is (0, 0), and a body of equal rows has one cell too.  A wave takes
//                 the cell of its first active lane, ballots the lanes that have the same one and adds their number once; the other
//                 lanes add 1 each.  The result does not depend on what same-address LDS atomics cost.
// No kernel waits on another workgroup: any grid is a correct one.
// Every load of a body byte is inside [rows, rows + n_rows * row_bytes): an address is rows + r * row_bytes + skip + b with r < n_rows and
// b + (bytes loaded) <= row_bytes - skip, both tested by the lane that loads -- or, for a streamed tile, rows + t0 * row_bytes + b with
// t0 + nr <= n_rows and b + (bytes loaded) <= nr * row_bytes; nothing is loaded in wider pieces than the piece that is tested and nothing
// is rounded to an aligned address.  The launch knobs of this file are its own: KMX_SPECTRA_CUS and KMX_SPECTRA_GRID.
#include "matrix_host.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 SP_NONE = 0xFFFFFFFFu;        // the ordinal of a column that is not listed
constexpr u32 SP_BLOCK = 64;                // units of a row a workgroup of HIST takes: a lane a unit
constexpr u32 SP_HIST_LDS_CAP = 255;        // the largest C1 whose bins 1 ... C1 live in LDS: 255 * 64 words
constexpr u32 SP_HIST_WAVES = 8;            // waves of a HIST workgroup: they share the block's bins
constexpr u32 SP_HIST_ROWS = 8;             // rows a HIST wave has in flight
constexpr u32 SP_LDS_PER_CU = 160 * 1024;   // the persistent grids: as many workgroups a CU as their LDS admits, 2 at the least, 8 at the most
constexpr u32 SP_MIN_RUN = 256;             // rows of a work item, at the least (an item's flush is paid once a run)
constexpr u32 SP_MIN_RUN_PA = 4096;         // ... of k_spectra_hist_pa
constexpr u32 SP_MAX_GRID = 1u << 16;       // workgroups of a launch: the kernels stride over their work
constexpr u32 SP_GROUP = 16;                // pairs of a group, at the most
constexpr u32 SP_JOINT_LDS_WORDS = 12288;   // 48 KiB: a group's tables
constexpr u32 SP_JOINT_LDS_CAP = 109;       // the largest C2 whose table fits them: 110^2 = 12100
constexpr u32 SP_STAGE_BYTES = 16384;       // a streamed tile of rows in LDS
constexpr u32 SP_TILE = 256;                // rows of a tile, at the most: a thread a row of one pair
constexpr u32 SP_GATHER_FACTOR = 2;         // gather while SP_GATHER_FACTOR * 128 * U <= row_bytes

static_assert(sizeof(kmx_spectra_task) == 80, "kmx_spectra_task is 80 bytes");
static_assert(SP_HIST_LDS_CAP * SP_BLOCK * 4 <= 65536 && SP_JOINT_LDS_WORDS * 4 + SP_STAGE_BYTES <= 65536, "a workgroup's LDS is 64 KiB at the most");
static_assert((SP_JOINT_LDS_CAP + 1) * (SP_JOINT_LDS_CAP + 1) <= SP_JOINT_LDS_WORDS && (SP_JOINT_LDS_CAP + 2) * (SP_JOINT_LDS_CAP + 2) > SP_JOINT_LDS_WORDS, "SP_JOINT_LDS_CAP");

// work item w: run w / n_blocks of run_rows rows, column block w % n_blocks.  ordt: the ordinal of every input column, SP_NONE where it is
// not listed, 8 * ceil(N / 8) entries.  hist: u64 [M][C1 + 2].  Dynamic LDS: C1 * 64 words when LDS.
template <bool LDS>
__global__ __launch_bounds__(64 * SP_HIST_WAVES)
void k_spectra_hist_count(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 C1, const u32* __restrict__ ordt,
                          u32 n_blocks, u32 run_rows, u64 n_items, u64* __restrict__ hist)
{
  extern __shared__ u32 s_bins[];
  __shared__ u32 s_ord[SP_BLOCK];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u64 stride = (u64)C1 + 2;
  for (u64 w = blockIdx.x; w < n_items; w += gridDim.x) {
    const u64 col = (w % n_blocks) * SP_BLOCK + lane;
    const u64 r0 = (w / n_blocks) * run_rows, r1 = std::min<u64>(r0 + run_rows, n_rows);
    const u32 o = col < N ? ordt[col] : SP_NONE;
    __syncthreads();      // (the item before this one has been flushed)
    if (LDS) for (u32 i = tid; i < C1 * SP_BLOCK; i += 64 * SP_HIST_WAVES) s_bins[i] = 0;
    if (wave == 0) s_ord[lane] = o;
    __syncthreads();
    u32 zeros = 0; u64 tail = 0;
    if (o != SP_NONE) {
      const u8* q = rows + skip + 4 * col;      // (col < N: the count's four bytes end inside the row)
      u64* mine = hist + (u64)o * stride;
      for (u64 r = r0 + wave; r < r1; r += SP_HIST_WAVES * SP_HIST_ROWS) {
        u32 v[SP_HIST_ROWS];
#pragma unroll
        for (u32 k = 0; k < SP_HIST_ROWS; k++) { const u64 rr = r + SP_HIST_WAVES * k; v[k] = rr < r1 ? reinterpret_cast<const UDword*>(q + rr * row_bytes)->v : 0u; }
#pragma unroll
        for (u32 k = 0; k < SP_HIST_ROWS; k++) {
          if (r + SP_HIST_WAVES * k >= r1) continue;
          if (v[k] == 0) { zeros++; continue; }
          const u32 b = std::min(v[k], C1);
          if (v[k] >= C1) tail += v[k];
          if (LDS) atomicAdd(&s_bins[(b - 1) * SP_BLOCK + lane], 1u); else atomicAdd(&mine[b], 1ull);
        }
      }
      if (zeros) atomicAdd(&mine[0], (u64)zeros);
      if (tail) atomicAdd(&mine[stride - 1], tail);
    }
    if (LDS) {
      __syncthreads();
      // a wave's lanes take consecutive bins of one column: its adds fall on contiguous words of the table (the LDS reads conflict; they are few)
      for (u32 i = tid; i < C1 * SP_BLOCK; i += 64 * SP_HIST_WAVES) {
        const u32 c = i / C1, b = i - c * C1;
        const u32 n = s_bins[b * SP_BLOCK + c], oc = s_ord[c];
        if (n && oc != SP_NONE) atomicAdd(&hist[(u64)oc * stride + b + 1], (u64)n);
      }
    }
  }
}

// the same items; a lane a payload byte.  The waves' ones meet in LDS ([bit][byte of the block]) and leave once an item
__global__ __launch_bounds__(64 * SP_HIST_WAVES)
void k_spectra_hist_pa(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 C1, const u32* __restrict__ ordt,
                       u32 n_blocks, u32 run_rows, u64 n_items, u64* __restrict__ hist)
{
  __shared__ u32 s_ones[8 * SP_BLOCK];
  static_assert(8 * SP_BLOCK == 64 * SP_HIST_WAVES, "a thread a counter");
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u64 units = ((u64)N + 7) / 8, stride = (u64)C1 + 2;
  for (u64 w = blockIdx.x; w < n_items; w += gridDim.x) {
    const u64 un0 = (w % n_blocks) * SP_BLOCK, un = un0 + lane;
    const u64 r0 = (w / n_blocks) * run_rows, r1 = std::min<u64>(r0 + run_rows, n_rows);
    __syncthreads();      // (the item before this one has been flushed)
    s_ones[tid] = 0;
    __syncthreads();
    if (un < units) {
      const u8* q = rows + skip + un;
      u32 ones[8] = {};
      for (u64 r = r0 + wave; r < r1; r += SP_HIST_WAVES * SP_HIST_ROWS) {
        u32 x[SP_HIST_ROWS];
#pragma unroll
        for (u32 k = 0; k < SP_HIST_ROWS; k++) { const u64 rr = r + SP_HIST_WAVES * k; x[k] = rr < r1 ? (u32)q[rr * row_bytes] : 0u; }
#pragma unroll
        for (u32 k = 0; k < SP_HIST_ROWS; k++) {
#pragma unroll
          for (u32 b = 0; b < 8; b++) ones[b] += (x[k] >> b) & 1u;
        }
      }
#pragma unroll
      for (u32 b = 0; b < 8; b++) if (ones[b]) atomicAdd(&s_ones[b * SP_BLOCK + lane], ones[b]);
    }
    __syncthreads();
    // thread (bit, byte): column 8 * byte + bit
    const u64 mine = un0 + lane;
    const u32 o = mine < units ? ordt[8 * mine + wave] : SP_NONE;      // (ordt has 8 entries a payload byte; the padding bits are SP_NONE)
    if (o != SP_NONE) {
      const u32 n = s_ones[tid], z = (u32)(r1 - r0) - n;
      u64* line = hist + (u64)o * stride;
      if (z) atomicAdd(&line[0], (u64)z);
      if (n) { atomicAdd(&line[1], (u64)n); if (C1 == 1) atomicAdd(&line[2], (u64)n); }
    }
  }
}

// work item w: run w / n_groups of run_rows rows, pair group w % n_groups (pairs g * G ... ).  TR: rows of a tile.  joint: u64
// [P][C2 + 1][C2 + 1].  Dynamic LDS: G * (C2 + 1)^2 words when LDS, then SP_STAGE_BYTES bytes when STREAM.
template <bool COUNT, bool STREAM, bool LDS>
__global__ __launch_bounds__(256)
void k_spectra_joint(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 C2, const uint2* __restrict__ pairs, u32 P, u32 G,
                     u32 n_groups, u32 TR, u32 run_rows, u64 n_items, u64* __restrict__ joint)
{
  extern __shared__ u32 s_mem[];
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 W = C2 + 1, cells = W * W;
  u32* s_tab = s_mem;
  u32* s_stage = s_mem + (LDS ? G * cells : 0u);
  const u8* s_bytes = reinterpret_cast<const u8*>(s_stage);
  for (u64 w = blockIdx.x; w < n_items; w += gridDim.x) {
    const u32 p0 = (u32)(w % n_groups) * G, np = std::min(G, P - p0);
    const u64 r0 = (w / n_groups) * run_rows, r1 = std::min<u64>(r0 + run_rows, n_rows);
    u64* out = joint + (u64)p0 * cells;
    if (LDS) {
      __syncthreads();      // (the item before this one has been flushed)
      for (u32 i = tid; i < np * cells; i += 256) s_tab[i] = 0;
      __syncthreads();
    }
    for (u64 t0 = r0; t0 < r1; t0 += TR) {
      const u32 nr = (u32)std::min<u64>(TR, r1 - t0);
      if (STREAM) {
        const u64 nbytes = nr * row_bytes;
        if (nbytes > SP_STAGE_BYTES) break;      // (never: TR rows fit the stage)
        const u8* src = rows + t0 * row_bytes;
        __syncthreads();      // (the tile before this one has been read)
        for (u64 b = 4ull * tid; b + 4 <= nbytes; b += 1024) s_stage[b >> 2] = reinterpret_cast<const UDword*>(src + b)->v;
        if (tid < (nbytes & 3)) reinterpret_cast<u8*>(s_stage)[(nbytes & ~3ull) + tid] = src[(nbytes & ~3ull) + tid];
        __syncthreads();
      }
      const u32 total = nr * np;
      for (u32 i0 = 0; i0 < total; i0 += 256) {      // (uniform over the workgroup)
        const u32 i = i0 + tid;
        const bool act = i < total;
        u32 idx = 0;
        if (act) {
          const u32 p = i / nr, lr = i - p * nr;
          const uint2 pr = pairs[p0 + p];
          u32 a, b;
          if (STREAM) {
            const u8* q = s_bytes + (u64)lr * row_bytes + skip;
            if (COUNT) {
              const u8 *qa = q + 4ull * pr.x, *qb = q + 4ull * pr.y;
              a = (u32)qa[0] | (u32)qa[1] << 8 | (u32)qa[2] << 16 | (u32)qa[3] << 24;
              b = (u32)qb[0] | (u32)qb[1] << 8 | (u32)qb[2] << 16 | (u32)qb[3] << 24;
            } else { a = (q[pr.x >> 3] >> (pr.x & 7u)) & 1u; b = (q[pr.y >> 3] >> (pr.y & 7u)) & 1u; }
          } else {
            const u8* q = rows + (t0 + lr) * row_bytes + skip;
            if (COUNT) { a = reinterpret_cast<const UDword*>(q + 4ull * pr.x)->v; b = reinterpret_cast<const UDword*>(q + 4ull * pr.y)->v; }
            else { a = ((u32)q[pr.x >> 3] >> (pr.x & 7u)) & 1u; b = ((u32)q[pr.y >> 3] >> (pr.y & 7u)) & 1u; }
          }
          idx = p * cells + std::min(a, C2) * W + std::min(b, C2);
        }
        // the wave's hot cell: the first active lane's, added once for every lane that shares it
        const u64 todo = __ballot(act);
        if (todo) {      // (uniform over the wave)
          const int lead = __ffsll((long long)todo) - 1;
          const u32 hot = (u32)__shfl((int)idx, lead);
          const u64 same = __ballot(act && idx == hot);
          const u32 n = (int)lane == lead ? (u32)__popcll(same) : (u32)(act && idx != hot);
          if (n) { if (LDS) atomicAdd(&s_tab[idx], n); else atomicAdd(&out[idx], (u64)n); }
        }
      }
    }
    if (LDS) {
      __syncthreads();
      for (u32 i = tid; i < np * cells; i += 256) { const u32 n = s_tab[i]; if (n) atomicAdd(&out[i], (u64)n); }
    }
  }
}

static u32 sp_cus(const kmx_ctx* ctx) { return (u32)std::max(kmx_env_cus("KMX_SPECTRA_CUS", ctx), 1); }
static u32 sp_grid(u64 dflt) { return kmx_env_grid("KMX_SPECTRA_GRID", dflt); }
// the workgroups of a persistent grid whose workgroup holds `lds` bytes
static u32 sp_grid_of(u32 cus, size_t lds) { return sp_grid(std::min<u64>((u64)cus * std::min<u64>(8, std::max<u64>(2, SP_LDS_PER_CU / std::max<size_t>(lds, 1))), SP_MAX_GRID)); }

// the pairs of a call in groups: G pairs a group, U the most distinct columns a group has, sum_u their sum over the groups
struct JointPlan { u32 G, n_groups, U; u64 sum_u; bool lds, stream; };
static JointPlan joint_plan(const u32* pairs, u32 P, u32 C2, u64 row_bytes)
{
  JointPlan p{};
  const u32 cells = (C2 + 1) * (C2 + 1);
  p.lds = C2 <= SP_JOINT_LDS_CAP;
  p.G = p.lds ? std::min(SP_GROUP, SP_JOINT_LDS_WORDS / cells) : SP_GROUP;
  p.n_groups = (P + p.G - 1) / p.G;
  for (u32 g = 0; g < p.n_groups; g++) {
    const u32 p0 = g * p.G, np = std::min(p.G, P - p0);
    std::vector<u32> c(pairs + 2ull * p0, pairs + 2ull * (p0 + np));
    std::sort(c.begin(), c.end());
    const u32 u = (u32)(std::unique(c.begin(), c.end()) - c.begin());
    p.U = std::max(p.U, u); p.sum_u += u;
  }
  p.stream = (u64)SP_GATHER_FACTOR * 128 * p.U > row_bytes;
  return p;
}

// how a body's rows are cut into runs for `grid` workgroups over n_side items a run: -> rows of a run
static u32 sp_run_rows(u64 n_rows, u64 n_side, u32 grid, u32 least = SP_MIN_RUN)
{
  const u64 runs = std::max<u64>(1, grid / n_side);
  return (u32)std::max<u64>(least, (n_rows + runs - 1) / runs);
}

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
struct kmx_spectra_result : MatResult {
  u32 n_use = 0, n_pairs = 0, cap1 = 0, cap2 = 0, flags = 0;
  u64 joint_read = 0;      // the bytes the chosen road reads
  u64 *d_hist = nullptr, *d_joint = nullptr;
};

static int spectra_check(kmx_ctx* ctx, const kmx_spectra_task* T, const char* who, u64* row_bytes)
{
  const MatCheck c{ctx, who};
  const u32 N = T->n_cols, M = T->n_use, P = T->n_pairs;
  const bool hist = T->flags & KMX_SPECTRA_HIST, joint = T->flags & KMX_SPECTRA_JOINT;
  int rc;
  if ((rc = c.n_cols(N)) || (rc = c.no_bloom(T->mode, ": a Bloom row is a hash bit, it has no count")) || (rc = c.mode(T->mode)) ||
      (rc = c.key_words(T->key_words)) || (rc = c.flags(T->flags, KMX_SPECTRA_HIST | KMX_SPECTRA_JOINT))) return rc;
  if (!hist && !joint) return c.no(KMX_E_INVAL, ": one of KMX_SPECTRA_HIST and KMX_SPECTRA_JOINT is needed");
  if (hist) {
    if (M == 0) return c.no(KMX_E_INVAL, ": KMX_SPECTRA_HIST needs a list of at least one column");
    if ((rc = c.list_fits(M, N, "listed")) || (rc = c.identity(T->cols, M, N, "n_use"))) return rc;
    if (T->cap1 < 1 || T->cap1 > 65535) return c.no(KMX_E_INVAL, ": cap1 must be 1 ... 65535");
  } else if (M || T->cols || T->hist) return c.no(KMX_E_INVAL, ": n_use, cols or hist without KMX_SPECTRA_HIST");
  if (joint) {
    if (P == 0 || !T->pairs) return c.no(KMX_E_INVAL, ": KMX_SPECTRA_JOINT needs at least one pair");
    if (T->cap2 < 1 || T->cap2 > 255) return c.no(KMX_E_INVAL, ": cap2 must be 1 ... 255");
  } else if (P || T->pairs || T->joint) return c.no(KMX_E_INVAL, ": n_pairs, pairs or joint without KMX_SPECTRA_JOINT");
  *row_bytes = MatCheck::row_bytes(T->key_words, T->mode, N);
  if ((rc = c.row_fits(*row_bytes)) || (rc = c.n_rows(T->n_rows))) return rc;
  if (hist && (u64)M * ((u64)T->cap1 + 2) >= (1ull << 30)) return c.no(KMX_E_UNSUPPORTED, ": a hist table of 8 GiB and more");
  if (joint && (u64)P * (T->cap2 + 1) * (T->cap2 + 1) >= (1ull << 30)) return c.no(KMX_E_UNSUPPORTED, ": a joint table of 8 GiB and more");
  if ((rc = c.rows(T->n_rows, T->rows))) return rc;
  if (hist && (rc = c.col_list(T->cols, M, N))) return rc;
  if (joint) for (u64 i = 0; i < 2ull * P; i++) if (T->pairs[i] >= N) return c.no(KMX_E_INVAL, ": a pair's column index at or above n_cols");
  return KMX_OK;
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int spectra_queue(kmx_ctx* ctx, const kmx_spectra_task* T, kmx_spectra_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, M = R->n_use = T->n_use, P = R->n_pairs = T->n_pairs, skip = 8 * T->key_words, n_rows = (u32)R->n_rows;
  const u32 C1 = R->cap1 = T->cap1, C2 = R->cap2 = T->cap2;
  R->flags = T->flags;
  const bool count = T->mode == KMX_MODE_COUNT, hist = T->flags & KMX_SPECTRA_HIST, joint = T->flags & KMX_SPECTRA_JOINT;
  const u64 n_ord = ((u64)N + 7) / 8 * 8, hist_bytes = 8ull * M * ((u64)C1 + 2), cells = (u64)(C2 + 1) * (C2 + 1), joint_bytes = 8ull * P * cells;
  u32 *h_ordt = nullptr, *d_ordt = nullptr; uint2 *h_pairs = nullptr, *d_pairs = nullptr;
  JointPlan jp{};
  if (hist) {
    h_ordt = (u32*)R->pin(4 * n_ord);      // page-locked: the ordinal table on its way up
    if (!h_ordt) return ctx->fail(KMX_E_NOMEM, "kmx_spectra: host allocation failed");
    for (u64 i = 0; i < n_ord; i++) h_ordt[i] = !T->cols && i < N ? (u32)i : SP_NONE;
    if (T->cols) for (u32 j = 0; j < M; j++) h_ordt[T->cols[j]] = j;
    d_ordt = (u32*)R->tmp(4 * n_ord);
    R->d_hist = T->hist ? (u64*)T->hist : (u64*)R->keep(hist_bytes);
  }
  if (joint) {
    h_pairs = (uint2*)R->pin(8ull * P);
    if (!h_pairs) return ctx->fail(KMX_E_NOMEM, "kmx_spectra: host allocation failed");
    for (u32 p = 0; p < P; p++) h_pairs[p] = make_uint2(T->pairs[2ull * p], T->pairs[2ull * p + 1]);
    jp = joint_plan(T->pairs, P, C2, R->row_bytes);
    R->joint_read = jp.stream ? (u64)jp.n_groups * R->n_rows * R->row_bytes : R->n_rows * (count ? 4 : 1) * jp.sum_u;
    d_pairs = (uint2*)R->tmp(8ull * P);
    R->d_joint = T->joint ? (u64*)T->joint : (u64*)R->keep(joint_bytes);
  }
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_spectra: device allocation failed");
  if (hist) KMX_HIP(ctx, hipMemcpyAsync(d_ordt, h_ordt, 4 * n_ord, hipMemcpyHostToDevice, st));
  if (joint) KMX_HIP(ctx, hipMemcpyAsync(d_pairs, h_pairs, 8ull * P, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R, 3);      // ev: start, behind HIST, end
  if (rc != KMX_OK) return rc;
  if (hist && !T->hist) KMX_HIP(ctx, hipMemsetAsync(R->d_hist, 0, hist_bytes, st));
  if (joint && !T->joint) KMX_HIP(ctx, hipMemsetAsync(R->d_joint, 0, joint_bytes, st));
  const u32 cus = sp_cus(ctx);
  const u8* rows = (const u8*)T->rows;
  if (n_rows && hist) {
    const u64 units = count ? N : ((u64)N + 7) / 8;
    const bool lds = count && C1 <= SP_HIST_LDS_CAP;
    const size_t lds_bytes = lds ? (size_t)C1 * SP_BLOCK * 4 : 0;
    const u32 cap = sp_grid_of(cus, lds_bytes), n_blocks = (u32)((units + SP_BLOCK - 1) / SP_BLOCK), run = sp_run_rows(n_rows, n_blocks, cap, count ? SP_MIN_RUN : SP_MIN_RUN_PA);
    const u64 items = (((u64)n_rows + run - 1) / run) * n_blocks;
    const dim3 grid((u32)std::min<u64>(items, cap)), wg(64 * SP_HIST_WAVES);
    if (!count) hipLaunchKernelGGL(k_spectra_hist_pa, grid, wg, 0, st, rows, n_rows, R->row_bytes, skip, N, C1, (const u32*)d_ordt, n_blocks, run, items, R->d_hist);
    else if (lds)
      hipLaunchKernelGGL(k_spectra_hist_count<true>, grid, wg, lds_bytes, st, rows, n_rows, R->row_bytes, skip, N, C1, (const u32*)d_ordt, n_blocks, run, items, R->d_hist);
    else hipLaunchKernelGGL(k_spectra_hist_count<false>, grid, wg, 0, st, rows, n_rows, R->row_bytes, skip, N, C1, (const u32*)d_ordt, n_blocks, run, items, R->d_hist);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[1], st));
  if (n_rows && joint) {
    const u32 TR = jp.stream ? (u32)std::min<u64>(SP_TILE, SP_STAGE_BYTES / R->row_bytes) : SP_TILE;
    if (TR == 0) return ctx->fail(KMX_E_HIP, "kmx_spectra: a streamed row does not fit the stage");      // (never: see the file header)
    const size_t lds = (jp.lds ? (size_t)jp.G * cells * 4 : 0) + (jp.stream ? SP_STAGE_BYTES : 0);
    const u32 cap = sp_grid_of(cus, lds), run = (sp_run_rows(n_rows, jp.n_groups, cap) + TR - 1) / TR * TR;
    const u64 items = (((u64)n_rows + run - 1) / run) * jp.n_groups;
    const dim3 grid((u32)std::min<u64>(items, cap));
#define KMX_SP_JOINT(CNT, STR, LD) hipLaunchKernelGGL((k_spectra_joint<CNT, STR, LD>), grid, dim3(256), lds, st, rows, n_rows, R->row_bytes, skip, C2, \
                                                      (const uint2*)d_pairs, P, jp.G, jp.n_groups, TR, run, items, R->d_joint)
    switch ((count ? 4 : 0) | (jp.stream ? 2 : 0) | (jp.lds ? 1 : 0)) {
      case 0: KMX_SP_JOINT(false, false, false); break;
      case 1: KMX_SP_JOINT(false, false, true); break;
      case 2: KMX_SP_JOINT(false, true, false); break;
      case 3: KMX_SP_JOINT(false, true, true); break;
      case 4: KMX_SP_JOINT(true, false, false); break;
      case 5: KMX_SP_JOINT(true, false, true); break;
      case 6: KMX_SP_JOINT(true, true, false); break;
      default: KMX_SP_JOINT(true, true, true); break;
    }
#undef KMX_SP_JOINT
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R);
}

extern "C" int kmx_spectra_dev(kmx_ctx* ctx, const kmx_spectra_task* task, kmx_spectra_result** out)
{ return mat_call(ctx, task, out, false, "kmx_spectra_dev", "kmx_spectra", spectra_check, spectra_queue); }
extern "C" int kmx_spectra_host(kmx_ctx* ctx, const kmx_spectra_task* task, kmx_spectra_result** out)
{ return mat_call(ctx, task, out, true, "kmx_spectra_host", "kmx_spectra", spectra_check, spectra_queue); }

extern "C" int kmx_spectra_result_wait(kmx_spectra_result* R) { return mat_wait(R); }
extern "C" uint64_t* kmx_spectra_result_hist_dev(kmx_spectra_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_hist : nullptr; }
extern "C" uint64_t* kmx_spectra_result_joint_dev(kmx_spectra_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_joint : nullptr; }
extern "C" int kmx_spectra_result_copy_hist(kmx_spectra_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_hist, (u64)R->n_use * ((u64)R->cap1 + 2), 8, "kmx_spectra_result_copy_hist: the call was made without KMX_SPECTRA_HIST") : KMX_E_INVAL; }
extern "C" int kmx_spectra_result_copy_joint(kmx_spectra_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_joint, (u64)R->n_pairs * (R->cap2 + 1) * (R->cap2 + 1), 8, "kmx_spectra_result_copy_joint: the call was made without KMX_SPECTRA_JOINT") : KMX_E_INVAL; }
extern "C" double kmx_spectra_result_kernel_ms(kmx_spectra_result* R) { return mat_kernel_ms(R); }
extern "C" int kmx_spectra_result_kernel_parts_ms(kmx_spectra_result* R, double* hist_ms, double* joint_ms)
{ return mat_kernel_parts_ms(R, {hist_ms, joint_ms}, R ? R->flags & 3u : 0u); }
extern "C" uint64_t kmx_spectra_result_algo_bytes(kmx_spectra_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  u64 b = 0;
  if (R->flags & KMX_SPECTRA_HIST) b += R->n_rows * R->row_bytes + 8ull * R->n_use * ((u64)R->cap1 + 2);
  if (R->flags & KMX_SPECTRA_JOINT) b += R->joint_read + 8ull * R->n_pairs * (R->cap2 + 1) * (R->cap2 + 1);
  return b;
}
extern "C" void kmx_spectra_result_free(kmx_spectra_result* R) { mat_free(R); }
