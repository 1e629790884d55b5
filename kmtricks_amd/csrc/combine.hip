// combine.hip -- `kmx combine` on the device: the matrices of several runs that share a repartition joined by key, every block's
// columns behind the previous block's (km::MatrixMerger / PartitionMerger, include/kmtricks/matrix.hpp:396-886).  gfx950, wave64.
//
//   k_combine_keys    every block's keys gathered into a dense array (rows are up to 16 KB apart: a search at row stride would touch
//                     a cache line per probe)
//   k_combine_rank    a workgroup owns CB_TILE consecutive rows of one block, a thread one row's key.  Per other block two binary
//                     searches (first and last key of the tile) give the tile's span of that block's keys, which is staged in LDS
//                     when it fits; every row then searches the span.
//                       FIRST  is the row the first holder of its key (no block with a smaller index has it)?  -> a bit per row and
//                              a count per tile
//                       PLACE  the row's output index = over all blocks, the first holders below its key (tile base + the bits
//                              below); the row writes its own index + 1 into src[block][output row].  One writer per cell.
//   k_combine_scan    exclusive scan of every block's tile counts (a workgroup per block; no look-back, no spinning)
//   k_combine_total   output rows = the sum of the blocks' first holders; KMX_COMBINE_DROP_LAST takes the last row off when exactly
//                     one block's src column holds it
//   k_combine_move    a workgroup takes a run of consecutive output rows (about 128 KB) and cuts its bytes into 16-byte pieces aligned
//                     to the DESTINATION; a thread builds a piece and stores it whole.  A piece inside one 4-byte-count block's
//                     columns of a present row is one 16-byte load at the source's own alignment, a piece of an absent block is
//                     zeros; the others (keys, block boundaries, row ends, narrow counts, every PA piece) are built unit by unit.
//
// Nothing here holds a row in LDS: no limit on the number of columns.  No atomics, no library kernels.
#include "matrix_host.hpp"

namespace kmx {

constexpr u32 CB_TILE = 256;           // rows of a rank tile = threads of a workgroup
constexpr u32 CB_LDS_W = 2048;         // u64 words of keys staged per span (16 KB)
constexpr u32 CB_MAX_GRID = 1u << 18;  // workgroups of a launch: every kernel strides over its work

struct CombineBlock {      // one block as the kernels see it (array in HBM)
  const u8* rows;
  u64 irb;                 // bytes of a row: key + payload
  u64 key_off;             // rows of the blocks in front of it (its place in the dense key array)
  u32 n_rows, n_cols;
  u32 cb;                  // bytes of a count (COUNT)
  u32 pos;                 // its first column in the output
  u32 toff;                // its first tile slot: tiles + 1 slots a block (tile counts / bases with the total behind them, 4 u64 of bits a slot)
  u32 ntiles;
};

// a row's key: rows start at any byte (a .kmer body with 1-byte counts has 9-byte rows)
template <int KW> __device__ __forceinline__ Key<KW> cb_row_key(const u8* p) {
  if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) return load_key<KW>(p);
  Key<KW> k;
#pragma unroll
  for (int i = 0; i < KW; i++) {
    u64 w = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) w |= (u64)p[8 * i + b] << (8 * b);
    k.w[i] = w;
  }
  return k;
}
template <int KW> __device__ __forceinline__ Key<KW> cb_dense_key(const u64* p) {
  Key<KW> k;
#pragma unroll
  for (int i = 0; i < KW; i++) k.w[i] = p[i];
  return k;
}

// first key of keys[lo, hi) that is not below k (UPPER: that is above k); keys in global memory or LDS
template <int KW, bool UPPER> __device__ __forceinline__ u32 cb_bound(const u64* keys, u32 lo, u32 hi, const Key<KW>& k) {
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    const Key<KW> m = cb_dense_key<KW>(keys + (size_t)mid * KW);
    const bool right = UPPER ? !key_less<KW>(k, m) : key_less<KW>(m, k);
    if (right) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// work item f of a launch over the blocks' tile slots (ntiles + 1 a block) -> its block; false: past the end
__device__ __forceinline__ bool cb_slot(const CombineBlock* blocks, u32 nb, u32 f, u32* blk, u32* tile) {
  u32 i = 0;
  while (i + 1 < nb && blocks[i + 1].toff <= f) i++;
  *blk = i; *tile = f - blocks[i].toff;
  return *tile < blocks[i].ntiles;
}

template <int KW>
__global__ __launch_bounds__(CB_TILE)
void k_combine_keys(const CombineBlock* __restrict__ blocks, u32 nb, u32 n_slots, u64* __restrict__ keys)
{
  for (u32 f = blockIdx.x; f < n_slots; f += gridDim.x) {
    u32 i, t;
    if (!cb_slot(blocks, nb, f, &i, &t)) continue;
    const CombineBlock b = blocks[i];
    const u32 row = t * CB_TILE + threadIdx.x;
    if (row >= b.n_rows) continue;
    const Key<KW> k = cb_row_key<KW>(b.rows + (u64)row * b.irb);
    u64* dst = keys + (b.key_off + row) * KW;
#pragma unroll
    for (int w = 0; w < KW; w++) dst[w] = k.w[w];
  }
}

// first holders of block j in front of its row x: the tile's base + the bits below x in the tile
__device__ __forceinline__ u32 cb_firsts_below(const CombineBlock& bj, const u32* __restrict__ tbase, const u64* __restrict__ fbits, u32 x) {
  const u32 t = x >> 8, b = x & 255u;
  u32 v = tbase[bj.toff + t];
  if (b) {
    const u64* w = fbits + (size_t)(bj.toff + t) * 4;
#pragma unroll
    for (u32 q = 0; q < 4; q++) {
      if (b >= 64 * (q + 1)) v += (u32)__popcll(w[q]);
      else if (b > 64 * q) v += (u32)__popcll(w[q] & ((1ULL << (b - 64 * q)) - 1ULL));
    }
  }
  return v;
}

// PLACE = false: the FIRST pass (blocks below the tile's own), PLACE = true: the PLACE pass (every other block)
template <int KW, bool PLACE>
__global__ __launch_bounds__(CB_TILE)
void k_combine_rank(const CombineBlock* __restrict__ gblocks, u32 nb, u32 n_slots, const u64* __restrict__ keys,
                    u32* __restrict__ tcnt, u64* __restrict__ fbits, u32* __restrict__ src, u64 cap)
{
  constexpr u32 CAP = CB_LDS_W / KW;
  __shared__ u64 s_keys[CB_LDS_W];
  __shared__ u32 s_lo[64], s_hi[64];
  __shared__ CombineBlock s_blk[64];      // the descriptors, read once: every tile walks them, and looks into up to 63 of them
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid < nb) s_blk[tid] = gblocks[tid];
  __syncthreads();
  const CombineBlock* blocks = s_blk;
  for (u32 f = blockIdx.x; f < n_slots; f += gridDim.x) {
    u32 i, t;
    if (!cb_slot(blocks, nb, f, &i, &t)) continue;      // (uniform over the workgroup)
    const CombineBlock bi = blocks[i];
    const u32 row0 = t * CB_TILE, nr = min(CB_TILE, bi.n_rows - row0), row = row0 + tid;
    const u64* my = keys + bi.key_off * KW;
    Key<KW> k = key_inf<KW>();
    if (tid < nr) k = cb_dense_key<KW>(my + (size_t)row * KW);
    const u32 jn = PLACE ? nb : i;      // the blocks to look into: [0, jn) without i
    // the tile's span of every such block: thread j the lower end, thread 64 + j the upper end
    if (tid < 128) {
      const u32 j = tid & 63u;
      if (j < jn && j != i) {
        const CombineBlock bj = blocks[j];
        const u64* kj = keys + bj.key_off * KW;
        if (tid < 64) s_lo[j] = cb_bound<KW, false>(kj, 0, bj.n_rows, cb_dense_key<KW>(my + (size_t)row0 * KW));
        else s_hi[j] = cb_bound<KW, true>(kj, 0, bj.n_rows, cb_dense_key<KW>(my + (size_t)(row0 + nr - 1) * KW));
      }
    }
    __syncthreads();
    bool first = tid < nr;
    u32 place = 0;
    for (u32 j = 0; j < jn; j++) {
      if (j == i) continue;
      const CombineBlock bj = blocks[j];
      const u32 lo = s_lo[j], hi = s_hi[j];      // hi >= lo: the keys ascend
      const u32 span = hi > lo ? hi - lo : 0;
      const u64* kj = keys + (bj.key_off + lo) * KW;
      const bool staged = span > 0 && span <= CAP;
      if (staged) for (u32 q = tid; q < span * KW; q += CB_TILE) s_keys[q] = kj[q];
      __syncthreads();
      if (tid < nr) {
        const u64* base = staged ? s_keys : kj;
        const u32 x = span ? cb_bound<KW, false>(base, 0, span, k) : 0u;
        if constexpr (PLACE) place += cb_firsts_below(bj, tcnt, fbits, lo + x);
        else if (x < span && key_eq<KW>(cb_dense_key<KW>(base + (size_t)x * KW), k)) first = false;
      }
      __syncthreads();
    }
    if constexpr (PLACE) {
      if (tid < nr) {
        place += cb_firsts_below(bi, tcnt, fbits, row);
        if (place < cap) src[(u64)i * cap + place] = row + 1;      // (always, when every block's keys ascend strictly)
      }
    } else {
      const u64 bal = __ballot(first);
      if (lane == 0) fbits[(size_t)(bi.toff + t) * 4 + wave] = bal;
      const int c = __syncthreads_count(first);
      if (tid == 0) tcnt[bi.toff + t] = (u32)c;
    }
    __syncthreads();      // (s_lo / s_hi are rewritten by the next tile)
  }
}

// a[0, n) of every block -> its exclusive prefix sums in place, the total in a[n]; a workgroup per block
__global__ __launch_bounds__(1024)
void k_combine_scan(const CombineBlock* __restrict__ blocks, u32* __restrict__ tcnt)
{
  __shared__ u32 s_w[16];
  __shared__ u32 s_carry;
  u32* a = tcnt + blocks[blockIdx.x].toff;
  const u32 n = blocks[blockIdx.x].ntiles;
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (u32 base = 0; base < n; base += 1024) {
    const u32 i = base + tid;
    const u32 x = i < n ? a[i] : 0u;
    const u32 inc = wave_incl_scan(x, (int)lane);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u32 before = s_carry;
    for (u32 w = 0; w < wave; w++) before += s_w[w];
    if (i < n) a[i] = before + inc - x;
    __syncthreads();
    if (tid == 1023) s_carry = before + inc;
    __syncthreads();
  }
  if (tid == 0) a[n] = s_carry;
}

// one wave: tot[0] = output rows (after KMX_COMBINE_DROP_LAST), tot[1] = distinct keys of the union
__global__ __launch_bounds__(64)
void k_combine_total(const CombineBlock* __restrict__ blocks, u32 nb, const u32* __restrict__ tcnt, const u32* __restrict__ src, u64 cap,
                     int drop_last, u32* __restrict__ tot)
{
  const u32 j = threadIdx.x;
  u32 v = j < nb ? tcnt[blocks[j].toff + blocks[j].ntiles] : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  u32 rows = v;
  if (drop_last && rows) {
    const bool holds = j < nb && src[(u64)j * cap + (rows - 1)] != 0;
    if (__popcll(__ballot(holds)) == 1) rows--;
  }
  if (j == 0) { tot[0] = rows; tot[1] = v; }
}

// 16 bytes at any address: one global_load_dwordx4 (the hardware takes the address as it comes)
struct __attribute__((packed, aligned(1))) CbPiece { u32 w[4]; };
struct __attribute__((packed, aligned(1))) CbWord { u32 w; };
struct __attribute__((packed, aligned(1))) CbHalf { u16 w; };

// a whole piece leaves in one global_store_dwordx4.  The output is written once and read by nobody here: a streaming store -- which
// also keeps the compiler from folding it with the dword and byte stores of the run's two ragged ends
__device__ __forceinline__ void cb_store16(u8* p, uint4 q) {
  typedef u32 v4 __attribute__((ext_vector_type(4)));
  v4 v; v.x = q.x; v.y = q.y; v.z = q.z; v.w = q.w;
  __builtin_nontemporal_store(v, reinterpret_cast<v4*>(p));
}

struct CbLite { const u8* rows; u64 irb; u32 pos, n_cols, cb, pad; };

// PA = false: count rows, units of 4 bytes (keys and counts of the output are 4-byte aligned: rows of 8 * kw + 4 * N bytes behind a
// 256-byte aligned base).  PA = true: units of a byte.
template <bool PA>
__global__ __launch_bounds__(CB_TILE)
void k_combine_move(const CombineBlock* __restrict__ blocks, u32 nb, u32 kb, u32 n_cols, u32 orb, const u32* __restrict__ src, u64 cap,
                    const u32* __restrict__ tot, u32 sr_log, u8* __restrict__ out)
{
  constexpr u32 U = PA ? 1 : 4;
  __shared__ CbLite s_b[64];
  __shared__ u32 s_fblk[CB_TILE], s_frow[CB_TILE];      // the run's rows: the first block that holds the row, and where
  const u32 tid = threadIdx.x;
  if (tid < nb) { const CombineBlock b = blocks[tid]; s_b[tid] = CbLite{b.rows, b.irb, b.pos, b.n_cols, b.cb, 0}; }
  const u32 n_out = tot[0], sr = 1u << sr_log;
  const u32 n_groups = (u32)(((u64)n_out + sr - 1) >> sr_log);
  // the block that holds column `col`: the last one whose first column is not behind it (every block has a column)
  auto block_of = [&](u32 col) { u32 lo = 0, hi = nb; while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (s_b[mid].pos <= col) lo = mid; else hi = mid; } return lo; };
  for (u32 g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const u32 r0 = g << sr_log, nr = min(sr, n_out - r0);
    __syncthreads();
    if (tid < nr) {
      u32 fb = 0, fr = 0;
      for (u32 i = 0; i < nb; i++) { const u32 s = src[(u64)i * cap + r0 + tid]; if (s) { fb = i; fr = s - 1; break; } }
      s_fblk[tid] = fb; s_frow[tid] = fr;
    }
    __syncthreads();
    // one unit of the output: U bytes at byte c of the run's row r
    auto unit = [&](u32 r, u32 c) -> u32 {
      if (c < kb) {
        const CbLite& b = s_b[s_fblk[r]];
        const u8* p = b.rows + (u64)s_frow[r] * b.irb + c;
        if constexpr (PA) return *p; else return reinterpret_cast<const CbWord*>(p)->w;
      }
      if constexpr (!PA) {
        const u32 col = (c - kb) >> 2, i = block_of(col);
        const CbLite& b = s_b[i];
        const u32 s = src[(u64)i * cap + r0 + r];
        if (!s) return 0u;
        const u8* p = b.rows + (u64)(s - 1) * b.irb + kb + (u64)(col - b.pos) * b.cb;
        return b.cb == 4 ? reinterpret_cast<const CbWord*>(p)->w : b.cb == 2 ? (u32)reinterpret_cast<const CbHalf*>(p)->w : (u32)*p;
      } else {
        // the output's bits [bit0, bit1): shift and OR of the blocks that overlap them; padding bits of a block are not read in,
        // those of the output stay 0
        const u32 bit0 = (c - kb) * 8, bit1 = min(bit0 + 8, n_cols);
        u32 v = 0;
        for (u32 i = block_of(bit0); i < nb && s_b[i].pos < bit1; i++) {
          const CbLite& b = s_b[i];
          const u32 s = src[(u64)i * cap + r0 + r];
          if (!s) continue;
          const u32 lo = max(bit0, b.pos), hi = min(bit1, b.pos + b.n_cols), sb = lo - b.pos, nbit = hi - lo;
          const u8* p = b.rows + (u64)(s - 1) * b.irb + kb + (sb >> 3);
          u32 w = p[0];
          if ((sb & 7u) + nbit > 8) w |= (u32)p[1] << 8;
          v |= ((w >> (sb & 7u)) & ((1u << nbit) - 1u)) << (lo - bit0);
        }
        return v;
      }
    };
    const u64 B0 = (u64)r0 * orb, B1 = B0 + (u64)nr * orb;      // (nr * orb < 2^32: a run is about 128 KB, or one row)
    for (u64 p = (B0 >> 4) + tid; p < ((B1 + 15) >> 4); p += CB_TILE) {
      const u64 o = p << 4;
      const bool whole = o >= B0 && o + 16 <= B1;
      const u32 rel = o >= B0 ? (u32)(o - B0) : 0u;      // first byte of the piece that belongs to the run
      u32 r = rel / orb, c = rel - r * orb;
      if constexpr (!PA) {
        if (whole && c >= kb && c + 16 <= orb) {
          const u32 col = (c - kb) >> 2, i = block_of(col);
          const CbLite& b = s_b[i];
          if (b.cb == 4 && col + 4 <= b.pos + b.n_cols) {
            const u32 s = src[(u64)i * cap + r0 + r];
            uint4 q = make_uint4(0, 0, 0, 0);
            if (s) {
              const CbPiece pc = *reinterpret_cast<const CbPiece*>(b.rows + (u64)(s - 1) * b.irb + kb + (u64)(col - b.pos) * 4);
              q = make_uint4(pc.w[0], pc.w[1], pc.w[2], pc.w[3]);
            }
            cb_store16(out + o, q);
            continue;
          }
        }
      }
      // a piece over a key, a block boundary, narrow counts, a row's end or an end of the run (and every PA piece): unit by unit
      const u32 j0 = o >= B0 ? 0u : (u32)(B0 - o), j1 = o + 16 > B1 ? (u32)(B1 - o) : 16u;      // the piece's bytes that belong to the run
      u32 w[4];
#pragma unroll
      for (u32 q = 0; q < 4; q++) {
        u32 x = 0;
        for (u32 j = 4 * q; j < 4 * q + 4; j += U) {
          if (j < j0 || j >= j1) continue;
          if (c >= orb) { c = 0; r++; }
          x |= unit(r, c) << (8 * (j & 3u));
          c += U;
        }
        w[q] = x;
      }
      if (whole) cb_store16(out + o, make_uint4(w[0], w[1], w[2], w[3]));
      else {
#pragma unroll
        for (u32 q = 0; q < 4; q++) {
          if constexpr (!PA) { if (4 * q >= j0 && 4 * q < j1) *reinterpret_cast<u32*>(out + o + 4 * q) = w[q]; }
          else for (u32 j = 4 * q; j < 4 * q + 4; j++) if (j >= j0 && j < j1) out[o + j] = (u8)(w[q] >> (8 * (j & 3u)));
        }
      }
    }
  }
}

// ---- launchers: this file's own (no header declares them; their names stay among the library's dynamic symbols as they were) --------
static u32 cb_grid(u64 items) { return (u32)std::min<u64>(std::max<u64>(items, 1), kmx_grid_cap(CB_MAX_GRID)); }

u32 combine_tiles(u32 n) { return (n + CB_TILE - 1) / CB_TILE; }

hipError_t launch_combine_keys(int kw, const CombineBlock* blocks, u32 nb, u32 n_slots, u64* keys, hipStream_t st)
{
  const dim3 grid(cb_grid(n_slots)), wg(CB_TILE);
  switch (kw) {
    case 1: hipLaunchKernelGGL(k_combine_keys<1>, grid, wg, 0, st, blocks, nb, n_slots, keys); break;
    case 2: hipLaunchKernelGGL(k_combine_keys<2>, grid, wg, 0, st, blocks, nb, n_slots, keys); break;
    case 3: hipLaunchKernelGGL(k_combine_keys<3>, grid, wg, 0, st, blocks, nb, n_slots, keys); break;
    case 4: hipLaunchKernelGGL(k_combine_keys<4>, grid, wg, 0, st, blocks, nb, n_slots, keys); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <bool PLACE>
static hipError_t launch_rank(int kw, const CombineBlock* blocks, u32 nb, u32 n_slots, const u64* keys, u32* tcnt, u64* fbits, u32* src, u64 cap, hipStream_t st)
{
  const dim3 grid(cb_grid(n_slots)), wg(CB_TILE);
  switch (kw) {
    case 1: hipLaunchKernelGGL((k_combine_rank<1, PLACE>), grid, wg, 0, st, blocks, nb, n_slots, keys, tcnt, fbits, src, cap); break;
    case 2: hipLaunchKernelGGL((k_combine_rank<2, PLACE>), grid, wg, 0, st, blocks, nb, n_slots, keys, tcnt, fbits, src, cap); break;
    case 3: hipLaunchKernelGGL((k_combine_rank<3, PLACE>), grid, wg, 0, st, blocks, nb, n_slots, keys, tcnt, fbits, src, cap); break;
    case 4: hipLaunchKernelGGL((k_combine_rank<4, PLACE>), grid, wg, 0, st, blocks, nb, n_slots, keys, tcnt, fbits, src, cap); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_combine_first(int kw, const CombineBlock* blocks, u32 nb, u32 n_slots, const u64* keys, u32* tcnt, u64* fbits, hipStream_t st)
{ return launch_rank<false>(kw, blocks, nb, n_slots, keys, tcnt, fbits, nullptr, 0, st); }

hipError_t launch_combine_place(int kw, const CombineBlock* blocks, u32 nb, u32 n_slots, const u64* keys, u32* tcnt, u64* fbits, u32* src, u64 cap, hipStream_t st)
{ return launch_rank<true>(kw, blocks, nb, n_slots, keys, tcnt, fbits, src, cap, st); }

hipError_t launch_combine_scan(const CombineBlock* blocks, u32 nb, u32* tcnt, hipStream_t st)
{
  hipLaunchKernelGGL(k_combine_scan, dim3(nb), dim3(1024), 0, st, blocks, tcnt);
  return hipGetLastError();
}

hipError_t launch_combine_total(const CombineBlock* blocks, u32 nb, const u32* tcnt, const u32* src, u64 cap, int drop_last, u32* tot, hipStream_t st)
{
  hipLaunchKernelGGL(k_combine_total, dim3(1), dim3(64), 0, st, blocks, nb, tcnt, src, cap, drop_last, tot);
  return hipGetLastError();
}

hipError_t launch_combine_move(int pa, const CombineBlock* blocks, u32 nb, u32 kb, u32 n_cols, u32 orb, const u32* src, u64 cap, const u32* tot,
                               u8* out, hipStream_t st)
{
  u32 sr_log = 8;      // rows of a workgroup: about 128 KB of them (the output's row count is known on the device only: cap bounds it)
  while (sr_log > 0 && ((u64)orb << sr_log) > 131072) sr_log--;
  const u64 groups = (cap + (1u << sr_log) - 1) >> sr_log;
  const dim3 grid(cb_grid(groups)), wg(CB_TILE);
  if (pa) hipLaunchKernelGGL(k_combine_move<true>, grid, wg, 0, st, blocks, nb, kb, n_cols, orb, src, cap, tot, sr_log, out);
  else hipLaunchKernelGGL(k_combine_move<false>, grid, wg, 0, st, blocks, nb, kb, n_cols, orb, src, cap, tot, sr_log, out);
  return hipGetLastError();
}

}  // namespace kmx

using namespace kmx;

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
// kmx_combine_dev / kmx_combine_host: the blocks of one partition (or of one key range of it) joined by key
struct kmx_combine_result : MatResult {      // n_rows: the blocks' rows together, the bound of the output's rows; n_cols: their columns together;
  u32 nb = 0, kw = 0, mode = 0, flags = 0;   // row_bytes: 0 (every block has its own); h_tot: [0] output rows, [1] distinct keys
  u32 n_slots = 0;
  u64 orb = 0, in_bytes = 0;                 // a row of the output; the bytes of the blocks' rows
  u8* d_out = nullptr;
};

static u64 combine_block_row_bytes(const kmx_combine_task* K, const kmx_block& b)
{ return 8ull * K->key_words + (K->mode == KMX_MODE_COUNT ? (u64)b.n_cols * b.count_bytes : ((u64)b.n_cols + 7) / 8); }

static int combine_check(kmx_ctx* ctx, const kmx_combine_task* K, const char* who, u64* orb, u64* cap, u64* n_cols)
{
  const MatCheck c{ctx, who};
  int rc;
  if ((rc = c.key_words(K->key_words))) return rc;
  if (MatCheck::is_bloom(K->mode)) return c.no(KMX_E_UNSUPPORTED, ": Bloom filter matrices are not combined (KMX_MODE_COUNT and KMX_MODE_PA rows only)");
  if ((rc = c.mode(K->mode))) return rc;
  if (K->flags & ~(u32)KMX_COMBINE_DROP_LAST) return c.no(KMX_E_INVAL, ": unknown flag (KMX_COMBINE_DROP_LAST is the only one)");
  if (K->n_blocks == 0) return c.no(KMX_E_INVAL, ": a task has at least one block");
  if (K->n_blocks > KMX_COMBINE_MAX_BLOCKS) return c.no(KMX_E_UNSUPPORTED, ": " + std::to_string(K->n_blocks) + " blocks, at most " + std::to_string(KMX_COMBINE_MAX_BLOCKS) + " are combined in one call");
  if (!K->blocks) return c.no(KMX_E_INVAL, ": null block array");
  u64 cols = 0, rows = 0;
  for (u32 i = 0; i < K->n_blocks; i++) {
    const kmx_block& b = K->blocks[i];
    const std::string bi = ": block " + std::to_string(i);
    if (b.n_cols == 0) return c.no(KMX_E_INVAL, bi + ": a block has at least one column");
    if (K->mode == KMX_MODE_COUNT && b.count_bytes != 1 && b.count_bytes != 2 && b.count_bytes != 4) return c.no(KMX_E_INVAL, bi + ": count_bytes must be 1, 2 or 4");
    if (b.n_rows && !b.rows) return c.no(KMX_E_INVAL, bi + ": null row pointer");
    if (b.n_rows > 0xFFFFFF00ull) return c.no(KMX_E_UNSUPPORTED, bi + ": more than 2^32 - 256 rows (combine the partition in key ranges)");
    if (combine_block_row_bytes(K, b) > 0xFFFFFFFFull) return c.no(KMX_E_UNSUPPORTED, bi + ": rows of 4 GiB and more");
    cols += b.n_cols; rows += b.n_rows;
  }
  *orb = 8ull * K->key_words + (K->mode == KMX_MODE_COUNT ? 4 * cols : (cols + 7) / 8);
  if (*orb > 0xFFFFFFFFull) return c.no(KMX_E_UNSUPPORTED, ": output rows of 4 GiB and more");
  // the output's rows are known on the device only; the blocks' rows together bound them
  if (rows > 0xFFFFFF00ull) return c.no(KMX_E_UNSUPPORTED, ": the blocks hold more than 2^32 - 256 rows together, the bound of the output's rows (combine the partition in key ranges)");
  *cap = rows; *n_cols = cols;
  return KMX_OK;
}

// the kernels of one call, queued on ctx->stream; rows[i]: block i's rows in device memory
static int combine_queue(kmx_ctx* ctx, const kmx_combine_task* K, const void* const* rows, kmx_combine_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 nb = R->nb, kw = R->kw;
  CombineBlock* h_desc = (CombineBlock*)R->pin(sizeof(CombineBlock) * nb);      // the blocks as the kernels see them, on their way up
  if (!(R->h_tot = (u32*)R->pin(64)) || !h_desc) return ctx->fail(KMX_E_NOMEM, "kmx_combine: host allocation failed");
  R->h_tot[0] = R->h_tot[1] = 0;
  u64 key_off = 0; u32 pos = 0, toff = 0;
  for (u32 i = 0; i < nb; i++) {
    const kmx_block& b = K->blocks[i];
    CombineBlock& d = h_desc[i];
    d.rows = (const u8*)rows[i]; d.irb = combine_block_row_bytes(K, b); d.key_off = key_off;
    d.n_rows = (u32)b.n_rows; d.n_cols = b.n_cols; d.cb = K->mode == KMX_MODE_COUNT ? b.count_bytes : 0; d.pos = pos; d.toff = toff;
    d.ntiles = combine_tiles(d.n_rows);
    key_off += b.n_rows; pos += b.n_cols; toff += d.ntiles + 1;
    R->in_bytes += b.n_rows * d.irb;
  }
  R->n_slots = toff;
  const u64 cap = R->n_rows;
  CombineBlock* d_desc = (CombineBlock*)R->tmp(sizeof(CombineBlock) * nb);
  u32* d_tot = (u32*)R->tmp(64);
  u32* d_tcnt = (u32*)R->tmp(4ull * toff);
  u64* d_fbits = (u64*)R->tmp(32ull * toff);
  u64* d_keys = (u64*)R->tmp(8ull * kw * cap);
  u32* d_src = (u32*)R->tmp(4ull * nb * cap);
  R->d_out = (u8*)R->keep(cap * R->orb + 16);      // every key held by one block only
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_combine: device allocation failed");
  KMX_HIP(ctx, hipMemcpyAsync(d_desc, h_desc, sizeof(CombineBlock) * nb, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipMemsetAsync(d_tot, 0, 64, st));
  if (cap) {
    KMX_HIP(ctx, hipMemsetAsync(d_src, 0, 4ull * nb * cap, st));
    KMX_HIP(ctx, launch_combine_keys((int)kw, d_desc, nb, toff, d_keys, st));
    KMX_HIP(ctx, launch_combine_first((int)kw, d_desc, nb, toff, d_keys, d_tcnt, d_fbits, st));
    KMX_HIP(ctx, launch_combine_scan(d_desc, nb, d_tcnt, st));
    KMX_HIP(ctx, launch_combine_place((int)kw, d_desc, nb, toff, d_keys, d_tcnt, d_fbits, d_src, cap, st));
    KMX_HIP(ctx, launch_combine_total(d_desc, nb, d_tcnt, d_src, cap, (R->flags & KMX_COMBINE_DROP_LAST) != 0, d_tot, st));
    KMX_HIP(ctx, launch_combine_move(R->mode == KMX_MODE_PA, d_desc, nb, 8 * kw, R->n_cols, (u32)R->orb, d_src, cap, d_tot, R->d_out, st));
  }
  return mat_queue_tail(R, d_tot, d_tot + 1);
}

static int combine_call(kmx_ctx* ctx, const kmx_combine_task* task, kmx_combine_result** out, bool host, const char* who)
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, std::string(who) + ": null argument");
  *out = nullptr;
  u64 orb = 0, cap = 0, n_cols = 0;
  int rc = combine_check(ctx, task, who, &orb, &cap, &n_cols);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  kmx_combine_result* R = new kmx_combine_result();
  R->ctx = ctx; R->name = "kmx_combine"; R->n_rows = cap; R->row_bytes = 0; R->n_cols = (u32)n_cols;
  R->nb = task->n_blocks; R->kw = task->key_words; R->mode = task->mode; R->flags = task->flags; R->orb = orb;
  std::vector<const void*> rows(task->n_blocks);
  for (u32 i = 0; i < task->n_blocks; i++) rows[i] = task->blocks[i].rows;
  if (host) {      // the blocks that do not lie on the device
    for (u32 i = 0; i < task->n_blocks; i++) {
      const kmx_block& b = task->blocks[i];
      const u64 bytes = b.n_rows * combine_block_row_bytes(task, b);
      if (bytes && !(task->block_on_device && task->block_on_device[i])) rows[i] = mat_upload_tmp(R, b.rows, bytes);
    }
    rc = R->nomem ? ctx->fail(KMX_E_NOMEM, std::string(who) + ": upload allocation failed") : mat_uploads_done(R, who);
  }
  if (rc == KMX_OK) rc = combine_queue(ctx, task, rows.data(), R);
  return mat_finish(rc, R, out, host);
}
extern "C" int kmx_combine_dev(kmx_ctx* ctx, const kmx_combine_task* task, kmx_combine_result** out) { return combine_call(ctx, task, out, false, "kmx_combine_dev"); }
extern "C" int kmx_combine_host(kmx_ctx* ctx, const kmx_combine_task* task, kmx_combine_result** out) { return combine_call(ctx, task, out, true, "kmx_combine_host"); }

extern "C" int kmx_combine_result_wait(kmx_combine_result* R) { return mat_wait(R); }
extern "C" uint64_t kmx_combine_result_rows(kmx_combine_result* R) { return mat_wait(R) == KMX_OK ? R->h_tot[0] : 0; }
extern "C" uint64_t kmx_combine_result_row_bytes(const kmx_combine_result* R) { return R ? R->orb : 0; }
extern "C" uint64_t kmx_combine_result_body_bytes(kmx_combine_result* R) { return kmx_combine_result_rows(R) * (R ? R->orb : 0); }
extern "C" const void* kmx_combine_result_body_dev(kmx_combine_result* R) { return mat_wait(R) == KMX_OK ? R->d_out : nullptr; }
extern "C" uint64_t kmx_combine_result_algo_bytes(kmx_combine_result* R) { return mat_wait(R) == KMX_OK ? R->in_bytes + (u64)R->h_tot[0] * R->orb : 0; }
extern "C" int kmx_combine_result_copy_body(kmx_combine_result* R, void* host_dst, uint64_t dst_bytes)
{ return mat_copy_out(R, host_dst, dst_bytes, R ? R->d_out : nullptr, kmx_combine_result_body_bytes(R), 1); }
extern "C" double kmx_combine_result_kernel_ms(kmx_combine_result* R) { return mat_kernel_ms(R); }
extern "C" void kmx_combine_result_free(kmx_combine_result* R) { mat_free(R); }
