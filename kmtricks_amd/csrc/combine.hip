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
#include "kmx_host.hpp"

namespace kmx {

constexpr u32 CB_TILE = 256;           // rows of a rank tile = threads of a workgroup
constexpr u32 CB_LDS_W = 2048;         // u64 words of keys staged per span (16 KB)
constexpr u32 CB_MAX_GRID = 1u << 18;  // workgroups of a launch: every kernel strides over its work

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

// ---- launchers ------------------------------------------------------------------------------------------------------------------
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
