// filter.hip -- `kmx filter` on the device: the rows of a sorted k-mer matrix joined with one sample's sorted count list
// (km::FilterTask / km::MatrixFilter, include/kmtricks/cmd.hpp:609-724, matrix.hpp:23-393).  gfx950, wave64.
//
//   k_filter_match    a workgroup owns FT_TILE consecutive rows, a thread reads one row's key; two binary searches (first and last key
//                     of the tile) give the tile's span of the key list, which is staged in LDS when it fits (else the rows search
//                     global memory inside the span).  Per row: hit = 1 + the key record it met (0: none) and the vector value;
//                     per key record met: a mark byte.  Keys are unique on both sides: every mark has one writer, plain stores.
//   k_filter_scan     exclusive scan of the tiles' kept rows (one workgroup; a few thousand numbers) -> every tile's place
//   k_filter_move     the kept rows of a run of rows are contiguous in the output: the run's output is cut in 16-byte pieces aligned to
//                     the DESTINATION, a thread gathers a piece (from the row, and in count mode the new column) and stores it
//                     whole; the pieces that hang over the run's first and last byte leave in dwords or bytes
//   k_filter_absent_* the key records without a mark, compacted (count per tile, the same scan, scatter)
//
// Nothing here holds a row in LDS or a row's cursors: no limit on the number of columns.
#include "matrix_host.hpp"

namespace kmx {

constexpr u32 FT_TILE = 256;           // rows of a match tile = threads of a workgroup
constexpr u32 FT_LDS_DW = 4096;        // dwords of key records staged per tile (16 KB)
constexpr u32 FT_MAX_GRID = 1u << 18;  // workgroups of a launch: every kernel strides over its work

// first record of recs[lo, hi) whose key is not below k (UPPER: is above k); recs in global memory or LDS
template <int KW, bool UPPER> __device__ __forceinline__ u32 ft_bound(const u8* recs, u32 lo, u32 hi, const Key<KW>& k) {
  constexpr u32 RB = KW * 8 + 4;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    const Key<KW> m = load_key<KW>(recs + (size_t)mid * RB);
    const bool right = UPPER ? !key_less<KW>(k, m) : key_less<KW>(m, k);
    if (right) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int KW>
__global__ __launch_bounds__(FT_TILE)
void k_filter_match(const u8* __restrict__ rows, u32 n_rows, u64 irb, const u8* __restrict__ key, u32 n_key, int pa,
                    u32* __restrict__ hit, u32* __restrict__ vec, u8* __restrict__ marks, u32* __restrict__ tile_cnt)
{
  constexpr u32 RB = KW * 8 + 4, RW = RB / 4, CAP = FT_LDS_DW / RW;
  __shared__ u32 s_recs[FT_LDS_DW];
  __shared__ u32 s_span[2];
  const u32 tid = threadIdx.x;
  const u32 n_tiles = (n_rows + FT_TILE - 1) / FT_TILE;
  for (u32 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u32 row0 = t * FT_TILE, nr = min(FT_TILE, n_rows - row0), row = row0 + tid;
    Key<KW> k = key_inf<KW>();
    if (tid < nr) k = load_row_key<KW>(rows + (u64)row * irb);
    if (tid == 0) s_span[0] = ft_bound<KW, false>(key, 0, n_key, k);
    if (tid == 64) { const Key<KW> last = load_row_key<KW>(rows + (u64)(row0 + nr - 1) * irb); s_span[1] = ft_bound<KW, true>(key, 0, n_key, last); }
    __syncthreads();
    const u32 lo = s_span[0], hi = s_span[1];      // hi >= lo: the rows ascend
    const u32 span = hi > lo ? hi - lo : 0;
    const bool staged = span > 0 && span <= CAP;
    if (staged) {
      const u32* src = reinterpret_cast<const u32*>(key) + (size_t)lo * RW;
      for (u32 i = tid; i < span * RW; i += FT_TILE) s_recs[i] = src[i];
    }
    __syncthreads();
    u32 h = 0, v = 0;
    if (tid < nr && span) {
      const u8* base = staged ? reinterpret_cast<const u8*>(s_recs) : key + (size_t)lo * RB;
      const u32 i = ft_bound<KW, false>(base, 0, span, k);
      if (i < span) {
        const u8* rec = base + (size_t)i * RB;
        if (key_eq<KW>(load_key<KW>(rec), k)) {
          h = lo + i + 1;
          v = pa ? 1u : reinterpret_cast<const u32*>(rec)[RW - 1];
          marks[lo + i] = 1;
        }
      }
    }
    if (tid < nr) { hit[row] = h; vec[row] = v; }
    const int kept = __syncthreads_count(h != 0);
    if (tid == 0) tile_cnt[t] = (u32)kept;
  }
}

// a[0, n) -> its exclusive prefix sums in place, the total in a[n]; one workgroup
__global__ __launch_bounds__(1024)
void k_filter_scan(u32* __restrict__ a, u32 n)
{
  __shared__ u32 s_w[16];
  __shared__ u32 s_carry;
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

// 16 bytes at an address that is a multiple of U only: one global_load_dwordx4 (the hardware takes the address as it comes)
template <int U> struct __attribute__((packed, aligned(U))) FtPiece { u32 w[4]; };

// U: what rows and row sizes are multiples of -- 4 (every count matrix; PA rows of 4 * n bytes) or 1.
// A workgroup moves the kept rows among `sr` consecutive rows (sr a power of two <= FT_TILE: about 128 KB of rows).
template <int U>
__global__ __launch_bounds__(FT_TILE)
void k_filter_move(const u8* __restrict__ rows, u32 n_rows, u64 irb, u64 orb, const u32* __restrict__ hit, const u32* __restrict__ vec,
                   const u32* __restrict__ tile_base, u32 sr, u8* __restrict__ out)
{
  typedef typename std::conditional<U == 4, u32, u8>::type unit;
  constexpr u32 UP = 16 / U;      // units of a piece
  __shared__ u32 s_w[FT_TILE / 64];
  __shared__ u32 s_src[FT_TILE];      // the run's kept rows: their place in the tile
  __shared__ u32 s_val[FT_TILE];      // ... and their value in the new column
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 n_tiles = (n_rows + FT_TILE - 1) / FT_TILE, per_tile = FT_TILE / sr;
  const u64 n_groups = (u64)n_tiles * per_tile;
  for (u64 g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const u32 t = (u32)(g / per_tile), sub = (u32)(g % per_tile);
    const u32 row = t * FT_TILE + tid;
    const u32 h = row < n_rows ? hit[row] : 0u;
    const u64 bal = __ballot(h != 0);
    if (lane == 0) s_w[wave] = (u32)__popcll(bal);
    __syncthreads();
    u32 rank = (u32)__popcll(bal & ((1ULL << lane) - 1ULL));
    for (u32 w = 0; w < wave; w++) rank += s_w[w];
    // the run [r0, r1) of the tile's rows; ranks of its first kept row and behind its last
    const u32 r0 = sub * sr, r1 = r0 + sr;
    u32 first = 0, end = 0;
    {
      // rank in front of row r0 / r1: whole waves below, plus the lanes below inside the wave that holds it
      auto rank_at = [&](u32 r) { u32 s = 0; for (u32 w = 0; w < (r >> 6) && w < FT_TILE / 64; w++) s += s_w[w]; return s; };
      first = rank_at(r0); end = rank_at(r1);
    }
    // (sr < 64: r0 and r1 may lie inside a wave -- the lanes below them in that wave's ballot)
    __shared__ u64 s_bal[FT_TILE / 64];
    if (lane == 0) s_bal[wave] = bal;
    __syncthreads();
    if (r0 & 63u) first += (u32)__popcll(s_bal[r0 >> 6] & ((1ULL << (r0 & 63u)) - 1ULL));
    if (r1 & 63u) end += (u32)__popcll(s_bal[r1 >> 6] & ((1ULL << (r1 & 63u)) - 1ULL));
    const u32 nk = end - first;
    if (h != 0 && tid >= r0 && tid < r1) { s_src[rank - first] = tid; s_val[rank - first] = vec[row]; }
    __syncthreads();
    if (nk) {
      const u64 B0 = ((u64)tile_base[t] + first) * orb, len = (u64)nk * orb, B1 = B0 + len;
      const u8* tile_rows = rows + (u64)t * FT_TILE * irb;
      const bool small = len <= 0xFFFFFFFFull;
      for (u64 p = (B0 >> 4) + tid; p < ((B1 + 15) >> 4); p += FT_TILE) {
        const u64 o = p << 4;
        const bool whole = o >= B0 && o + 16 <= B1;
        const u64 rel = o >= B0 ? o - B0 : 0;      // first byte of the piece that belongs to the run
        u32 r; u64 c;
        if (small) { r = (u32)rel / (u32)orb; c = (u32)rel - r * (u32)orb; } else { r = (u32)(rel / orb); c = rel - (u64)r * orb; }
        FtPiece<U> pc;
        if (whole && c + 16 <= irb) {
          pc = *reinterpret_cast<const FtPiece<U>*>(tile_rows + (u64)s_src[r] * irb + c);
          *reinterpret_cast<uint4*>(out + o) = make_uint4(pc.w[0], pc.w[1], pc.w[2], pc.w[3]);
          continue;
        }
        // a piece over a row's end, the new column, or an end of the run: unit by unit
        unit u[UP];
        const u32 j0 = o >= B0 ? 0u : (u32)(B0 - o) / U;
        u32 j1 = UP;
        if (o + 16 > B1) j1 = (u32)(B1 - o) / U;
#pragma unroll
        for (u32 j = 0; j < UP; j++) {
          if (j < j0 || j >= j1) continue;
          if (c >= orb) { c = 0; r++; }
          if (c < irb) u[j] = *reinterpret_cast<const unit*>(tile_rows + (u64)s_src[r] * irb + c);
          else u[j] = U == 4 ? (unit)s_val[r] : (unit)(s_val[r] >> (8 * (u32)(c - irb)));
          c += U;
        }
        if (whole) {
          uint4 q;
          if constexpr (U == 4) q = make_uint4(u[0], u[1], u[2], u[3]);
          else {
            u32 w[4];
#pragma unroll
            for (u32 i = 0; i < 4; i++) w[i] = (u32)u[4 * i] | ((u32)u[4 * i + 1] << 8) | ((u32)u[4 * i + 2] << 16) | ((u32)u[4 * i + 3] << 24);
            q = make_uint4(w[0], w[1], w[2], w[3]);
          }
          *reinterpret_cast<uint4*>(out + o) = q;
        } else {
#pragma unroll
          for (u32 j = 0; j < UP; j++) if (j >= j0 && j < j1) *reinterpret_cast<unit*>(out + o + (u64)j * U) = u[j];
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(FT_TILE)
void k_filter_absent_count(const u8* __restrict__ marks, u32 n_key, u32* __restrict__ tile_cnt)
{
  const u32 n_tiles = (n_key + FT_TILE - 1) / FT_TILE;
  for (u32 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u32 i = t * FT_TILE + threadIdx.x;
    const int c = __syncthreads_count(i < n_key && marks[i] == 0);
    if (threadIdx.x == 0) tile_cnt[t] = (u32)c;
  }
}

template <int KW>
__global__ __launch_bounds__(FT_TILE)
void k_filter_absent_scatter(const u8* __restrict__ key, const u8* __restrict__ marks, u32 n_key, const u32* __restrict__ tile_base, u8* __restrict__ out)
{
  constexpr u32 RW = (KW * 8 + 4) / 4;
  __shared__ u32 s_w[FT_TILE / 64];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u32 n_tiles = (n_key + FT_TILE - 1) / FT_TILE;
  for (u32 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u32 i = t * FT_TILE + tid;
    const bool absent = i < n_key && marks[i] == 0;
    const u64 bal = __ballot(absent);
    if (lane == 0) s_w[wave] = (u32)__popcll(bal);
    __syncthreads();
    u32 rank = (u32)__popcll(bal & ((1ULL << lane) - 1ULL));
    for (u32 w = 0; w < wave; w++) rank += s_w[w];
    if (absent) {
      const u32* src = reinterpret_cast<const u32*>(key) + (size_t)i * RW;
      u32* dst = reinterpret_cast<u32*>(out) + ((size_t)tile_base[t] + rank) * RW;
#pragma unroll
      for (u32 w = 0; w < RW; w++) dst[w] = src[w];
    }
    __syncthreads();
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
static u32 ft_grid(u64 items) { return (u32)std::min<u64>(std::max<u64>(items, 1), kmx_grid_cap(FT_MAX_GRID)); }

u32 filter_tiles(u32 n) { return (n + FT_TILE - 1) / FT_TILE; }

hipError_t launch_filter_match(int kw, const u8* rows, u32 n_rows, u64 irb, const u8* key, u32 n_key, int pa,
                               u32* hit, u32* vec, u8* marks, u32* tile_cnt, hipStream_t st)
{
  const u32 grid = ft_grid(filter_tiles(n_rows));
  switch (kw) {
    case 1: hipLaunchKernelGGL(k_filter_match<1>, dim3(grid), dim3(FT_TILE), 0, st, rows, n_rows, irb, key, n_key, pa, hit, vec, marks, tile_cnt); break;
    case 2: hipLaunchKernelGGL(k_filter_match<2>, dim3(grid), dim3(FT_TILE), 0, st, rows, n_rows, irb, key, n_key, pa, hit, vec, marks, tile_cnt); break;
    case 3: hipLaunchKernelGGL(k_filter_match<3>, dim3(grid), dim3(FT_TILE), 0, st, rows, n_rows, irb, key, n_key, pa, hit, vec, marks, tile_cnt); break;
    case 4: hipLaunchKernelGGL(k_filter_match<4>, dim3(grid), dim3(FT_TILE), 0, st, rows, n_rows, irb, key, n_key, pa, hit, vec, marks, tile_cnt); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_filter_scan(u32* a, u32 n, hipStream_t st)
{
  hipLaunchKernelGGL(k_filter_scan, dim3(1), dim3(1024), 0, st, a, n);
  return hipGetLastError();
}

hipError_t launch_filter_move(const u8* rows, u32 n_rows, u64 irb, u64 orb, const u32* hit, const u32* vec, const u32* tile_base,
                              u8* out, hipStream_t st)
{
  u32 sr = FT_TILE;      // rows of a workgroup: about 128 KB of them
  while (sr > 1 && (u64)sr * irb > 131072) sr >>= 1;
  const u64 groups = (u64)filter_tiles(n_rows) * (FT_TILE / sr);
  const bool dwords = irb % 4 == 0 && orb % 4 == 0 && (reinterpret_cast<uintptr_t>(rows) & 3u) == 0;
  if (dwords) hipLaunchKernelGGL(k_filter_move<4>, dim3(ft_grid(groups)), dim3(FT_TILE), 0, st, rows, n_rows, irb, orb, hit, vec, tile_base, sr, out);
  else hipLaunchKernelGGL(k_filter_move<1>, dim3(ft_grid(groups)), dim3(FT_TILE), 0, st, rows, n_rows, irb, orb, hit, vec, tile_base, sr, out);
  return hipGetLastError();
}

hipError_t launch_filter_absent_count(const u8* marks, u32 n_key, u32* tile_cnt, hipStream_t st)
{
  hipLaunchKernelGGL(k_filter_absent_count, dim3(ft_grid(filter_tiles(n_key))), dim3(FT_TILE), 0, st, marks, n_key, tile_cnt);
  return hipGetLastError();
}

hipError_t launch_filter_absent_scatter(int kw, const u8* key, const u8* marks, u32 n_key, const u32* tile_base, u8* out, hipStream_t st)
{
  const u32 grid = ft_grid(filter_tiles(n_key));
  switch (kw) {
    case 1: hipLaunchKernelGGL(k_filter_absent_scatter<1>, dim3(grid), dim3(FT_TILE), 0, st, key, marks, n_key, tile_base, out); break;
    case 2: hipLaunchKernelGGL(k_filter_absent_scatter<2>, dim3(grid), dim3(FT_TILE), 0, st, key, marks, n_key, tile_base, out); break;
    case 3: hipLaunchKernelGGL(k_filter_absent_scatter<3>, dim3(grid), dim3(FT_TILE), 0, st, key, marks, n_key, tile_base, out); break;
    case 4: hipLaunchKernelGGL(k_filter_absent_scatter<4>, dim3(grid), dim3(FT_TILE), 0, st, key, marks, n_key, tile_base, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace kmx

using namespace kmx;

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
// kmx_filter_dev / kmx_filter_host: a run of whole rows of one partition's matrix against the new sample's count list
struct kmx_filter_result : MatResult {      // row_bytes: a row as it came in; h_tot: [0] kept rows, [1] absent records
  u32 n_key = 0, want = 0, kw = 0;
  u64 orb = 0;                              // a row of M
  u32* d_vec = nullptr;                     // null without KMX_FILTER_V
  u8 *d_out = nullptr, *d_absent = nullptr;
  u8* h_marks = nullptr;                    // kmx_filter_host: where the marks go back to
};

static int filter_check(kmx_ctx* ctx, const kmx_filter_task* K, const char* who, u64* irb, u64* orb)
{
  const MatCheck c{ctx, who};
  int rc;
  if ((rc = c.key_words(K->key_words))) return rc;
  if (MatCheck::is_bloom(K->mode))
    return c.no(KMX_E_UNSUPPORTED, ": Bloom filter matrices are not filtered (KMX_MODE_COUNT and KMX_MODE_PA rows of k-mer matrices only; hash matrices neither)");
  if ((rc = c.mode(K->mode)) || (rc = c.n_cols(K->n_cols))) return rc;
  if (K->want == 0 || (K->want & ~(u32)(KMX_FILTER_M | KMX_FILTER_V | KMX_FILTER_K))) return c.no(KMX_E_INVAL, ": want must be a non-empty set of KMX_FILTER_M | KMX_FILTER_V | KMX_FILTER_K");
  if (K->n_rows && !K->rows) return c.no(KMX_E_INVAL, ": null row pointer");
  if (K->key.n && !K->key.recs) return c.no(KMX_E_INVAL, ": null record pointer");
  if ((uintptr_t)K->key.recs & 3u) return c.no(KMX_E_INVAL, ": record pointers must be 4-byte aligned");
  *irb = MatCheck::row_bytes(K->key_words, K->mode, K->n_cols);
  *orb = *irb + (K->mode == KMX_MODE_COUNT ? 4 : 0);
  if ((rc = c.row_fits(*orb))) return rc;
  if (K->n_rows > 0xFFFFFF00ull) return c.no(KMX_E_UNSUPPORTED, ": more than 2^32 - 256 rows in one call (filter the partition in runs of rows)");
  if (K->key.n > 0xFFFFFF00ull) return c.no(KMX_E_UNSUPPORTED, ": more than 2^32 - 256 records in the key list");
  return KMX_OK;
}

// the kernels of one call, queued on ctx->stream; every pointer of K a device pointer
static int filter_queue(kmx_ctx* ctx, const kmx_filter_task* K, kmx_filter_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 n_rows = (u32)R->n_rows, n_key = R->n_key, tiles = filter_tiles(n_rows), ktiles = filter_tiles(n_key);
  const u64 irb = R->row_bytes, rb = R->kw * 8 + 4;
  const bool m = K->want & KMX_FILTER_M, v = K->want & KMX_FILTER_V, k = K->want & KMX_FILTER_K;
  if (!(R->h_tot = (u32*)R->pin(64))) return ctx->fail(KMX_E_NOMEM, "kmx_filter: host allocation failed");
  R->h_tot[0] = R->h_tot[1] = 0;
  u32* d_hit = (u32*)R->tmp(4ull * n_rows);
  u32* d_vec = (u32*)(v ? R->keep(4ull * n_rows) : R->tmp(4ull * n_rows));
  u32* d_tiles = (u32*)R->tmp(4ull * (tiles + 1));
  u32* d_ktiles = nullptr;
  u8 *marks = K->marks, *marks_own = nullptr;
  if (!marks) marks = marks_own = (u8*)R->tmp(n_key);
  if (v) R->d_vec = d_vec;
  if (m) R->d_out = (u8*)R->keep((u64)n_rows * R->orb + 16);      // every row kept
  if (k) { d_ktiles = (u32*)R->tmp(4ull * (ktiles + 1)); R->d_absent = (u8*)R->keep((u64)n_key * rb); }
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_filter: device allocation failed");
  if (marks_own && n_key) KMX_HIP(ctx, hipMemsetAsync(marks_own, 0, n_key, st));
  int rc = mat_queue_head(R);
  if (rc != KMX_OK) return rc;
  if (n_rows) KMX_HIP(ctx, launch_filter_match((int)R->kw, (const u8*)K->rows, n_rows, irb, (const u8*)K->key.recs, n_key, K->mode == KMX_MODE_PA,
                                               d_hit, d_vec, marks, d_tiles, st));
  KMX_HIP(ctx, launch_filter_scan(d_tiles, tiles, st));
  if (m && n_rows) KMX_HIP(ctx, launch_filter_move((const u8*)K->rows, n_rows, irb, R->orb, d_hit, d_vec, d_tiles, R->d_out, st));
  if (k) {
    if (n_key) KMX_HIP(ctx, launch_filter_absent_count(marks, n_key, d_ktiles, st));
    KMX_HIP(ctx, launch_filter_scan(d_ktiles, ktiles, st));
    if (n_key) KMX_HIP(ctx, launch_filter_absent_scatter((int)R->kw, (const u8*)K->key.recs, marks, n_key, d_ktiles, R->d_absent, st));
  }
  if (R->h_marks && n_key) KMX_HIP(ctx, hipMemcpyAsync(R->h_marks, marks, n_key, hipMemcpyDeviceToHost, st));
  return mat_queue_tail(R, d_tiles + tiles, k ? d_ktiles + ktiles : nullptr);
}

extern "C" uint8_t* kmx_filter_marks_alloc(kmx_ctx* ctx, uint64_t n)
{
  if (!ctx || hipSetDevice(ctx->device) != hipSuccess) return nullptr;
  u8* p = (u8*)ctx->dalloc(n);
  if (!p) { ctx->fail(KMX_E_NOMEM, "kmx_filter_marks_alloc: device allocation failed"); return nullptr; }
  if (hipMemsetAsync(p, 0, n ? n : 1, ctx->stream) != hipSuccess) { ctx->dfree(p); ctx->fail(KMX_E_HIP, "kmx_filter_marks_alloc: clearing failed"); return nullptr; }
  return p;
}
extern "C" void kmx_filter_marks_free(kmx_ctx* ctx, uint8_t* marks) { if (ctx && marks) { (void)hipStreamSynchronize(ctx->stream); ctx->dfree(marks); } }

static int filter_call(kmx_ctx* ctx, const kmx_filter_task* task, kmx_filter_result** out, bool host, const char* who)
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, std::string(who) + ": null argument");
  *out = nullptr;
  u64 irb = 0, orb = 0;
  int rc = filter_check(ctx, task, who, &irb, &orb);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  kmx_filter_result* R = new kmx_filter_result();
  R->ctx = ctx; R->name = "kmx_filter"; R->n_rows = task->n_rows; R->row_bytes = irb; R->n_cols = task->n_cols;
  R->n_key = (u32)task->key.n; R->want = task->want; R->kw = task->key_words; R->orb = orb;
  kmx_filter_task dt = *task;
  if (host) {      // the rows and, unless they lie on the device, the key list and its marks
    const u64 rows_bytes = task->n_rows * irb, key_bytes = task->key.n * (task->key_words * 8 + 4);
    if (rows_bytes) dt.rows = mat_upload_tmp(R, task->rows, rows_bytes);
    if (!task->key_on_device) {
      if (key_bytes) dt.key.recs = mat_upload_tmp(R, task->key.recs, key_bytes);
      if (task->marks && task->key.n) { dt.marks = (u8*)mat_upload_tmp(R, task->marks, task->key.n); R->h_marks = task->marks; }
    }
    rc = R->nomem ? ctx->fail(KMX_E_NOMEM, std::string(who) + ": upload allocation failed") : mat_uploads_done(R, who);
  }
  if (rc == KMX_OK) rc = filter_queue(ctx, &dt, R);
  return mat_finish(rc, R, out, host);
}
extern "C" int kmx_filter_dev(kmx_ctx* ctx, const kmx_filter_task* task, kmx_filter_result** out) { return filter_call(ctx, task, out, false, "kmx_filter_dev"); }
extern "C" int kmx_filter_host(kmx_ctx* ctx, const kmx_filter_task* task, kmx_filter_result** out) { return filter_call(ctx, task, out, true, "kmx_filter_host"); }

extern "C" int kmx_filter_result_wait(kmx_filter_result* R) { return mat_wait(R); }
extern "C" uint64_t kmx_filter_result_rows(kmx_filter_result* R) { return mat_wait(R) == KMX_OK ? R->h_tot[0] : 0; }
extern "C" uint64_t kmx_filter_result_row_bytes(const kmx_filter_result* R) { return R ? R->orb : 0; }
extern "C" uint64_t kmx_filter_result_body_bytes(kmx_filter_result* R) { return R && (R->want & KMX_FILTER_M) ? kmx_filter_result_rows(R) * R->orb : 0; }
extern "C" const void* kmx_filter_result_body_dev(kmx_filter_result* R) { return mat_wait(R) == KMX_OK ? R->d_out : nullptr; }
extern "C" const void* kmx_filter_result_vector_dev(kmx_filter_result* R) { return mat_wait(R) == KMX_OK ? R->d_vec : nullptr; }
extern "C" uint64_t kmx_filter_result_vector_len(const kmx_filter_result* R) { return R && (R->want & KMX_FILTER_V) ? R->n_rows : 0; }
extern "C" uint64_t kmx_filter_result_absent(kmx_filter_result* R) { return R && (R->want & KMX_FILTER_K) && mat_wait(R) == KMX_OK ? R->h_tot[1] : 0; }
extern "C" const void* kmx_filter_result_absent_dev(kmx_filter_result* R) { return mat_wait(R) == KMX_OK ? R->d_absent : nullptr; }
extern "C" int kmx_filter_result_copy_body(kmx_filter_result* R, void* host_dst, uint64_t dst_bytes)
{ return mat_copy_out(R, host_dst, dst_bytes, R ? R->d_out : nullptr, kmx_filter_result_body_bytes(R), 1); }
extern "C" int kmx_filter_result_copy_vector(kmx_filter_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return mat_copy_out(R, host_dst, dst_entries, R ? R->d_vec : nullptr, kmx_filter_result_vector_len(R), 4); }
extern "C" int kmx_filter_result_copy_absent(kmx_filter_result* R, void* host_dst, uint64_t dst_bytes)
{ return mat_copy_out(R, host_dst, dst_bytes, R ? R->d_absent : nullptr, R ? kmx_filter_result_absent(R) * (R->kw * 8 + 4) : 0, 1); }
extern "C" double kmx_filter_result_kernel_ms(kmx_filter_result* R) { return mat_kernel_ms(R); }
extern "C" uint64_t kmx_filter_result_algo_bytes(kmx_filter_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  const u64 rb = R->kw * 8 + 4;
  u64 b = R->n_rows * 8 * R->kw + (u64)R->n_key * rb;
  if (R->want & KMX_FILTER_M) b += (u64)R->h_tot[0] * (R->row_bytes + R->orb);
  if (R->want & KMX_FILTER_V) b += 4 * R->n_rows;
  if (R->want & KMX_FILTER_K) b += (u64)R->h_tot[1] * rb;
  return b;
}
extern "C" void kmx_filter_result_free(kmx_filter_result* R) { mat_free(R); }
