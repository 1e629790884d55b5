// dist.hip -- `kmx dist` on the device: how the samples of a matrix relate to each other.  From the rows of one partition's matrix body
// (.count / .count_hash, .pa / .pa_hash, .cmbf) the N x N tables inter[i][j] = rows that hold samples i and j, and mins[i][j] = the sum
// over the rows of min(count_i, count_j): what the Jaccard and Bray-Curtis distances are computed from (include/kmx.h, section "dist").
// No reference counterpart in the kmtricks tree (Simka computes these tables on the CPU).  gfx950, wave64.
//
//   k_dist_slab    one pass over the rows, whichever mode: the presence bits, sample-major, in blocks of 64 samples.  Word w of sample
//                  s (bit r & 63 = row 64 w + r holds s) lies at slab[((s >> 6) * W + w) * 64 + (s & 63)], W = ceil(n_rows / 64): the 64
//                  samples of a block lie side by side, so a wave's store is 512 contiguous bytes here and a panel of k_dist_pairs is
//                  one contiguous run.  COUNT: a lane a column, 64 dword loads down the rows (a wave's load is 256 contiguous bytes),
//                  bit r = count != 0.  PA / BF: a lane a BYTE of the row (a wave's load is 64 contiguous bytes), its 8 columns in 8
//                  accumulators.  Padding columns and padding rows are zero.
//   k_dist_pairs   a workgroup a pair of sample blocks (I <= J) and a run of words: the two 64 x DP_CH word panels through LDS, a
//                  thread a 4 x 4 block of pairs, popcount(a & b) into u32 accumulators (a run is shorter than 2^26 words: no
//                  overflow), 64-bit atomic adds into the table at the run's end -- [i][j] and [j][i] for I < J; the diagonal block
//                  computes its whole square and writes every cell once.
//   k_dist_mins    the same decomposition over the count rows themselves: DM_TR rows x 64 counts of I and of J through LDS, min + add
//                  into u64 accumulators.
// Every load of a body byte is inside [rows, rows + n_rows * row_bytes) by construction: an address is rows + r * row_bytes + skip + b
// with r < n_rows and b + (bytes loaded) <= row_bytes - skip, both tested by the lane that loads; nothing is loaded in wider pieces
// than the piece that is tested (a byte for PA / BF, a count's dword for COUNT) and nothing is rounded to an aligned address.
#include "matrix_host.hpp"

#include <algorithm>
#include <cstring>

namespace kmx {

constexpr u32 DP_CH = 32;                 // slab words (64 rows each) of a panel in LDS: 2 x 16 KB
constexpr u64 DP_RUN_MIN = 64;            // words of the shortest run a workgroup of k_dist_pairs takes (4096 rows) ...
constexpr u64 DP_RUN_MAX = 1ull << 24;    // ... and of the longest: 2^24 words x 64 bits = 2^30 per u32 accumulator
constexpr u32 DM_TR = 32;                 // rows of a tile of k_dist_mins in LDS: 2 x 8 KB
constexpr u64 DM_RUN_MIN = 256;           // rows of the shortest run of k_dist_mins
constexpr u32 DIST_WGS_PER_CU = 8;        // workgroups a launch aims at: the number of runs per block pair follows


template <bool COUNT>
__global__ __launch_bounds__(256)
void k_dist_slab(const u8* __restrict__ rows, u64 n_rows, u64 row_bytes, u32 skip, u32 N, u32 NB, u64 W, u32 ct_n, u64 n_tiles,
                 u64* __restrict__ slab)
{
  const u32 lane = threadIdx.x & 63u;
  const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (u64)gridDim.x * 4;
  for (u64 t = wave; t < n_tiles; t += n_waves) {
    const u64 w = t / ct_n;
    const u32 ct = (u32)(t % ct_n);
    const u64 r0 = w * 64;
    const u32 nr = (u32)min((u64)64, n_rows - r0);      // (w < W: at least one row)
    if (COUNT) {      // a tile: 64 rows x the 64 columns of block ct
      const u32 c = ct * 64 + lane;
      u32 lo = 0, hi = 0;
      if (c < N) {
        const u8* p = rows + r0 * row_bytes + skip + 4ull * c;
        for (u32 r = 0; r < min(nr, 32u); r++) lo |= (u32)(reinterpret_cast<const UDword*>(p + r * row_bytes)->v != 0) << r;
        for (u32 r = 32; r < nr; r++) hi |= (u32)(reinterpret_cast<const UDword*>(p + r * row_bytes)->v != 0) << (r - 32);
      }
      slab[((u64)ct * W + w) * 64 + lane] = (u64)lo | ((u64)hi << 32);
    } else {          // a tile: 64 rows x 64 payload bytes (the 8 column blocks from 8 ct on)
      const u32 nb = (N + 7) / 8, bi = ct * 64 + lane;
      u32 lo[8], hi[8];
#pragma unroll
      for (int j = 0; j < 8; j++) { lo[j] = 0; hi[j] = 0; }
      if (bi < nb) {
        const u8* p = rows + r0 * row_bytes + skip + bi;
        const u32 keep = 8 * bi + 8 <= N ? 0xFFu : (1u << (N - 8 * bi)) - 1u;      // the padding bits of the last byte
        for (u32 r = 0; r < min(nr, 32u); r++) {
          const u32 x = p[r * row_bytes] & keep;
#pragma unroll
          for (int j = 0; j < 8; j++) lo[j] |= ((x >> j) & 1u) << r;
        }
        for (u32 r = 32; r < nr; r++) {
          const u32 x = p[r * row_bytes] & keep;
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
__device__ __forceinline__ void dist_pair_of(u32 bp, u32 NB, u32& I, u32& J)
{
  u32 i = 0;
  while (bp >= NB - i) { bp -= NB - i; i++; }
  I = i; J = i + bp;
}

__global__ __launch_bounds__(256)
void k_dist_pairs(const u64* __restrict__ slab, u64 W, u32 N, u32 NB, u32 runs, u64 run_words, u64* __restrict__ inter)
{
  __shared__ uint4 A[DP_CH * 32];      // [word][64 samples] u64
  __shared__ uint4 B[DP_CH * 32];
  u32 I, J;
  dist_pair_of(blockIdx.x / runs, NB, I, J);
  const u64 w0 = (u64)(blockIdx.x % runs) * run_words, w1 = min(W, w0 + run_words);
  if (w0 >= w1) return;
  const bool diag = I == J;
  const u32 tid = threadIdx.x, ti = tid >> 4, tj = tid & 15u;
  u32 acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; x++)
#pragma unroll
    for (int y = 0; y < 4; y++) acc[x][y] = 0;
  const uint4* Bp = diag ? A : B;
  for (u64 wc = w0; wc < w1; wc += DP_CH) {
    const u32 cn = (u32)min((u64)DP_CH, w1 - wc);
    const uint4* sa = reinterpret_cast<const uint4*>(slab + ((u64)I * W + wc) * 64);
    const uint4* sb = reinterpret_cast<const uint4*>(slab + ((u64)J * W + wc) * 64);
    __syncthreads();      // the chunk before this one has been read
    for (u32 i = tid; i < cn * 32; i += 256) {
      A[i] = sa[i];
      if (!diag) B[i] = sb[i];
    }
    __syncthreads();
    for (u32 k = 0; k < cn; k++) {
      const uint4 a01 = A[k * 32 + ti * 2], a23 = A[k * 32 + ti * 2 + 1], b01 = Bp[k * 32 + tj * 2], b23 = Bp[k * 32 + tj * 2 + 1];
      const u64 a[4] = {(u64)a01.x | ((u64)a01.y << 32), (u64)a01.z | ((u64)a01.w << 32), (u64)a23.x | ((u64)a23.y << 32), (u64)a23.z | ((u64)a23.w << 32)};
      const u64 b[4] = {(u64)b01.x | ((u64)b01.y << 32), (u64)b01.z | ((u64)b01.w << 32), (u64)b23.x | ((u64)b23.y << 32), (u64)b23.z | ((u64)b23.w << 32)};
#pragma unroll
      for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] += (u32)__popcll(a[x] & b[y]);
    }
  }
#pragma unroll
  for (int x = 0; x < 4; x++)
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const u32 i = I * 64 + ti * 4 + x, j = J * 64 + tj * 4 + y;
      if (i < N && j < N && acc[x][y]) {
        atomicAdd(&inter[(u64)i * N + j], (u64)acc[x][y]);
        if (!diag) atomicAdd(&inter[(u64)j * N + i], (u64)acc[x][y]);
      }
    }
}

__global__ __launch_bounds__(256)
void k_dist_mins(const u8* __restrict__ rows, u64 n_rows, u64 row_bytes, u32 skip, u32 N, u32 NB, u32 runs, u64 run_rows, u64* __restrict__ mins)
{
  __shared__ uint4 A[DM_TR * 16];      // [row][64 counts]
  __shared__ uint4 B[DM_TR * 16];
  u32 I, J;
  dist_pair_of(blockIdx.x / runs, NB, I, J);
  const u64 r0 = (u64)(blockIdx.x % runs) * run_rows, r1 = min(n_rows, r0 + run_rows);
  if (r0 >= r1) return;
  const bool diag = I == J;
  const u32 tid = threadIdx.x, ti = tid >> 4, tj = tid & 15u;
  u64 acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; x++)
#pragma unroll
    for (int y = 0; y < 4; y++) acc[x][y] = 0;
  const uint4* Bp = diag ? A : B;
  u32* Aw = reinterpret_cast<u32*>(A);
  u32* Bw = reinterpret_cast<u32*>(B);
  for (u64 rc = r0; rc < r1; rc += DM_TR) {
    const u32 cn = (u32)min((u64)DM_TR, r1 - rc);
    __syncthreads();
    for (u32 i = tid; i < cn * 64; i += 256) {      // a wave a row: 256 contiguous bytes
      const u8* p = rows + (rc + (i >> 6)) * row_bytes + skip;
      const u32 ca = I * 64 + (i & 63u), cb = J * 64 + (i & 63u);
      Aw[i] = ca < N ? reinterpret_cast<const UDword*>(p + 4ull * ca)->v : 0u;
      if (!diag) Bw[i] = cb < N ? reinterpret_cast<const UDword*>(p + 4ull * cb)->v : 0u;
    }
    __syncthreads();
    for (u32 k = 0; k < cn; k++) {
      const uint4 a4 = A[k * 16 + ti], b4 = Bp[k * 16 + tj];
      const u32 a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] += min(a[x], b[y]);
    }
  }
#pragma unroll
  for (int x = 0; x < 4; x++)
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const u32 i = I * 64 + ti * 4 + x, j = J * 64 + tj * 4 + y;
      if (i < N && j < N && acc[x][y]) {
        atomicAdd(&mins[(u64)i * N + j], acc[x][y]);
        if (!diag) atomicAdd(&mins[(u64)j * N + i], acc[x][y]);
      }
    }
}

// runs per block pair: enough workgroups to fill the chip, no run below run_min units or above run_max, a run a multiple of `step`
static void dist_runs(u64 units, u64 pairs, u32 n_cu, u64 run_min, u64 run_max, u32 step, u32* runs, u64* run_len)
{
  u64 r = std::max<u64>(1, (u64)std::max(n_cu, 1u) * DIST_WGS_PER_CU / pairs);
  r = std::min(r, (units + run_min - 1) / run_min);
  r = std::max<u64>(std::max<u64>(r, (units + run_max - 1) / run_max), 1);
  u64 len = (units + r - 1) / r;
  len = (len + step - 1) / step * step;
  *run_len = len;
  *runs = (u32)std::min<u64>((units + len - 1) / len, 0xFFFFFFFFull);
}

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
struct kmx_dist_result : MatResult {
  u64 slab_bytes = 0;
  bool want_mins = false;
  u64 *d_inter = nullptr, *d_mins = nullptr;
};

static int dist_check(kmx_ctx* ctx, const kmx_dist_task* T, const char* who, u64* row_bytes)
{
  const MatCheck c{ctx, who};
  int rc;
  if ((rc = c.n_cols(T->n_cols))) return rc;
  if (T->mode == KMX_MODE_BFC || T->mode == KMX_MODE_BFT)
    return c.no(KMX_E_UNSUPPORTED, ": counting Bloom filter and transposed bodies are not supported (KMX_MODE_COUNT, KMX_MODE_PA and KMX_MODE_BF only)");
  if (T->mode != KMX_MODE_COUNT && T->mode != KMX_MODE_PA && T->mode != KMX_MODE_BF) return c.no(KMX_E_INVAL, ": mode must be KMX_MODE_COUNT, KMX_MODE_PA or KMX_MODE_BF");
  if (T->key_words > 4) return c.no(KMX_E_INVAL, ": key_words must be at most 4");
  if (T->key_words == 0 && T->mode != KMX_MODE_BF) return c.no(KMX_E_INVAL, ": count and presence/absence rows have a key (key_words 1 ... 4)");
  if (T->key_words != 0 && T->mode == KMX_MODE_BF) return c.no(KMX_E_INVAL, ": Bloom filter rows have no key (key_words 0)");
  if ((T->want_mins || T->mins) && T->mode != KMX_MODE_COUNT) return c.no(KMX_E_INVAL, ": only count rows have counts to take minima of (want_mins needs KMX_MODE_COUNT)");
  if (T->mins && !T->want_mins) return c.no(KMX_E_INVAL, ": a mins table without want_mins");
  if ((rc = c.rows(T->n_rows, T->rows))) return rc;
  *row_bytes = MatCheck::row_bytes(T->key_words, T->mode, T->n_cols);
  if ((rc = c.row_fits(*row_bytes))) return rc;
  if (T->n_cols > 32768) return c.no(KMX_E_UNSUPPORTED, ": more than 32768 samples (a table would be 8 GiB and more)");
  if (T->n_rows > (1ull << 56) / *row_bytes) return c.no(KMX_E_UNSUPPORTED, ": a body of 2^56 bytes and more");
  return KMX_OK;
}

// the kernels of one call, queued on ctx->stream; T->rows a device pointer
static int dist_queue(kmx_ctx* ctx, const kmx_dist_task* T, kmx_dist_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, NB = (N + 63) / 64, skip = 8 * T->key_words, n_cu = (u32)std::max(kmx_plan_cus(ctx), 1);
  const u64 n_rows = T->n_rows, W = (n_rows + 63) / 64, table = (u64)N * N, pairs = (u64)NB * (NB + 1) / 2;
  const bool count = T->mode == KMX_MODE_COUNT;
  R->want_mins = T->want_mins != 0;
  u32 p_runs = 1, m_runs = 1; u64 p_len = DP_CH, m_len = DM_TR;
  if (n_rows) {
    dist_runs(W, pairs, n_cu, DP_RUN_MIN, DP_RUN_MAX, DP_CH, &p_runs, &p_len);
    dist_runs(n_rows, pairs, n_cu, DM_RUN_MIN, 1ull << 40, DM_TR, &m_runs, &m_len);
    if (pairs * p_runs > 0x7FFFFFFFull || (R->want_mins && pairs * m_runs > 0x7FFFFFFFull))
      return ctx->fail(KMX_E_UNSUPPORTED, "kmx_dist: too many rows for one call (send the body in runs of rows)");
  }
  R->slab_bytes = (u64)NB * 64 * W * 8;
  u64* d_slab = nullptr;
  if (n_rows && !(d_slab = (u64*)R->tmp(R->slab_bytes))) return ctx->fail(KMX_E_NOMEM, "kmx_dist: device allocation failed (send the body in runs of rows)");
  // a table of the call's own starts at zero; one the caller handed in is on neither list
  const bool own_inter = !T->inter, own_mins = R->want_mins && !T->mins;
  R->d_inter = own_inter ? (u64*)R->keep(8 * table) : (u64*)T->inter;
  R->d_mins = own_mins ? (u64*)R->keep(8 * table) : R->want_mins ? (u64*)T->mins : nullptr;
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_dist: device allocation failed");
  int rc = mat_queue_head(R, 4);      // ev: start, behind the slab, behind the pairs, end
  if (rc != KMX_OK) return rc;
  if (own_inter) KMX_HIP(ctx, hipMemsetAsync(R->d_inter, 0, 8 * table, st));
  if (own_mins) KMX_HIP(ctx, hipMemsetAsync(R->d_mins, 0, 8 * table, st));
  if (n_rows) {
    const u8* rows = (const u8*)T->rows;
    const u32 ct_n = count ? NB : (NB + 7) / 8;
    const u64 n_tiles = W * ct_n;
    const u32 grid = (u32)std::min<u64>((n_tiles + 3) / 4, kmx_grid_cap(1u << 20));
    if (count) hipLaunchKernelGGL(k_dist_slab<true>, dim3(grid), dim3(256), 0, st, rows, n_rows, R->row_bytes, skip, N, NB, W, ct_n, n_tiles, d_slab);
    else hipLaunchKernelGGL(k_dist_slab<false>, dim3(grid), dim3(256), 0, st, rows, n_rows, R->row_bytes, skip, N, NB, W, ct_n, n_tiles, d_slab);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[1], st));
  if (n_rows) {
    hipLaunchKernelGGL(k_dist_pairs, dim3((u32)(pairs * p_runs)), dim3(256), 0, st, (const u64*)d_slab, W, N, NB, p_runs, p_len, R->d_inter);
    KMX_HIP(ctx, hipGetLastError());
  }
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[2], st));
  if (n_rows && R->want_mins) {
    hipLaunchKernelGGL(k_dist_mins, dim3((u32)(pairs * m_runs)), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, NB, m_runs, m_len, R->d_mins);
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R);
}

extern "C" int kmx_dist_dev(kmx_ctx* ctx, const kmx_dist_task* task, kmx_dist_result** out)
{ return mat_call(ctx, task, out, false, "kmx_dist_dev", "kmx_dist", dist_check, dist_queue); }
extern "C" int kmx_dist_host(kmx_ctx* ctx, const kmx_dist_task* task, kmx_dist_result** out)
{ return mat_call(ctx, task, out, true, "kmx_dist_host", "kmx_dist", dist_check, dist_queue); }

extern "C" int kmx_dist_result_wait(kmx_dist_result* R) { return mat_wait(R); }
extern "C" uint64_t* kmx_dist_result_inter_dev(kmx_dist_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_inter : nullptr; }
extern "C" uint64_t* kmx_dist_result_mins_dev(kmx_dist_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_mins : nullptr; }
extern "C" int kmx_dist_result_copy_inter(kmx_dist_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_inter, (u64)R->n_cols * R->n_cols, 8) : KMX_E_INVAL; }
extern "C" int kmx_dist_result_copy_mins(kmx_dist_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_mins, (u64)R->n_cols * R->n_cols, 8, "kmx_dist_result_copy_mins: the call was made without want_mins") : KMX_E_INVAL; }
extern "C" double kmx_dist_result_kernel_ms(kmx_dist_result* R) { return mat_kernel_ms(R); }
extern "C" int kmx_dist_result_kernel_parts_ms(kmx_dist_result* R, double* slab_ms, double* pairs_ms, double* mins_ms)
{ return mat_kernel_parts_ms(R, {slab_ms, pairs_ms, mins_ms}, R && R->want_mins ? 7u : 3u); }
extern "C" uint64_t kmx_dist_result_algo_bytes(kmx_dist_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  const u64 table = 8ull * R->n_cols * R->n_cols;
  return R->n_rows * R->row_bytes + 2 * R->slab_bytes + table + (R->want_mins ? R->n_rows * 4 * R->n_cols + table : 0);
}
extern "C" void kmx_dist_result_free(kmx_dist_result* R) { mat_free(R); }
