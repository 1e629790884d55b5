// groupsum.hip -- a group-by over a matrix body on the device: per label of a row and listed sample, the rows that hold the sample and the
// sum of their counts (include/kmx.h, section "groupsum"; with the unitig ids of kmx_unitigs_* as labels MUSET's unitig x sample
// abundance table).  No reference counterpart in the kmtricks tree.  gfx950, wave64.
//
//   k_gs_rows   a wave a chunk of rows (mat_row_plan), L lanes a row, a lane an ORDINAL of the list (the column comes from a table per
//               ordinal, the identity included).  Lists of 64 ordinals and more give the wave a row and 64 ordinals a trip over the chunk;
//               shorter lists give L lanes a row and each of the 64 / L groups of lanes a run of L neighbouring rows.  A lane keeps
//               (rows present, sum of counts) of its ordinal in registers while neighbouring rows share their label and adds them to the
//               tables when the label changes: non-returning device-scope atomics, one per (run of equal labels, ordinal present in it).
//               Labels outside [g0, g0 + G) end a run and add nothing.
// The kernel waits on nothing: any grid is a correct one.  Every load of a body byte is inside [rows, rows + n_rows * row_bytes): an
// address is rows + r * row_bytes + skip + b with r < n_rows and b + (bytes loaded) <= row_bytes - skip, both tested by the lane that
// loads (c < N).  A table index is (g - g0) * M + j with g - g0 < G and j < M.  The launch knobs are this file's own: KMX_GROUPSUM_CUS and
// KMX_GROUPSUM_GRID.
#include "matrix_host.hpp"

#include <algorithm>

namespace kmx {

constexpr u32 GS_OUT = 0xFFFFFFFFu;       // "outside the window" as a run's label (a label inside is g - g0 < G <= 2^32 - 1)
constexpr u32 GS_WGS_PER_CU = 8;
constexpr u32 GS_MAX_GRID = 1u << 16;
constexpr u32 GS_WAVES_PER_SIMD = 8;

static_assert(sizeof(kmx_groupsum_task) == 88, "kmx_groupsum_task is 88 bytes");

template <bool COUNT> __device__ __forceinline__ u32 gs_unit(const u8* q, u32 c) { return COUNT ? reinterpret_cast<const UDword*>(q + 4ull * c)->v : (u32)q[c >> 3]; }
template <bool COUNT> __device__ __forceinline__ bool gs_present(u32 v, u32 c, u32 a) { return COUNT ? v >= a : (bool)((v >> (c & 7u)) & 1u); }

// colt: the input column of every ordinal, M entries.  L: lanes of a row (a power of two <= 64, >= M when below 64); RW: rows of a wave's
// chunk (64 when L < 64)
template <bool COUNT, bool SUMS>
__global__ __launch_bounds__(256)
void k_gs_rows(const u8* __restrict__ rows, u32 n_rows, u64 row_bytes, u32 skip, u32 N, u32 M, u32 L, u32 RW, const u32* __restrict__ colt,
               const u32* __restrict__ groups, u32 a, u32 g0, u32 G, u32* __restrict__ present, u64* __restrict__ sums, u32* __restrict__ size)
{
  const u32 lane = threadIdx.x & 63u, u = lane & (L - 1u), sub = lane / L;
  const u32 rps = RW / (64u / L);      // rows of a group of L lanes: RW with L == 64, L below
  const u64 n_chunks = ((u64)n_rows + RW - 1) / RW;
  for (u64 ch = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; ch < n_chunks; ch += (u64)gridDim.x * 4) {
    const u64 row0 = ch * RW + (u64)sub * rps, rend = min(row0 + rps, (u64)n_rows);
    for (u64 j0 = 0; j0 < M; j0 += L) {      // (one trip when L < 64)
      const u64 j = j0 + u;
      const u32 c = j < M ? colt[j] : N;     // (N: no column)
      u32 cur = GS_OUT, np = 0, nsz = 0;
      u64 sm = 0;
      auto flush = [&]() {
        if (cur == GS_OUT) return;
        if (np) atomicAdd(&present[(u64)cur * M + j], np);
        if (SUMS && sm) atomicAdd(&sums[(u64)cur * M + j], sm);
        if (j == 0 && nsz) atomicAdd(&size[cur], nsz);
      };
      for (u64 row = row0; row < rend; row++) {
        const u32 gl = groups[row];
        const u32 key = gl >= g0 && gl - g0 < G ? gl - g0 : GS_OUT;
        if (key != cur) { flush(); cur = key; np = 0; nsz = 0; sm = 0; }
        if (key == GS_OUT) continue;
        nsz++;
        if (c < N) {
          const u32 v = gs_unit<COUNT>(rows + row * row_bytes + skip, c);
          if (gs_present<COUNT>(v, c, a)) { np++; if (SUMS) sm += v; }
        }
      }
      flush();
    }
  }
}

static u32 gs_cus(const kmx_ctx* ctx) { return (u32)std::max(kmx_env_cus("KMX_GROUPSUM_CUS", ctx), 1); }
static u32 gs_grid(u64 dflt) { return kmx_env_grid("KMX_GROUPSUM_GRID", dflt); }

}  // namespace kmx

using namespace kmx;

// ---- C ABI: the shared host path is matrix_host.hpp ------------------------------------------------------------------------------------
struct kmx_groupsum_result : MatResult {
  u32 n_use = 0, G = 0;
  bool want_sums = false;
  u32 *d_present = nullptr, *d_size = nullptr;
  u64* d_sums = nullptr;
};

static int groupsum_check(kmx_ctx* ctx, const kmx_groupsum_task* T, const char* who, u64* row_bytes)
{
  const MatCheck c{ctx, who};
  const u32 N = T->n_cols, M = T->n_use;
  int rc;
  if ((rc = c.n_cols(N, M, "list")) || (rc = c.no_bloom(T->mode, ": a Bloom row is a hash bit, not a k-mer of a group")) || (rc = c.mode(T->mode)) ||
      (rc = c.key_words(T->key_words)) || (rc = c.min_abund(T->min_abund, T->mode)) || (rc = c.flags(T->flags, KMX_GROUPSUM_SUMS))) return rc;
  if (T->n_groups == 0) return c.no(KMX_E_INVAL, ": a window of no groups");
  if ((u64)T->g0 + T->n_groups > (1ull << 32)) return c.no(KMX_E_INVAL, ": the window ends beyond 2^32");
  if ((T->flags & KMX_GROUPSUM_SUMS) && T->mode == KMX_MODE_PA) return c.no(KMX_E_INVAL, ": sums need counts (KMX_MODE_COUNT)");
  if (T->sums && T->mode == KMX_MODE_PA) return c.no(KMX_E_INVAL, ": a sums table needs counts (KMX_MODE_COUNT)");
  if (T->sums && !(T->flags & KMX_GROUPSUM_SUMS)) return c.no(KMX_E_INVAL, ": a sums table without KMX_GROUPSUM_SUMS");
  if ((rc = c.list_fits(M, N, "listed")) || (rc = c.identity(T->cols, M, N, "n_use"))) return rc;
  *row_bytes = MatCheck::row_bytes(T->key_words, T->mode, N);
  if ((rc = c.row_fits(*row_bytes)) || (rc = c.n_rows(T->n_rows))) return rc;
  if ((u64)T->n_groups * M > (1ull << 32)) return c.no(KMX_E_UNSUPPORTED, ": tables of more than 2^32 entries (send the groups in windows)");
  if ((rc = c.rows(T->n_rows, T->rows))) return rc;
  if (T->n_rows && !T->groups) return c.no(KMX_E_INVAL, ": null groups");
  return c.col_list(T->cols, M, N);
}

// the kernel of one call, queued on ctx->stream; T->rows a device pointer; HOST: T->groups a host array, sent up here
template <bool HOST>
static int groupsum_queue(kmx_ctx* ctx, const kmx_groupsum_task* T, kmx_groupsum_result* R)
{
  hipStream_t st = ctx->stream;
  const u32 N = T->n_cols, M = R->n_use = T->n_use, skip = 8 * T->key_words, n_rows = (u32)R->n_rows, G = R->G = T->n_groups;
  const bool count = T->mode == KMX_MODE_COUNT, sm = R->want_sums = (T->flags & KMX_GROUPSUM_SUMS) != 0;
  const u64 cells = (u64)G * M;
  u32* h_colt = (u32*)R->pin(4ull * M);      // page-locked: the column table on its way up
  if (!h_colt) return ctx->fail(KMX_E_NOMEM, "kmx_groupsum: host allocation failed");
  for (u32 j = 0; j < M; j++) h_colt[j] = T->cols ? T->cols[j] : j;
  u32* d_colt = (u32*)R->tmp(4ull * M);
  // a table of the call's own starts at zero; one the caller handed in is on neither list
  const bool own_p = !T->present, own_s = sm && !T->sums, own_z = !T->size;
  R->d_present = own_p ? (u32*)R->keep(4 * cells) : T->present;
  R->d_size = own_z ? (u32*)R->keep(4ull * G) : T->size;
  if (sm) R->d_sums = own_s ? (u64*)R->keep(8 * cells) : (u64*)T->sums;
  const u32* d_groups = T->groups;
  if (HOST && n_rows) d_groups = (u32*)R->tmp(4ull * n_rows);
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, "kmx_groupsum: device allocation failed (send the groups in windows)");
  KMX_HIP(ctx, hipMemcpyAsync(d_colt, h_colt, 4ull * M, hipMemcpyHostToDevice, st));
  if (HOST && n_rows) KMX_HIP(ctx, hipMemcpyAsync((void*)d_groups, T->groups, 4ull * n_rows, hipMemcpyHostToDevice, st));
  int rc = mat_queue_head(R, 2);
  if (rc != KMX_OK) return rc;
  if (own_p) KMX_HIP(ctx, hipMemsetAsync(R->d_present, 0, 4 * cells, st));
  if (own_z) KMX_HIP(ctx, hipMemsetAsync(R->d_size, 0, 4ull * G, st));
  if (own_s) KMX_HIP(ctx, hipMemsetAsync(R->d_sums, 0, 8 * cells, st));
  if (n_rows) {
    const u32 cus = gs_cus(ctx);
    const RowPlan p = mat_row_plan(M, n_rows, cus, GS_WAVES_PER_SIMD);
    const u32 grid = (u32)std::min<u64>((p.chunks + 3) / 4, gs_grid(std::min<u64>((u64)cus * GS_WGS_PER_CU, GS_MAX_GRID)));
#define GS_LAUNCH(C, S)                                                                                                                          \
  hipLaunchKernelGGL((k_gs_rows<C, S>), dim3(grid), dim3(256), 0, st, (const u8*)T->rows, n_rows, R->row_bytes, skip, N, M, p.L, p.RW, (const u32*)d_colt, \
                     d_groups, T->min_abund, T->g0, G, R->d_present, R->d_sums, R->d_size)
    if (!count) GS_LAUNCH(false, false);
    else if (sm) GS_LAUNCH(true, true);
    else GS_LAUNCH(true, false);
#undef GS_LAUNCH
    KMX_HIP(ctx, hipGetLastError());
  }
  return mat_queue_tail(R);
}

extern "C" int kmx_groupsum_dev(kmx_ctx* ctx, const kmx_groupsum_task* task, kmx_groupsum_result** out)
{ return mat_call(ctx, task, out, false, "kmx_groupsum_dev", "kmx_groupsum", groupsum_check, groupsum_queue<false>); }
extern "C" int kmx_groupsum_host(kmx_ctx* ctx, const kmx_groupsum_task* task, kmx_groupsum_result** out)
{ return mat_call(ctx, task, out, true, "kmx_groupsum_host", "kmx_groupsum", groupsum_check, groupsum_queue<true>); }

extern "C" int kmx_groupsum_result_wait(kmx_groupsum_result* R) { return mat_wait(R); }
extern "C" uint32_t* kmx_groupsum_result_present_dev(kmx_groupsum_result* R) { return mat_wait(R) == KMX_OK ? R->d_present : nullptr; }
extern "C" uint64_t* kmx_groupsum_result_sums_dev(kmx_groupsum_result* R) { return mat_wait(R) == KMX_OK ? (uint64_t*)R->d_sums : nullptr; }
extern "C" uint32_t* kmx_groupsum_result_size_dev(kmx_groupsum_result* R) { return mat_wait(R) == KMX_OK ? R->d_size : nullptr; }
extern "C" int kmx_groupsum_result_copy_present(kmx_groupsum_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_present, (u64)R->G * R->n_use, 4) : KMX_E_INVAL; }
extern "C" int kmx_groupsum_result_copy_sums(kmx_groupsum_result* R, uint64_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_sums, (u64)R->G * R->n_use, 8, "kmx_groupsum_result_copy_sums: the call was made without KMX_GROUPSUM_SUMS") : KMX_E_INVAL; }
extern "C" int kmx_groupsum_result_copy_size(kmx_groupsum_result* R, uint32_t* host_dst, uint64_t dst_entries)
{ return R ? mat_copy_out(R, host_dst, dst_entries, R->d_size, R->G, 4) : KMX_E_INVAL; }
extern "C" double kmx_groupsum_result_kernel_ms(kmx_groupsum_result* R) { return mat_kernel_ms(R); }
extern "C" uint64_t kmx_groupsum_result_algo_bytes(kmx_groupsum_result* R)
{
  if (mat_wait(R) != KMX_OK) return 0;
  const u64 cells = (u64)R->G * R->n_use;
  return R->n_rows * (R->row_bytes + 4) + 4ull * R->G + 4 * cells + (R->want_sums ? 8 * cells : 0);
}
extern "C" void kmx_groupsum_result_free(kmx_groupsum_result* R) { mat_free(R); }
