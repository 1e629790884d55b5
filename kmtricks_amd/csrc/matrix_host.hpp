// matrix_host.hpp -- the host path the calls of libkmx share that take a matrix body (or a list of keys, or reads against a set) and give
// tables, kept rows or records: kmx_select_*, kmx_colsums_*, kmx_diff_*, kmx_dist_*, kmx_pan_*, kmx_colors_*, kmx_gram_*, kmx_assoc_*,
// kmx_spectra_* and kmx_groupsum_* through mat_call; kmx_filter_*, kmx_combine_*, kmx_unitigs_*, kmx_kset_* and kmx_match_* with an entry
// of their own (their inputs are not one body) over the same parts.  A family (select.hip, diff.hip, dist.hip, pan.hip, colors.hip,
// gram.hip, assoc.hip, spectra.hip, groupsum.hip; filter.hip, combine.hip, unitigs.hip, match.hip) keeps what is its own: its extra
// limits, its blocks and their sizes, its launches, its formula for algo_bytes and its accessors.  Everything else is here, once.
#pragma once
#include "kmx_host.hpp"

#include <algorithm>
#include <initializer_list>

#pragma GCC visibility push(hidden)      // internal to libkmx: none of this joins the library's dynamic symbols
namespace kmx {

// what the result types have in common; kmx_select_result and its siblings derive from it
struct MatResult {
  kmx_ctx* ctx = nullptr;
  const char* name = "";                // "kmx_select", ...: leads the message of wait
  u64 n_rows = 0, row_bytes = 0;        // the body as it came in
  u32 n_cols = 0;
  hipEvent_t ev_in = nullptr, ev_done = nullptr, ev[5] = {};      // ev: the first n_ev are the family's profiling events, start ... end
  int n_ev = 2;
  bool waited = false; int status = KMX_OK;
  hipError_t up_err = hipSuccess;       // _host calls: the first upload that failed (mat_upload)
  void* d_in = nullptr;                 // _host calls: the upload
  std::vector<void*> scratch, owned;    // pool blocks that go back at wait / at free; a table the caller handed in is on neither
  bool nomem = false;                   // a block of the two lists could not be had
  std::vector<void*> pinned;            // page-locked buffers: tables on their way up, totals on their way down
  u32* h_tot = nullptr;                 // one of them: what mat_queue_tail reads back

  void* take(std::vector<void*>& list, u64 bytes)
  {
    void* p = ctx->dalloc(bytes);
    if (p) list.push_back(p); else nomem = true;
    return p;
  }
  void* tmp(u64 bytes) { return take(scratch, bytes); }
  void* keep(u64 bytes) { return take(owned, bytes); }
  void* pin(u64 bytes)                  // nullptr: none to be had
  {
    void* p = ctx->halloc(bytes);
    if (p) pinned.push_back(p);
    return p;
  }
};

// the limits the families share, each with its one message; every test returns KMX_OK or the refusal.  The words that differ between
// families are arguments.
struct MatCheck {
  kmx_ctx* ctx; std::string w;
  int no(int code, const std::string& what) const { return ctx->fail(code, w + what); }
  static bool is_bloom(u32 m) { return m == KMX_MODE_BF || m == KMX_MODE_BFC || m == KMX_MODE_BFT; }
  static u64 row_bytes(u32 key_words, u32 mode, u32 n_cols) { return 8ull * key_words + (mode == KMX_MODE_COUNT ? 4ull * n_cols : ((u64)n_cols + 7) / 8); }
  int n_cols(u32 n) const { return n == 0 ? no(KMX_E_INVAL, ": a matrix has at least one column") : KMX_OK; }
  int n_cols(u32 n, u32 m, const char* list) const      // list: "list", "selection"
  { return n == 0 || m == 0 ? no(KMX_E_INVAL, std::string(": a matrix has at least one column, and so has the ") + list) : KMX_OK; }
  int no_bloom(u32 mode, const char* why) const         // why: "", or ": " and what a Bloom row lacks
  { return is_bloom(mode) ? no(KMX_E_UNSUPPORTED, std::string(": Bloom filter bodies are not supported") + why + " (KMX_MODE_COUNT and KMX_MODE_PA only)") : KMX_OK; }
  int mode(u32 m) const { return m != KMX_MODE_COUNT && m != KMX_MODE_PA ? no(KMX_E_INVAL, ": mode must be KMX_MODE_COUNT or KMX_MODE_PA") : KMX_OK; }
  int key_words(u32 kw) const { return kw < 1 || kw > 4 ? no(KMX_E_INVAL, ": key_words must be 1 ... 4") : KMX_OK; }
  int min_abund(u32 a, u32 mode) const
  {
    if (a == 0) return no(KMX_E_INVAL, ": min_abund must be at least 1");
    return a > 1 && mode == KMX_MODE_PA ? no(KMX_E_INVAL, ": min_abund above 1 needs counts") : KMX_OK;
  }
  int flags(u32 f, u32 known) const { return f & ~known ? no(KMX_E_INVAL, ": unknown flag bits") : KMX_OK; }
  int list_fits(u32 m, u32 n, const char* kind) const      // kind: "output", "listed"
  { return m > n ? no(KMX_E_INVAL, std::string(": more ") + kind + " columns than input columns") : KMX_OK; }
  int identity(const void* cols, u32 m, u32 n, const char* field) const      // field: "n_out", "n_use"
  { return !cols && m != n ? no(KMX_E_INVAL, std::string(": cols = NULL is the identity and needs ") + field + " = n_cols") : KMX_OK; }
  int row_fits(u64 bytes) const { return bytes > 0xFFFFFFFFull ? no(KMX_E_UNSUPPORTED, ": rows of 4 GiB and more") : KMX_OK; }
  int n_rows(u64 n) const { return n > 0xFFFFFF00ull ? no(KMX_E_UNSUPPORTED, ": more than 2^32 - 256 rows in one call (send the body in runs of rows)") : KMX_OK; }
  int rows(u64 n, const void* p) const { return n && !p ? no(KMX_E_INVAL, ": null rows") : KMX_OK; }
  int col_list(const uint32_t* cols, u32 m, u32 n) const      // (m >= 1: n_cols)
  {
    if (!cols) return KMX_OK;
    std::vector<u32> s(cols, cols + m);
    std::sort(s.begin(), s.end());
    if (s.back() >= n) return no(KMX_E_INVAL, ": a column index at or above n_cols");
    return std::adjacent_find(s.begin(), s.end()) != s.end() ? no(KMX_E_INVAL, ": a column is listed twice") : KMX_OK;
  }
};

// every block, page-locked buffer and event back, R deleted
template <class Result> void mat_release(Result* R)
{
  kmx_ctx* c = R->ctx;
  for (void* p : R->scratch) c->dfree(p);
  for (void* p : R->owned) c->dfree(p);
  c->dfree(R->d_in);
  for (void* p : R->pinned) c->hfree(p);
  for (hipEvent_t e : {R->ev_in, R->ev_done, R->ev[0], R->ev[1], R->ev[2], R->ev[3], R->ev[4]}) if (e) (void)hipEventDestroy(e);
  delete R;
}

// ---- a _host call's inputs on their way up: every copy on ctx->up, then ctx->stream waits for them all.  An error stays with R
//      (the copies behind it are not queued) and is mat_uploads_done's refusal ----
inline void mat_upload(MatResult* R, void* dst, const void* src, u64 bytes)
{
  if (R->up_err == hipSuccess && bytes) R->up_err = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, R->ctx->up);
}
// ... into a scratch block of its own, which goes back at wait; nullptr: none to be had (R->nomem)
inline void* mat_upload_tmp(MatResult* R, const void* src, u64 bytes)
{
  void* d = R->tmp(bytes);
  if (d) mat_upload(R, d, src, bytes);
  return d;
}
inline int mat_uploads_done(MatResult* R, const char* who)
{
  kmx_ctx* ctx = R->ctx;
  hipError_t e = R->up_err;
  if (e == hipSuccess) e = hipEventCreateWithFlags(&R->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(R->ev_in, ctx->up);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, R->ev_in, 0);
  return e == hipSuccess ? KMX_OK : ctx->fail(KMX_E_HIP, std::string(who) + ": upload: " + hipGetErrorString(e));
}
// the end of every entry point: R handed out, or both streams (host: ctx->up too) waited for and R released
template <class Result> int mat_finish(int rc, Result* R, Result** out, bool host)
{
  if (rc == KMX_OK) { *out = R; return KMX_OK; }
  if (host) (void)hipStreamSynchronize(R->ctx->up);
  (void)hipStreamSynchronize(R->ctx->stream);
  mat_release(R);
  return rc;
}

// ---- the entry point: null arguments, the family's check (it gives the bytes of a row), a new result, for a _host call the body
//      (n_rows * row_bytes bytes) up, the family's queue.  who: "kmx_select_dev", ...; name: "kmx_select", ... ----
template <class Result, class Task>
int mat_call(kmx_ctx* ctx, const Task* task, Result** out, bool host, const char* who, const char* name,
             int (*check)(kmx_ctx*, const Task*, const char*, u64*), int (*queue)(kmx_ctx*, const Task*, Result*))
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, std::string(who) + ": null argument");
  *out = nullptr;
  u64 row_bytes = 0;
  int rc = check(ctx, task, who, &row_bytes);
  if (rc != KMX_OK) return rc;
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  Result* R = new Result();
  R->ctx = ctx; R->name = name; R->n_rows = task->n_rows; R->row_bytes = row_bytes; R->n_cols = task->n_cols;
  Task dt = *task;
  const u64 bytes = task->n_rows * row_bytes;
  if (host && bytes) {
    if (!(R->d_in = ctx->dalloc(bytes))) rc = ctx->fail(KMX_E_NOMEM, std::string(who) + ": upload allocation failed (send the body in runs of rows)");
    else {
      mat_upload(R, R->d_in, task->rows, bytes);
      rc = mat_uploads_done(R, who);
      dt.rows = R->d_in;
    }
  }
  if (rc == KMX_OK) rc = queue(ctx, &dt, R);
  return mat_finish(rc, R, out, host);
}

// ---- X_queue: the family takes its buffers and blocks (R->pin, R->tmp, R->keep) and uploads its tables, then mat_queue_head, its clears
//      and launches (with the events between the first and the last), mat_queue_tail ----
// head: with profiling on the family's n_ev events, the first recorded
inline int mat_queue_head(MatResult* R, int n_ev = 2)
{
  kmx_ctx* ctx = R->ctx;
  R->n_ev = n_ev;
  if (ctx->profiling) {
    for (int i = 0; i < n_ev; i++) KMX_HIP(ctx, hipEventCreate(&R->ev[i]));
    KMX_HIP(ctx, hipEventRecord(R->ev[0], ctx->stream));
  }
  return KMX_OK;
}
// tail: with profiling on the last event, h_tot[0] read back from d_tot (and h_tot[1] from d_more), ev_done
inline int mat_queue_tail(MatResult* R, const u32* d_tot = nullptr, const u32* d_more = nullptr)
{
  kmx_ctx* ctx = R->ctx;
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev[R->n_ev - 1], ctx->stream));
  if (d_tot) KMX_HIP(ctx, hipMemcpyAsync(&R->h_tot[0], d_tot, 4, hipMemcpyDeviceToHost, ctx->stream));
  if (d_more) KMX_HIP(ctx, hipMemcpyAsync(&R->h_tot[1], d_more, 4, hipMemcpyDeviceToHost, ctx->stream));
  KMX_HIP(ctx, hipEventCreateWithFlags(&R->ev_done, hipEventDisableTiming));
  KMX_HIP(ctx, hipEventRecord(R->ev_done, ctx->stream));
  return KMX_OK;
}

// ---- the result calls ----
inline int mat_wait(MatResult* R)
{
  if (!R) return KMX_E_INVAL;
  if (R->waited) return R->status;
  R->waited = true;
  const hipError_t e = hipEventSynchronize(R->ev_done);
  if (e != hipSuccess) return R->status = R->ctx->fail(KMX_E_HIP, std::string(R->name) + ": " + hipGetErrorString(e));
  // the call has run: its scratch and the upload go back to the pool; the owned blocks stay
  kmx_ctx* c = R->ctx;
  for (void* p : R->scratch) c->dfree(p);
  R->scratch.clear();
  c->dfree(R->d_in); R->d_in = nullptr;
  return R->status = KMX_OK;
}
// waits; entries * entry_bytes bytes of src to dst.  no_src: the refusal for a table the call did not make
inline int mat_copy_out(MatResult* R, void* dst, u64 dst_entries, const void* src, u64 entries, u32 entry_bytes, const char* no_src = nullptr)
{
  if (!R) return KMX_E_INVAL;
  const int rc = mat_wait(R);
  if (rc != KMX_OK) return rc;
  if (!src && no_src) return R->ctx->fail(KMX_E_INVAL, no_src);
  if (dst_entries < entries) return R->ctx->fail(KMX_E_INVAL, "destination too small");
  if (!entries) return KMX_OK;
  if (!dst) return R->ctx->fail(KMX_E_INVAL, "null destination");
  return kmx_copy_to_host(R->ctx, dst, src, (u64)entry_bytes * entries);
}
inline double mat_kernel_ms(MatResult* R)
{
  if (!R || !R->ev[0] || !R->ev[R->n_ev - 1] || mat_wait(R) != KMX_OK) return -1.0;
  float ms = 0;
  return hipEventElapsedTime(&ms, R->ev[0], R->ev[R->n_ev - 1]) == hipSuccess ? (double)ms : -1.0;
}
// part i lies between events i and i + 1; -1 without profiling, or where the call was not asked for the part (bit i of `made` is 0)
inline int mat_kernel_parts_ms(MatResult* R, std::initializer_list<double*> parts, u32 made = ~0u)
{
  for (double* p : parts) if (p) *p = -1.0;
  if (!R) return KMX_E_INVAL;
  if (!R->ev[0] || !R->ev[R->n_ev - 1] || mat_wait(R) != KMX_OK) return KMX_OK;
  int i = 0;
  for (double* p : parts) {
    float ms = 0;
    if (p && ((made >> i) & 1u) && hipEventElapsedTime(&ms, R->ev[i], R->ev[i + 1]) == hipSuccess) *p = (double)ms;
    i++;
  }
  return KMX_OK;
}
template <class Result> void mat_free(Result* R)
{
  if (!R) return;
  (void)hipSetDevice(R->ctx->device);
  if (R->ev_done) (void)hipEventSynchronize(R->ev_done);
  mat_release(R);
}

// ---- the launch plan of the kernels that give a row to L lanes: L the power of two at or above the row's units, 64 at the most; a wave
//      takes a chunk of RW rows -- 64, or with L == 64 as few (4 at the least) as it takes for the chip to have `waves` waves a SIMD ----
inline u32 pow2_at_or_above(u64 x, u32 cap) { u32 p = 1; while (p < cap && p < x) p <<= 1; return p; }
struct RowPlan { u32 L, RW; u64 chunks; };
inline RowPlan mat_row_plan(u64 units, u64 n_rows, u32 cus, u32 waves)
{
  RowPlan p{pow2_at_or_above(units, 64), 64, 0};
  if (p.L == 64) while (p.RW > 4 && n_rows / p.RW < (u64)cus * 4 * waves) p.RW >>= 1;
  p.chunks = (n_rows + p.RW - 1) / p.RW;
  return p;
}

}  // namespace kmx
#pragma GCC visibility pop
