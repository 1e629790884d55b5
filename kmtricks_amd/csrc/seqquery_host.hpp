// seqquery_host.hpp -- the host path the four sequence-query calls share (kmx_query_*, kmx_zquery_*, kmx_kquery_*, kmx_cquery_*):
// reads, a repartition table and one matrix body a partition go in, per-query tables come out.  A family (query.hip, zquery.hip,
// kquery.hip, cquery.hip) keeps what is its own: its extra limits, its blocks and their clears, its launches, its formula for
// algo_bytes and its accessors.  Everything else is here, once.
#pragma once
#include "kmx_host.hpp"

#include <cstring>

#pragma GCC visibility push(hidden)      // internal to libkmx: none of this joins the library's dynamic symbols
namespace kmx {

// what the four result types have in common; kmx_query_result and its siblings derive from it
struct SeqResult {
  kmx_ctx* ctx = nullptr;
  const char* name = "";                // "kmx_query", ...: leads the messages of wait and of a failed allocation
  u64 n_seqs = 0, n_bases = 0;
  u32 n_cols = 0, n_parts = 0;
  hipEvent_t ev_in = nullptr, ev_done = nullptr, ev0 = nullptr, ev1 = nullptr;
  bool waited = false; int status = KMX_OK;
  std::vector<void*> d_in;              // _host calls: the uploads
  const u8** h_rows = nullptr;          // page-locked: the row pointers (kquery: and the partitions' rows as u32 behind them) on their way up
  const u8** d_rows = nullptr;
  u32* h_tot = nullptr;                 // page-locked: the totals read back at the end of the call ([0] valid k-mers, but see zquery)
  std::vector<void*> scratch, owned;    // pool blocks that go back at wait / at free (the tables a kept result accumulates into)
  bool nomem = false;                   // a block of the two lists could not be had

  void* take(std::vector<void*>& list, u64 bytes)
  {
    void* p = ctx->dalloc(bytes);
    if (p) list.push_back(p); else nomem = true;
    return p;
  }
  void* tmp(u64 bytes) { return take(scratch, bytes); }
  void* keep(u64 bytes) { return take(owned, bytes); }
  template <class Task> void init(kmx_ctx* c, const char* family, const Task& K, u64 bases)
  { ctx = c; name = family; n_seqs = K.n_seqs; n_bases = bases; n_cols = K.n_cols; n_parts = K.nb_parts; }
};

// the limits the families share, each with its one message; every test returns KMX_OK or the refusal
struct SeqCheck {
  kmx_ctx* ctx; std::string w;
  int no(int code, const char* what) const { return ctx->fail(code, w + what); }
  int kmer_size(u32 k) const { return k < 8 || k > 127 ? no(KMX_E_INVAL, ": kmer_size must be in [8, 127]") : KMX_OK; }
  int minim_size(u32 m, u32 k) const { return m < 4 || m > 15 || m >= k ? no(KMX_E_INVAL, ": minim_size must be in [4, 15] and below kmer_size") : KMX_OK; }
  int nb_parts(u32 p) const { return p < 1 || p > 65535 ? no(KMX_E_INVAL, ": nb_parts must be in [1, 65535]") : KMX_OK; }
  int n_cols(u32 n) const { return n == 0 ? no(KMX_E_INVAL, ": a matrix has at least one column") : KMX_OK; }
  int tables(const void* repart, const void* rows) const { return !repart || !rows ? no(KMX_E_INVAL, ": null repartition table or row pointer array") : KMX_OK; }
  int reads(const void* offsets, u64 n_seqs, const void* bases) const { return !offsets || (n_seqs && !bases) ? no(KMX_E_INVAL, ": null reads") : KMX_OK; }
  int window(u64 w_) const { return w_ == 0 ? no(KMX_E_INVAL, ": a window has at least one row") : KMX_OK; }
  int window_fits(u64 w_) const { return w_ > 0xFFFFFFFFull ? no(KMX_E_UNSUPPORTED, ": windows of 2^32 rows and more") : KMX_OK; }
  int n_seqs(u64 n) const { return n >= (1ull << 31) ? no(KMX_E_UNSUPPORTED, ": 2^31 queries and more in one call (send them in batches)") : KMX_OK; }
  int row_fits(u64 bytes) const { return bytes > 0xFFFFFFFFull ? no(KMX_E_UNSUPPORTED, ": rows of 4 GiB and more") : KMX_OK; }
};

// the query section's limits, in its order (kmx_query_*; kmx_zquery_* applies them before its own)
template <class Task> int seq_check_bloom(kmx_ctx* ctx, const Task* K, const char* who)
{
  const SeqCheck c{ctx, who};
  int rc;
  if ((rc = c.kmer_size(K->kmer_size)) || (rc = c.minim_size(K->minim_size, K->kmer_size)) || (rc = c.nb_parts(K->nb_parts)) || (rc = c.n_cols(K->n_cols)) ||
      (rc = c.tables(K->repart, K->rows)) || (rc = c.reads(K->offsets, K->n_seqs, K->bases)) || (rc = c.window(K->window)) || (rc = c.window_fits(K->window)) ||
      (rc = c.n_seqs(K->n_seqs))) return rc;
  return KMX_OK;
}

// ---- the entry points: X_call(ctx, task, out, host, who) is seq_args, the family's check, seq_n_bases, a new result, seq_upload (host),
//      the family's queue and seq_finish ----
template <class Result> int seq_args(kmx_ctx* ctx, const void* task, Result** out, const char* who)
{
  if (!ctx) return KMX_E_INVAL;
  if (!task || !out) return ctx->fail(KMX_E_INVAL, std::string(who) + ": null argument");
  *out = nullptr;
  return KMX_OK;
}
// the end of the last query (the grid's size).  host: from offsets, which must start at 0 and not descend; else read back from the
// device (8 bytes: the call's first GPU work).  2^32 bases and more are refused.
inline int seq_n_bases(kmx_ctx* ctx, const uint64_t* offsets, u64 n_seqs, bool host, const char* who, u64* n_bases)
{
  const std::string w(who);
  if (host) {
    if (offsets[0] != 0) return ctx->fail(KMX_E_INVAL, w + ": offsets[0] must be 0");
    for (u64 i = 0; i < n_seqs; i++) if (offsets[i] > offsets[i + 1]) return ctx->fail(KMX_E_INVAL, w + ": offsets must not descend");
    *n_bases = offsets[n_seqs];
  } else {
    KMX_HIP(ctx, hipSetDevice(ctx->device));
    KMX_HIP(ctx, hipMemcpyAsync(n_bases, offsets + n_seqs, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (*n_bases > 0xFFFFFFFFull) return ctx->fail(KMX_E_UNSUPPORTED, w + ": 2^32 bases and more in one call (send the queries in batches)");
  return KMX_OK;
}

// a _host call: bases, offsets, the repartition table and the rows of every partition of the call (part_bytes(p) bytes) go up on
// ctx->up and take their places in *dt (drows, nb_parts null pointers of the caller's, holds dt->rows while the call is queued);
// ctx->stream waits for them
template <class Task, class PartBytes>
int seq_upload(SeqResult* R, Task* dt, std::vector<const uint8_t*>& drows, const char* who, PartBytes part_bytes)
{
  kmx_ctx* ctx = R->ctx;
  const std::string w(who);
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  hipError_t e = hipSuccess;
  auto upload = [&](const void* src, u64 bytes) -> void* {
    void* d = ctx->dalloc(bytes);
    if (!d) return nullptr;
    R->d_in.push_back(d);
    if (bytes && e == hipSuccess) e = hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->up);
    return d;
  };
  const uint8_t* const* rows = dt->rows;
  if (!(dt->bases = (const char*)upload(dt->bases, R->n_bases)) || !(dt->offsets = (const uint64_t*)upload(dt->offsets, 8 * (dt->n_seqs + 1))) ||
      !(dt->repart = (const uint16_t*)upload(dt->repart, 2ull << (2 * dt->minim_size))))
    return ctx->fail(KMX_E_NOMEM, w + ": upload allocation failed");
  for (u32 p = 0; p < dt->nb_parts; p++) {
    if (!rows[p]) continue;
    if (!(drows[p] = (const uint8_t*)upload(rows[p], part_bytes(p)))) return ctx->fail(KMX_E_NOMEM, w + ": upload allocation failed");
  }
  dt->rows = drows.data();
  if (e == hipSuccess) e = hipEventCreateWithFlags(&R->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(R->ev_in, ctx->up);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, R->ev_in, 0);
  if (e != hipSuccess) return ctx->fail(KMX_E_HIP, w + ": upload: " + hipGetErrorString(e));
  return KMX_OK;
}

// every block, page-locked buffer and event back, R deleted
template <class Result> void seq_release(Result* R)
{
  kmx_ctx* c = R->ctx;
  for (void* p : R->scratch) c->dfree(p);
  for (void* p : R->owned) c->dfree(p);
  for (void* p : R->d_in) c->dfree(p);
  c->hfree(R->h_tot); c->hfree((void*)R->h_rows);
  for (hipEvent_t e : {R->ev_in, R->ev_done, R->ev0, R->ev1}) if (e) (void)hipEventDestroy(e);
  delete R;
}
// rc == KMX_OK: the result is the caller's.  Else both streams (host: ctx->up too) are waited for and the result is released.
template <class Result> int seq_finish(Result* R, int rc, bool host, Result** out)
{
  if (rc == KMX_OK) { *out = R; return KMX_OK; }
  if (host) (void)hipStreamSynchronize(R->ctx->up);
  (void)hipStreamSynchronize(R->ctx->stream);
  seq_release(R);
  return rc;
}

// ---- X_queue: the family takes its blocks (R->tmp, R->keep), then seq_queue_head, its clears and launches, seq_queue_tail ----
// head: h_tot (tot_bytes, zeroed) and the row pointers page-locked -- with n_rows the partitions' rows follow them as u32, 12 bytes a
// partition in all --, d_rows taken and uploaded, the allocations of the call checked, ev0 with profiling on
inline int seq_queue_head(SeqResult* R, const uint8_t* const* rows, const uint64_t* n_rows, u64 tot_bytes)
{
  kmx_ctx* ctx = R->ctx;
  const u32 P = R->n_parts;
  const u64 rows_bytes = (n_rows ? 12ull : 8ull) * P;
  if (!(R->h_tot = (u32*)ctx->halloc(tot_bytes)) || !(R->h_rows = (const u8**)ctx->halloc(rows_bytes)))
    return ctx->fail(KMX_E_NOMEM, std::string(R->name) + ": host allocation failed");
  memset(R->h_tot, 0, tot_bytes);
  u32* h_nrows = (u32*)(R->h_rows + P);
  for (u32 p = 0; p < P; p++) {
    R->h_rows[p] = rows[p];
    if (n_rows) h_nrows[p] = rows[p] ? (u32)n_rows[p] : 0u;
  }
  R->d_rows = (const u8**)R->tmp(rows_bytes);
  if (R->nomem) return ctx->fail(KMX_E_NOMEM, std::string(R->name) + ": device allocation failed");
  KMX_HIP(ctx, hipMemcpyAsync((void*)R->d_rows, (const void*)R->h_rows, rows_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (ctx->profiling) {
    KMX_HIP(ctx, hipEventCreate(&R->ev0)); KMX_HIP(ctx, hipEventCreate(&R->ev1));
    KMX_HIP(ctx, hipEventRecord(R->ev0, ctx->stream));
  }
  return KMX_OK;
}
// tail: ev1 with profiling on, h_tot[0 .. n_tot) read back from d_tot (and h_tot[n_tot] from d_more), ev_done
inline int seq_queue_tail(SeqResult* R, const u32* d_tot, u32 n_tot, const u32* d_more = nullptr)
{
  kmx_ctx* ctx = R->ctx;
  if (ctx->profiling) KMX_HIP(ctx, hipEventRecord(R->ev1, ctx->stream));
  KMX_HIP(ctx, hipMemcpyAsync(R->h_tot, d_tot, 4ull * n_tot, hipMemcpyDeviceToHost, ctx->stream));
  if (d_more) KMX_HIP(ctx, hipMemcpyAsync(R->h_tot + n_tot, d_more, 4, hipMemcpyDeviceToHost, ctx->stream));
  KMX_HIP(ctx, hipEventCreateWithFlags(&R->ev_done, hipEventDisableTiming));
  KMX_HIP(ctx, hipEventRecord(R->ev_done, ctx->stream));
  return KMX_OK;
}

// ---- the result calls ----
inline int seq_wait(SeqResult* R)
{
  if (!R) return KMX_E_INVAL;
  if (R->waited) return R->status;
  R->waited = true;
  const hipError_t e = hipEventSynchronize(R->ev_done);
  if (e != hipSuccess) return R->status = R->ctx->fail(KMX_E_HIP, std::string(R->name) + ": " + hipGetErrorString(e));
  // the call has run: its scratch and uploads go back to the pool; the owned tables stay (a result kept as the accumulator of later
  // partition groups holds nothing else)
  kmx_ctx* c = R->ctx;
  for (void* p : R->scratch) c->dfree(p);
  for (void* p : R->d_in) c->dfree(p);
  R->scratch.clear(); R->d_in.clear(); R->d_rows = nullptr;
  c->hfree((void*)R->h_rows); R->h_rows = nullptr;
  return R->status = KMX_OK;
}
// waits; entries * entry_bytes bytes of src to dst.  no_src: the refusal for a table the call did not make
inline int seq_copy_out(SeqResult* R, void* dst, u64 dst_entries, const void* src, u64 entries, u32 entry_bytes, const char* no_src = nullptr)
{
  if (!R) return KMX_E_INVAL;
  const int rc = seq_wait(R);
  if (rc != KMX_OK) return rc;
  if (dst_entries < entries) return R->ctx->fail(KMX_E_INVAL, "destination too small");
  if (!entries) return KMX_OK;
  if (!dst) return R->ctx->fail(KMX_E_INVAL, "null destination");
  if (!src && no_src) return R->ctx->fail(KMX_E_INVAL, no_src);
  return kmx_copy_to_host(R->ctx, dst, src, (u64)entry_bytes * entries);
}
inline double seq_kernel_ms(SeqResult* R)
{
  if (!R || !R->ev0 || !R->ev1 || seq_wait(R) != KMX_OK) return -1.0;
  float ms = 0;
  return hipEventElapsedTime(&ms, R->ev0, R->ev1) == hipSuccess ? (double)ms : -1.0;
}
template <class Result> void seq_free(Result* R)
{
  if (!R) return;
  (void)hipSetDevice(R->ctx->device);
  if (R->ev_done) (void)hipEventSynchronize(R->ev_done);
  seq_release(R);
}

}  // namespace kmx
#pragma GCC visibility pop
