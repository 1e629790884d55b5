// kmx_api.hip -- C ABI of libkmx (include/kmx.h), the part no kernel belongs to (about 430 lines): context, device and pinned memory
// pools, stores, peer access, copies to the host, kmx_set_*.  The batch merge driver is merge_host.hip; every other call lies beside its kernels.
// No CPU fallback anywhere: every entry point needs a live HIP device.
#include "kmx_host.hpp"

#include <algorithm>
#include <chrono>
#include <sys/mman.h>
#include <unordered_map>
#include <mutex>
#include <cstdlib>
#include <cstring>

using namespace kmx;

static thread_local std::string g_create_err;

// ---- memory pools ----------------------------------------------------------------------------------
void* kmx_ctx::dalloc(size_t bytes)
{
  if (bytes == 0) bytes = 256;
  // (round 6) large blocks come in size classes an eighth of a power of two apart: the arenas of a job's batches differ by a few per cent
  // from batch to batch and from pass to pass (their size follows the running estimates), and a request a little above every free
  // block was a hipMalloc of 600 MB -- 18 ms with the GPU idle, in the middle of the whole-job figure (profiles/r06_whole_job_timeline.txt)
  if (bytes >= (8u << 20)) { size_t p2 = (size_t)1 << 23; while (p2 * 2 <= bytes) p2 *= 2; const size_t q = p2 >> 3; bytes = (bytes + q - 1) / q * q; }
  int best = -1;
  for (size_t i = 0; i < pool.size(); i++)
    if (!pool[i].used && pool[i].bytes >= bytes && pool[i].bytes <= 2 * bytes + (1u << 20) &&
        (best < 0 || pool[i].bytes < pool[best].bytes)) best = (int)i;
  if (best >= 0) { pool[best].used = true; return pool[best].p; }
  // a large block that has to be made is made as large as the largest one asked for so far (when that is within 1.5 x): after a few
  // batches every arena block of a job fits every arena request, and the pool stops growing (it had reached 104 GB in 431 blocks over
  // the whole job of configs[2], a quarter of it free, and still missed)
  if (bytes >= (64u << 20)) { big_max = std::max(big_max, bytes); if (big_max <= bytes + bytes / 2) bytes = big_max; }
  void* p = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  struct Tr { size_t b; std::chrono::steady_clock::time_point t; kmx_ctx* c; ~Tr() { static const bool on = getenv("KMX_TRACE") != nullptr || getenv("KMX_TRACE_ALLOC") != nullptr; if (on) { size_t fr = 0, tot = 0; for (auto& x : c->pool) { tot += x.bytes; if (!x.used) fr += x.bytes; }
    fprintf(stderr, "[kmx alloc] device pool +%zu MB: %.2f ms (pool %zu MB in %zu blocks, %zu MB of it free)\n", b >> 20, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(), tot >> 20, c->pool.size(), fr >> 20); } } } tr{bytes, t0, this};
  if (hipMalloc(&p, bytes) != hipSuccess) {
    // drop cached blocks and retry once
    for (auto& b : pool) if (!b.used && b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    pool.erase(std::remove_if(pool.begin(), pool.end(), [](const kmx_pool_block& b) { return b.p == nullptr; }), pool.end());
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  }
  pool.push_back({p, bytes, true});
  return p;
}
void kmx_ctx::dfree(void* p)
{
  if (!p) return;
  for (auto& b : pool) if (b.p == p) { b.used = false; return; }
}
void* kmx_ctx::halloc(size_t bytes)
{
  if (bytes == 0) bytes = 256;
  int best = -1;
  for (size_t i = 0; i < hpool.size(); i++)
    if (!hpool[i].used && hpool[i].bytes >= bytes && hpool[i].bytes <= 2 * bytes + (1u << 20) &&
        (best < 0 || hpool[i].bytes < hpool[best].bytes)) best = (int)i;
  if (best >= 0) { hpool[best].used = true; return hpool[best].p; }
  void* p = nullptr;
  p = kmx_pinned_alloc(bytes);
  if (!p) return nullptr;
  hpool.push_back({p, bytes, true});
  return p;
}
void kmx_ctx::hfree(void* p)
{
  if (!p) return;
  for (auto& b : hpool) if (b.p == p) { b.used = false; return; }
}

// ---- context -----------------------------------------------------------------------------------------
extern "C" int kmx_version(void) { return KMX_VERSION; }
extern "C" int kmx_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

extern "C" int kmx_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return KMX_E_NODEVICE;
  int cur = -1; (void)hipGetDevice(&cur);
  if (hipSetDevice(device) != hipSuccess) return KMX_E_NODEVICE;
  size_t fr = 0, tot = 0;
  const hipError_t e = hipMemGetInfo(&fr, &tot);
  if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
  if (e != hipSuccess) return KMX_E_HIP;
  if (free_bytes) *free_bytes = fr;
  if (total_bytes) *total_bytes = tot;
  return KMX_OK;
}

extern "C" uint64_t kmx_device_warm(int device, uint64_t bytes, const volatile int* stop)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n || bytes == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) return 0;
  const size_t piece = (size_t)1 << 30;
  std::vector<void*> held;
  uint64_t got = 0;
  while (got < bytes) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < tot / 4 + piece) break;      // (a quarter of the device stays free for whoever is working)
    if (stop && *stop) break;
    void* p = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipMalloc(&p, piece) != hipSuccess) { (void)hipGetLastError(); break; }
    held.push_back(p); got += piece;
    if (held.size() == 1 && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() < 5.0) break;      // (this memory has been handed out before)
  }
  for (void* p : held) (void)hipFree(p);
  return got;
}

extern "C" int kmx_create(int device, kmx_ctx** out)
{
  if (!out) { g_create_err = "kmx_create: out is NULL"; return KMX_E_INVAL; }
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_err = std::string("kmx_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                   "); libkmx has no CPU fallback";
    return KMX_E_NODEVICE;
  }
  if (device < 0 || device >= n) { g_create_err = "kmx_create: device index out of range"; return KMX_E_INVAL; }
  if ((e = hipSetDevice(device)) != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); return KMX_E_NODEVICE; }
  kmx_ctx* c = new kmx_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) { g_create_err = hipGetErrorString(e); delete c; return KMX_E_NODEVICE; }
  c->n_cu = prop.multiProcessorCount;
  { const char* fo = getenv("KMX_FILE_ORDER"); c->file_order = !(fo && fo[0] == '0'); }
  { const char* v = getenv("KMX_COLS_MIN_LISTS"); if (v && atoi(v) > 0) { c->cols_min_lists = (unsigned)atoi(v); c->cols_min_env = true; }
    v = getenv("KMX_COLS_MIN_LISTS_ORD"); if (v && atoi(v) > 0) { c->cols_min_lists_ord = (unsigned)atoi(v); c->cols_min_env = true; } }
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) { g_create_err = hipGetErrorString(e); delete c; return KMX_E_NODEVICE; }
  if ((e = hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking)) != hipSuccess) { g_create_err = hipGetErrorString(e); (void)hipStreamDestroy(c->stream); delete c; return KMX_E_NODEVICE; }
  if ((e = hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking)) != hipSuccess) { g_create_err = hipGetErrorString(e); (void)hipStreamDestroy(c->stream); (void)hipStreamDestroy(c->aux); delete c; return KMX_E_NODEVICE; }
  if ((e = hipStreamCreateWithFlags(&c->up, hipStreamNonBlocking)) != hipSuccess) { g_create_err = hipGetErrorString(e); (void)hipStreamDestroy(c->stream); (void)hipStreamDestroy(c->aux); (void)hipStreamDestroy(c->copy); delete c; return KMX_E_NODEVICE; }
  *out = c;
  return KMX_OK;
}

extern "C" void kmx_destroy(kmx_ctx* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipStreamSynchronize(ctx->aux);
  (void)hipStreamSynchronize(ctx->copy);
  (void)hipStreamSynchronize(ctx->up);
  for (auto& a : ctx->ahead) if (a.ev) (void)hipEventDestroy(a.ev);
  for (auto& e : ctx->copy_ev) if (e) (void)hipEventDestroy(e);
  for (auto& b : ctx->pool) if (b.p) (void)hipFree(b.p);
  if (ctx->d_hist) (void)hipFree(ctx->d_hist);
  if (ctx->d_rep) (void)hipFree(ctx->d_rep);
  if (ctx->d_stat) (void)hipFree(ctx->d_stat);
  for (auto& b : ctx->hpool) if (b.p) kmx_pinned_free(b.p);
  (void)hipStreamDestroy(ctx->stream);
  kmx_count_chain_forget(ctx);
  if (ctx->ev_split) (void)hipEventDestroy(ctx->ev_split);
  (void)hipStreamDestroy(ctx->aux);
  (void)hipStreamDestroy(ctx->copy);
  (void)hipStreamDestroy(ctx->up);
  delete ctx;
}

extern "C" const char* kmx_last_error(const kmx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }
extern "C" void* kmx_stream(kmx_ctx* ctx) { if (ctx) ctx->stream_shared = true; return ctx ? (void*)ctx->stream : nullptr; }
extern "C" void kmx_free(void* p) { free(p); }
// Page-locked host memory.  hipHostMalloc pins 4 KB pages one by one -- 5.6 ms for 32 MB, all of it under the runtime's lock, so
// that a thread pinning the pipeline's buffers stalls every other thread's launches and copies (the output ring, the read
// buffers).  An anonymous mapping backed by transparent huge pages, touched and then registered, is page-locked in 1.5 ms of which
// 0.1 ms are the runtime's (hipHostRegister over 16 pages of 2 MB instead of 8192 of 4 KB); device copies run at the same 55 GB/s
// (scripts/dev/pin_speed.hip).  Blocks of at least 2 MB take that road; smaller ones, and any failure on it, hipHostMalloc.
namespace {
std::mutex g_pin_mutex;
std::unordered_map<void*, size_t> g_pin_mapped;      // blocks that came from mmap + hipHostRegister: their mapped size
}
void* kmx_pinned_alloc(size_t bytes)
{
  if (bytes == 0) bytes = 256;
  static const bool thp_off = getenv("KMX_PINNED_HIPHOSTMALLOC") != nullptr;
  if (bytes >= (2u << 20) && !thp_off) {
    const size_t n = (bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
    void* q = mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (q != MAP_FAILED) {
      (void)madvise(q, n, MADV_HUGEPAGE);
      static const bool trace = getenv("KMX_TRACE") != nullptr;
      const auto t0 = std::chrono::steady_clock::now();
      for (size_t o = 0; o < n; o += 4096) static_cast<volatile char*>(q)[o] = 0;      // fault the pages in here, not under the runtime's lock
      const auto t1 = std::chrono::steady_clock::now();
      const hipError_t re = hipHostRegister(q, n, hipHostRegisterPortable);
      if (trace) fprintf(stderr, "[kmx alloc] pinned %zu MB: touch %.2f ms, register %.2f ms\n", n >> 20, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
      if (re == hipSuccess) {      // (portable: a process that drives several GPUs copies to and from it on all of them, as with hipHostMalloc)
        std::lock_guard<std::mutex> lk(g_pin_mutex);
        g_pin_mapped[q] = n;
        return q;
      }
      (void)hipGetLastError();
      munmap(q, n);
    }
  }
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}
void kmx_pinned_free(void* p)
{
  if (!p) return;
  size_t n = 0;
  { std::lock_guard<std::mutex> lk(g_pin_mutex); auto it = g_pin_mapped.find(p); if (it != g_pin_mapped.end()) { n = it->second; g_pin_mapped.erase(it); } }
  if (n) { (void)hipHostUnregister(p); munmap(p, n); }
  else (void)hipHostFree(p);
}
// [p, p + n) lies in a block kmx_alloc_pinned made by mapping + registering (2 MB and up): a copy from it is a DMA by itself
bool kmx_is_pinned(const void* p, size_t n)
{
  std::lock_guard<std::mutex> lk(g_pin_mutex);
  for (auto& b : g_pin_mapped) if ((const char*)p >= (const char*)b.first && (const char*)p + n <= (const char*)b.first + b.second) return true;
  return false;
}
extern "C" void* kmx_alloc_pinned(size_t bytes) { return kmx_pinned_alloc(bytes); }
extern "C" void kmx_free_pinned(void* p) { kmx_pinned_free(p); }
// ---- kmx_store: count lists resident in HBM between the count and the merge stage ---------------------------------
void kmx_store::start_ahead()
{
  if (ahead_on) return;
  ahead_on = true;
  const char* e = getenv("KMX_STORE_AHEAD");
  if (e && e[0] == '0') return;
  ahead = std::thread([this]() {
    (void)hipSetDevice(device);
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [this]() { return stop || spare.size() < 2; });
      if (stop) return;
      size_t held = 0; for (auto& c : chunks) held += c.cap; for (auto& c : spare) held += c.cap;
      if (limit && held + chunk_bytes > limit + chunk_bytes) { cv.wait_for(lk, std::chrono::milliseconds(50)); continue; }      // (at the limit: nothing more ahead)
      lk.unlock();
      void* p = nullptr;
      const auto t0 = std::chrono::steady_clock::now();
      const hipError_t er = hipMalloc(&p, chunk_bytes);
      { static const bool trace = getenv("KMX_TRACE") != nullptr; if (trace) fprintf(stderr, "[kmx alloc] store chunk ahead %zu MB: %.2f ms\n", chunk_bytes >> 20, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
      lk.lock();
      if (er != hipSuccess) { (void)hipGetLastError(); cv.wait_for(lk, std::chrono::milliseconds(200)); continue; }
      spare.push_back({(u8*)p, chunk_bytes, 0});
    }
  });
}
bool kmx_store::take_spare(size_t bytes, Chunk& out)
{
  if (bytes > chunk_bytes || spare.empty()) return false;
  out = spare.back(); spare.pop_back();
  cv.notify_one();
  return true;
}
void* kmx_store::alloc(size_t bytes)
{
  bytes = (bytes + 255) / 256 * 256;
  if (bytes == 0) bytes = 256;
  std::lock_guard<std::mutex> lk(mu);
  start_ahead();
  if (limit && used + bytes > limit) return nullptr;
  for (size_t i = 0; i < chunks.size(); i++) { auto& c = chunks[i]; if (!chunk_reserved(i) && c.cap - c.fill >= bytes) { void* p = c.p + c.fill; c.fill += bytes; used += bytes; return p; } }
  { Chunk sp; if (take_spare(bytes, sp)) { sp.fill = bytes; chunks.push_back(sp); used += bytes; return sp.p; } }
  int cur = -1; (void)hipGetDevice(&cur);
  if (cur != device && hipSetDevice(device) != hipSuccess) return nullptr;
  size_t cap = std::max(bytes, chunk_bytes);
  void* p = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipMalloc(&p, cap);
  if (e != hipSuccess && cap > bytes) { cap = bytes; e = hipMalloc(&p, cap); }      // (the device is nearly full: an exact block)
  { static const bool trace = getenv("KMX_TRACE") != nullptr; if (trace) fprintf(stderr, "[kmx alloc] store chunk %zu MB: %.2f ms\n", cap >> 20, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
  if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
  if (e != hipSuccess) return nullptr;
  chunks.push_back({(u8*)p, cap, bytes});
  used += bytes;
  return p;
}
void* kmx_store::try_reserve(size_t bytes)
{
  bytes = (bytes + 255) / 256 * 256;
  if (bytes == 0) bytes = 256;
  std::lock_guard<std::mutex> lk(mu);
  start_ahead();
  if (resvs.size() >= 8 || (limit && used + bytes > limit)) return nullptr;
  for (int pass = 0; pass < 2; pass++) {
    for (size_t i = 0; i < chunks.size(); i++) {
      auto& c = chunks[i];
      if (!chunk_reserved(i) && c.cap - c.fill >= bytes) { resvs.push_back({(int)i, c.fill, bytes}); void* p = c.p + c.fill; c.fill += bytes; used += bytes; return p; }
    }
    if (pass) break;
    // no free chunk with that much room: a new one, as alloc() makes it -- the one made ahead when there is one
    { Chunk sp; if (take_spare(bytes, sp)) { chunks.push_back(sp); continue; } }
    int cur = -1; (void)hipGetDevice(&cur);
    if (cur != device && hipSetDevice(device) != hipSuccess) return nullptr;
    const size_t cap = std::max(bytes, chunk_bytes);
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, cap);
    if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
    if (e != hipSuccess) { (void)hipGetLastError(); return nullptr; }      // (the device is nearly full: the caller waits for its size and takes exactly what it needs)
    chunks.push_back({(u8*)p, cap, 0});
  }
  return nullptr;
}
void kmx_store::commit(void* p, size_t used_bytes)
{
  used_bytes = (used_bytes + 255) / 256 * 256;
  std::lock_guard<std::mutex> lk(mu);
  for (size_t j = 0; j < resvs.size(); j++) {
    const Resv r = resvs[j];
    if (chunks[r.chunk].p + r.off != (u8*)p) continue;
    if (used_bytes > r.bytes) used_bytes = r.bytes;
    chunks[r.chunk].fill = r.off + used_bytes;      // (nothing was allocated behind the reservation: the chunk was left alone)
    used -= r.bytes - used_bytes;
    resvs.erase(resvs.begin() + j);
    return;
  }
}
extern "C" int kmx_store_create(int device, uint64_t limit_bytes, kmx_store** out)
{
  if (!out) return KMX_E_INVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { g_create_err = "kmx_store_create: no HIP device; libkmx has no CPU fallback"; return KMX_E_NODEVICE; }
  if (device < 0 || device >= n) { g_create_err = "kmx_store_create: device index out of range"; return KMX_E_INVAL; }
  int cur = -1; (void)hipGetDevice(&cur);
  if (hipSetDevice(device) != hipSuccess) { g_create_err = "kmx_store_create: hipSetDevice failed"; return KMX_E_NODEVICE; }
  size_t fr = 0, tot = 0;
  (void)hipMemGetInfo(&fr, &tot);
  if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
  kmx_store* s = new kmx_store();
  s->device = device;
  s->limit = limit_bytes ? (size_t)limit_bytes : (size_t)(tot / 10 * 6);
  s->chunk_bytes = (size_t)256 << 20;
  { const char* e = getenv("KMX_STORE_CHUNK_MB"); if (e && atol(e) >= 16 && atol(e) <= 65536) s->chunk_bytes = (size_t)atol(e) << 20; }
  *out = s;
  return KMX_OK;
}
extern "C" void kmx_store_destroy(kmx_store* s)
{
  if (!s) return;
  int cur = -1; (void)hipGetDevice(&cur);
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();
  { std::lock_guard<std::mutex> lk(s->mu); s->stop = true; }
  s->cv.notify_all();
  if (s->ahead.joinable()) s->ahead.join();
  for (auto& c : s->spare) (void)hipFree(c.p);
  for (auto& c : s->chunks) (void)hipFree(c.p);
  if (cur >= 0 && cur != s->device) (void)hipSetDevice(cur);
  delete s;
}
// ---- peer access between the GPUs of a node: a counting context on GPU a fills the store of GPU b with hipMemcpyPeerAsync.  With
//      peer access enabled that copy is one DMA over the xGMI link between the two; without it the runtime stages it through host
//      memory.  Asked for once per ordered pair, the outcome kept (and printed with KMX_TRACE=1): 1 direct, 0 staged. ----
namespace {
std::mutex g_peer_mutex;
signed char g_peer[64][64];      // 0 unknown, 1 enabled, -1 not available
}
int kmx_peer_path(int from, int to)
{
  if (from == to) return 1;
  if (from < 0 || to < 0 || from >= 64 || to >= 64) return 0;
  std::lock_guard<std::mutex> lk(g_peer_mutex);
  if (g_peer[from][to] == 0) {
    int can = 0, cur = -1;
    (void)hipGetDevice(&cur);
    signed char st = -1;
    if (hipDeviceCanAccessPeer(&can, from, to) == hipSuccess && can && hipSetDevice(from) == hipSuccess) {
      const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
      if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) st = 1;
      (void)hipGetLastError();
    }
    if (cur >= 0) (void)hipSetDevice(cur);
    g_peer[from][to] = st;
    if (getenv("KMX_TRACE")) fprintf(stderr, "[kmx] GPU %d -> GPU %d: %s\n", from, to, st == 1 ? "peer access enabled (copies go over xGMI)" : "no peer access (copies are staged through host memory)");
  }
  return g_peer[from][to] == 1 ? 1 : 0;
}
extern "C" int kmx_peer_access(int from_device, int to_device)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || from_device < 0 || to_device < 0 || from_device >= n || to_device >= n) return KMX_E_INVAL;
  return kmx_peer_path(from_device, to_device);
}
extern "C" uint64_t kmx_store_used(const kmx_store* s) { return s ? s->used : 0; }
extern "C" uint64_t kmx_store_limit(const kmx_store* s) { return s ? s->limit : 0; }
extern "C" int kmx_copy_to_host(kmx_ctx* ctx, void* dst, const void* src, uint64_t bytes)
{
  if (!ctx) return KMX_E_INVAL;
  if (!bytes) return KMX_OK;
  if (!dst || !src) return ctx->fail(KMX_E_INVAL, "kmx_copy_to_host: null pointer");
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  KMX_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->copy));
  KMX_HIP(ctx, hipStreamSynchronize(ctx->copy));
  return KMX_OK;
}

extern "C" int kmx_copy_to_host_async(kmx_ctx* ctx, void* dst, const void* src, uint64_t bytes, uint32_t* ticket)
{
  if (!ctx) return KMX_E_INVAL;
  if (!ticket || (bytes && (!dst || !src))) return ctx->fail(KMX_E_INVAL, "kmx_copy_to_host_async: null pointer");
  int slot = -1;
  for (int i = 0; i < 8; i++) if (!ctx->copy_out[i]) { slot = i; break; }
  if (slot < 0) return ctx->fail(KMX_E_INVAL, "kmx_copy_to_host_async: KMX_COPIES_AHEAD tickets are out already");
  KMX_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->copy_ev[slot]) KMX_HIP(ctx, hipEventCreateWithFlags(&ctx->copy_ev[slot], hipEventDisableTiming));
  if (bytes) KMX_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->copy));
  KMX_HIP(ctx, hipEventRecord(ctx->copy_ev[slot], ctx->copy));
  ctx->copy_out[slot] = true;
  *ticket = (uint32_t)slot;
  return KMX_OK;
}
extern "C" int kmx_copy_wait(kmx_ctx* ctx, uint32_t ticket)
{
  if (!ctx) return KMX_E_INVAL;
  if (ticket >= 8 || !ctx->copy_out[ticket]) return ctx->fail(KMX_E_INVAL, "kmx_copy_wait: no such ticket");
  ctx->copy_out[ticket] = false;
  KMX_HIP(ctx, hipEventSynchronize(ctx->copy_ev[ticket]));
  return KMX_OK;
}

extern "C" int kmx_set_profiling(kmx_ctx* ctx, int on) { if (!ctx) return KMX_E_INVAL; ctx->profiling = on != 0; return KMX_OK; }
extern "C" int kmx_set_file_order(kmx_ctx* ctx, int on) { if (!ctx) return KMX_E_INVAL; ctx->file_order = on != 0; return KMX_OK; }

