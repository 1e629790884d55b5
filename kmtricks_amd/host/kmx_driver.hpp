// kmx_driver.hpp -- what the commands of `kmx` that read a run's matrices share (select, dist, diff, pan, colors, pca, assoc, unitigs; query
// for the parts that fit its indexes): the reader of the command line's values, the run directory opened in steps -- the tools put checks
// of their own between them, and every one of them comes before kmx_create --, the --samples list, the devices and their budget, the
// shards' threads, the two-in-flight walk through a partition's runs of rows in its two shapes, and the text that goes to a file or to
// standard output.  A tool keeps its usage, its chain of options, its own refusals, its task and what it does with a result.
#pragma once
#include <kmx.h>
#include <algorithm>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include "kmx_io.hpp"
#include "kmx_run.hpp"

namespace kmxdrv {

namespace fs = std::filesystem;
using namespace kmxio;

inline void chk(kmx_ctx* c, int rc, const char* what) { if (rc != KMX_OK) die(std::string(what) + ": " + kmx_last_error(c)); }

// ---- the command line: the value behind option i, as a string or a number.  A number is digits alone: nothing empty, no sign ----
struct Args {
  int argc; char** argv; const char* usage;
  std::string need(int& i) const { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + usage); return argv[++i]; }
  unsigned long num(int& i) const
  {
    const std::string v = need(i);
    try { size_t n = 0; if (v.empty() || v[0] == '-') throw 1; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; }
    catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); }
  }
  uint32_t u32(int& i) const { const unsigned long x = num(i); if (x > 0xFFFFFFFFul) die(std::string(argv[i - 1]) + " does not fit 32 bits"); return (uint32_t)x; }
  double real(int& i) const
  {
    const std::string v = need(i);
    try { size_t n = 0; const double x = std::stod(v, &n); if (n != v.size()) throw 1; return x; }
    catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); }
  }
  double frac(int& i) const { const double x = real(i); if (!(x >= 0.0 && x <= 1.0)) die(std::string(argv[i - 1]) + " must be inside [0, 1]"); return x; }
  // -v [level]: the level kmtricks' own commands take is skipped
  bool verbose(const std::string& a, int& i) const
  {
    if (a != "-v" && a != "--verbose") return false;
    if (i + 1 < argc && argv[i + 1][0] != '-') i++;
    return true;
  }
  [[noreturn]] void unknown(const std::string& a) const { die("unknown option " + a + "\n" + usage); }
};

// `key=value` of the run's options.txt (cmd/all.hpp:85-125: one line of them): where the value lies
inline bool option_at(const std::string& line, const std::string& key, size_t* b, size_t* e)
{
  const size_t at = line.find(" " + key + "="); if (at == std::string::npos) return false;
  *b = at + key.size() + 2; *e = line.find(',', *b);
  if (*e == std::string::npos) *e = line.size();
  while (*e > *b && (line[*e - 1] == '\n' || line[*e - 1] == '\r' || line[*e - 1] == ' ')) --*e;
  return true;
}
inline std::string option_of(const std::string& line, const std::string& key) { size_t b, e; return option_at(line, key, &b, &e) ? line.substr(b, e - b) : ""; }

// what a mode's matrix files look like: extension, header bytes, magic, where the header keeps the column count
struct Kind { const char* mode; const char* ext; size_t hdr; uint64_t magic; size_t cols_at; bool kmer, pa, bf; };
const Kind KINDS[] = {{"kmer:count:bin", "count", 45, MAGIC_MATRIX, 33, true, false, false},
                      {"kmer:pa:bin", "pa", 45, MAGIC_PA, 29, true, true, false},
                      {"hash:count:bin", "count_hash", 37, MAGIC_MATRIX_HASH, 25, false, false, false},
                      {"hash:pa:bin", "pa_hash", 37, MAGIC_PA_HASH, 21, false, true, false},
                      {"hash:bf:bin", "cmbf", 49, MAGIC_BITMATRIX, 21, false, true, true}};      // (rows of Bloom filter bits, no key)
// the first FOUR of them are what most tools read, the first TWO have k-mers for keys
constexpr size_t KMER_KINDS = 2, MATRIX_KINDS = 4, ALL_KINDS = 5;
const char* const MATRIX_MODES = "kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin";

// ---- the run directory as `kmx pipeline` / kmtricks leave it, opened in steps: at, read_mode, shape, open_files; then load ----
struct RunDir {
  std::string tool, run, opt, mode;      // opt: the line of options.txt
  Kind kd{};
  bool reads_bf = false;
  uint32_t k = 0, N = 0, kw = 0;
  uint64_t P = 0, W = 0, stride = 0;     // W: a Bloom run's window
  std::vector<Sample> samples;
  std::vector<std::string> files;

  bool count() const { return !kd.pa; }
  uint32_t rmode() const { return kd.bf ? KMX_MODE_BF : count() ? KMX_MODE_COUNT : KMX_MODE_PA; }

  void at(const std::string& tool_, const std::string& run_)
  {
    tool = tool_; run = run_;
    if (!fs::exists(run + "/kmtricks.fof")) die(run + " is not a kmtricks runtime directory.");
  }
  // the mode options.txt names: one of the first n_kinds of KINDS, or the tool does not read the run (words: how its usage lists them)
  void read_mode(size_t n_kinds, const std::string& words)
  {
    { std::ifstream f(run + "/options.txt"); if (!f) die("Unable to read at " + run + "/options.txt"); std::getline(f, opt); }
    mode = option_of(opt, "count_format") + ":" + option_of(opt, "mode") + ":" + option_of(opt, "format");
    const Kind* found = std::find_if(KINDS, KINDS + n_kinds, [&](const Kind& c) { return mode == c.mode; });
    if (found == KINDS + n_kinds) die("kmx " + tool + " needs a run made with --mode " + words + "; " + run + " was made with " + mode);
    kd = *found;
    reads_bf = n_kinds == ALL_KINDS;
  }
  // k, the partitions, the samples (a tool that has parsed the fof already hands them in), the bytes of a row
  void shape(std::vector<Sample> parsed = {})
  {
    try { k = (uint32_t)std::stoul(option_of(opt, "kmer_size")); } catch (...) { die(run + "/options.txt names no kmer_size"); }
    if (k < 8 || k > 127) die("the run's options.txt names a k-mer size outside [8, 127]");
    if (kd.kmer) {
      uint16_t rp = 0;
      read_repartition(run + "/repartition_gatb/repartition.minimRepart", &rp);
      P = rp;
    } else {
      std::vector<uint8_t> hi = slurp(run + "/hash.info");
      if (hi.size() < 36) die(run + "/hash.info: Invalid file format.");
      P = rd<uint64_t>(&hi[8]); W = rd<uint64_t>(&hi[16]);
    }
    // (a tool that reads Bloom runs checks the window in the same breath, and words the two as one)
    if (P == 0 || P > 65535 || (kd.bf && W == 0))
      die(reads_bf ? "the run's partition count and window do not fit together" : "the run's partition count is outside [1, 65535]");
    samples = parsed.empty() ? parse_fof(run + "/kmtricks.fof", 1) : std::move(parsed);
    N = (uint32_t)samples.size();
    if (N == 0) die(run + "/kmtricks.fof names no sample");
    kw = kd.bf ? 0 : kd.kmer ? (k + 31) / 32 : 1;
    stride = 8ull * kw + (count() ? 4ull * N : (N + 7) / 8);
  }
  [[noreturn]] void truncated(uint64_t p) const { die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]); }
  // every partition's file, plain or .lz4, and what its header says
  void open_files()
  {
    files.resize(P);
    for (uint64_t p = 0; p < P; p++) {
      const std::string plain = run + "/matrices/matrix_" + std::to_string(p) + "." + kd.ext;
      files[p] = !fs::exists(plain) && fs::exists(plain + ".lz4") ? plain + ".lz4" : plain;
      std::ifstream f(files[p], std::ios::binary);
      uint8_t h[49];
      if (!f || !f.read((char*)h, (std::streamsize)kd.hdr)) die("Unable to read at " + plain);
      if (rd<uint64_t>(&h[0]) != MAGIC_BASE || rd<uint64_t>(&h[13]) != kd.magic) die("Invalid file format: " + files[p]);
      if (kd.kmer && (rd<uint32_t>(&h[21]) != k || rd<uint32_t>(&h[25]) != kw))
        die(files[p] + " was made with k = " + std::to_string(rd<uint32_t>(&h[21])) + " in " + std::to_string(rd<uint32_t>(&h[25])) + " words, the run's options.txt says " + std::to_string(k));
      const uint32_t c = rd<uint32_t>(&h[kd.cols_at]);
      if (c != N) die(files[p] + " has rows of " + std::to_string(c) + " columns, the run's kmtricks.fof has " + std::to_string(N) + " samples");
      if (kd.pa && !kd.bf && rd<uint32_t>(&h[kd.cols_at + 4]) != (N + 7) / 8) die("Invalid file format: " + files[p]);
      if (!kd.kmer && !kd.pa && rd<uint32_t>(&h[21]) != 4) die(files[p] + " has counts of " + std::to_string(rd<uint32_t>(&h[21])) + " bytes: kmx " + tool + " reads 4-byte counts");
      if (kd.bf && (rd<uint64_t>(&h[25]) != W * p || rd<uint64_t>(&h[33]) != W)) die(files[p] + ": its window disagrees with the run's hash.info");
      if (!h[12]) {      // (an lz4 body's size is known once it is unpacked: checked when it is read)
        std::error_code ec;
        const uint64_t body = fs::file_size(files[p], ec) - kd.hdr;
        if (ec || body % stride || (kd.bf && body != W * stride)) truncated(p);
      }
    }
  }
  // partition p's rows; a body is shared by the calls that read it and goes with the last of them
  std::shared_ptr<std::vector<uint8_t>> load(uint64_t p) const
  {
    std::vector<uint8_t> raw = slurp(files[p]);
    auto body = std::make_shared<std::vector<uint8_t>>(body_of(raw, kd.hdr, kd.magic, files[p]));
    raw = std::vector<uint8_t>();
    if (body->size() % stride || (kd.bf && body->size() != W * stride)) truncated(p);
    return body;
  }
};

// ---- files that name samples: id -> column of the fof; an id that is not `in`, or comes a second time, is refused at `where` ----
struct SampleIndex {
  std::map<std::string, uint32_t> at;
  std::vector<bool> seen;
  explicit SampleIndex(const std::vector<Sample>& samples) : seen(samples.size(), false) { for (uint32_t i = 0; i < samples.size(); i++) at[samples[i].id] = i; }
  uint32_t take(const std::string& id, const std::string& where, const std::string& in = "the run's kmtricks.fof")
  {
    const auto it = at.find(id);
    if (it == at.end()) die(where + "sample " + id + " is not in " + in);
    if (seen[it->second]) die(where + "sample " + id + " is named twice");
    seen[it->second] = true;
    return it->second;
  }
};

// the --samples list: one id a line, the columns in its order
inline std::vector<uint32_t> read_sample_list(const std::string& path, const std::vector<Sample>& samples)
{
  std::ifstream f(path);
  if (!f) die("Unable to read at " + path);
  SampleIndex index(samples);
  std::vector<uint32_t> cols;
  std::string line;
  for (uint64_t ln = 1; std::getline(f, line); ln++) {
    std::istringstream is(line);
    std::string id, more;
    if (!(is >> id)) continue;      // an empty line
    const std::string where = path + " line " + std::to_string(ln) + ": ";
    if (is >> more) die(where + "expected one sample id");
    cols.push_back(index.take(id, where));
  }
  if (cols.empty()) die(path + " names no sample");
  return cols;
}

// ---- the devices: gpus contexts over the devices there are, and the bytes a shard may fill: --batch-mb, or `tenths` of the least free
// memory, divided among the shards that share a device, and no less than 64 MiB ----
struct Devices {
  std::vector<kmx_ctx*> ctxs;
  uint64_t budget = 0;
  uint32_t G() const { return (uint32_t)ctxs.size(); }
  void close() { for (kmx_ctx* c : ctxs) kmx_destroy(c); }
};
inline Devices open_devices(uint32_t gpus, uint64_t batch_mb, uint32_t tenths)
{
  if (kmx_version() != KMX_VERSION) die("libkmx.so is not the version this driver was built for");
  const uint32_t G = gpus, ndev = (uint32_t)std::max(1, kmx_device_count());
  Devices d;
  d.ctxs.assign(G, nullptr);
  for (uint32_t g = 0; g < G; g++) if (kmx_create((int)(g % ndev), &d.ctxs[g]) != KMX_OK) die(std::string("kmx_create: ") + kmx_last_error(nullptr));
  d.budget = batch_mb << 20;
  if (!d.budget) {
    uint64_t fr = 0, tot = 0;
    for (uint32_t g = 0; g < std::min(G, ndev); g++) { uint64_t f = 0; if (kmx_device_memory((int)g, &f, &tot) == KMX_OK && (g == 0 || f < fr)) fr = f; }
    d.budget = std::max<uint64_t>(fr / 10 * tenths / std::max<uint32_t>(1, (G + ndev - 1) / ndev), 64ull << 20);
  }
  return d;
}
// two runs of rows are on the device at a time (one travels while the other is worked on): how many rows a run holds
inline uint64_t run_rows(uint64_t budget, uint64_t per_row) { return std::min<uint64_t>(std::max<uint64_t>(budget / 2 / per_row, 1), 0xFFFFFF00ull); }

// shard g = 0 ... G - 1, each on a thread of its own (shard 0 on this one); a shard's exception ends the command
template <class Shard> void in_shards(uint32_t G, Shard shard)
{
  auto guarded = [&](uint32_t g) { try { shard(g); } catch (const std::exception& e) { die(e.what()); } };
  std::vector<std::thread> workers;
  for (uint32_t g = 1; g < G; g++) workers.emplace_back(guarded, g);
  guarded(0);
  for (std::thread& w : workers) w.join();
}

// ---- the walk through shard g's partitions (p mod G == g) in runs of rows, two in flight, all adding into the tables of the shard's first
// call.  submit(rows, n_rows, first) fills the task -- the tables of `first`, or none -- and queues it; wait / free are the result type's,
// `what` names the call when a wait fails.  -> the first result, which owns the tables (the caller copies them out and frees it), or null
// for a shard without a partition ----
template <class R, class Submit>
R* accumulate_runs(const RunDir& dir, kmx_ctx* ctx, uint32_t g, uint32_t G, uint64_t run_rows, Submit submit, int (*wait)(R*), void (*free_)(R*), const char* what)
{
  R* first = nullptr;
  struct Flight { R* r; std::shared_ptr<std::vector<uint8_t>> body; };
  std::deque<Flight> flying;
  auto land = [&](size_t keep) {
    while (flying.size() > keep) {
      Flight f = flying.front(); flying.pop_front();
      chk(ctx, wait(f.r), what);
      if (f.r != first) free_(f.r);
    }
  };
  for (uint64_t p = g; p < dir.P; p += G) {
    auto body = dir.load(p);
    const uint64_t rows = body->size() / dir.stride;
    for (uint64_t r0 = 0; r0 < rows || (r0 == 0 && !first); r0 += run_rows) {      // (a shard's first call is made even for no rows: it owns the tables)
      const uint64_t n = std::min(run_rows, rows - r0);
      R* r = submit(n ? body->data() + r0 * dir.stride : nullptr, n, first);
      if (!first) { first = r; chk(ctx, wait(r), what); }      // (its tables are asked for by the next call)
      flying.push_back({r, body});
      land(1);      // the run before this one has been worked on; this one travels
      if (rows == 0) break;
    }
  }
  land(0);
  return first;
}

// ---- ... and where every run has a result of its own: the tool queues a run and puts its Flight -- the result, the body it reads, what
// else landed() needs -- here; the run before it lands meanwhile: landed(flight) waits for it, copies out and frees.  finish() at the end ----
template <class Flight, class Landed> struct TwoInFlight {
  Landed landed;
  std::deque<Flight> flying;
  explicit TwoInFlight(Landed l) : landed(l) {}
  void land(size_t keep) { while (flying.size() > keep) { Flight f = flying.front(); flying.pop_front(); landed(f); } }
  void put(const Flight& f) { flying.push_back(f); land(1); }      // the run before this one has been worked on; this one travels
  void finish() { land(0); }
};

// ---- the recurrence spectrum of the run over M of its samples (cols: which, or null for all N), through kmx_pan_host: spec, 3 (M + 1)
// numbers, and with `shared` the (M + 1) x N table beside it; the devices' tables are summed here ----
inline void pan_pass(const RunDir& dir, const Devices& dev, uint64_t run_rows, const uint32_t* cols, uint32_t M, uint32_t min_abund, std::vector<uint64_t>* spec,
                     std::vector<uint64_t>* shared)
{
  spec->assign(3 * ((uint64_t)M + 1), 0);
  if (shared) shared->assign(((uint64_t)M + 1) * dir.N, 0);
  std::mutex mu;
  in_shards(dev.G(), [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    kmx_pan_result* first = accumulate_runs<kmx_pan_result>(dir, ctx, g, dev.G(), run_rows, [&](const uint8_t* rows, uint64_t n, kmx_pan_result* first) {
      kmx_pan_task t; memset(&t, 0, sizeof t);
      t.key_words = dir.kw; t.mode = dir.rmode(); t.n_cols = dir.N; t.n_use = M;
      t.cols = cols; t.min_abund = min_abund; t.flags = shared ? KMX_PAN_SHARED : 0;
      t.n_rows = n; t.rows = rows;
      t.spectrum = first ? kmx_pan_result_spectrum_dev(first) : nullptr;
      t.shared = first && shared ? kmx_pan_result_shared_dev(first) : nullptr;
      kmx_pan_result* r = nullptr;
      chk(ctx, kmx_pan_host(ctx, &t, &r), "kmx_pan_host");
      return r;
    }, kmx_pan_result_wait, kmx_pan_result_free, "kmx_pan");
    if (!first) return;      // (more shards than partitions)
    std::vector<uint64_t> sp(spec->size()), sh(shared ? shared->size() : 0);
    chk(ctx, kmx_pan_result_copy_spectrum(first, sp.data(), sp.size()), "kmx_pan_result_copy_spectrum");
    if (shared) chk(ctx, kmx_pan_result_copy_shared(first, sh.data(), sh.size()), "kmx_pan_result_copy_shared");
    kmx_pan_result_free(first);
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < sp.size(); i++) (*spec)[i] += sp[i];
    for (size_t i = 0; i < sh.size(); i++) (*shared)[i] += sh[i];
  });
}

// ---- a text, or bytes, to a file; "": standard output ----
inline void write_text(const std::string& path, const void* data, size_t n)
{
  FILE* f = path.empty() ? stdout : fopen(path.c_str(), "w");
  if (!f) die("Unable to write at " + path);
  if (n && fwrite(data, 1, n, f) != n) die("write failed: " + (path.empty() ? std::string("stdout") : path));
  if (f != stdout) { if (fclose(f) != 0) die("write failed: " + path); } else fflush(stdout);
}
inline void write_text(const std::string& path, const std::string& txt) { write_text(path, txt.data(), txt.size()); }

}  // namespace kmxdrv
