// kmx_dist.cpp -- `kmx dist`: how the samples of a run relate to each other -- the sample-by-sample table of shared k-mers and the Jaccard
// and Bray-Curtis distances that follow from it (what Simka computes; no counterpart in the kmtricks tree).  The input is the run
// directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run, the .count_hash / .pa_hash matrices of a
// hash run, or the .cmbf Bloom matrices of a hash:bf:bin run (there the numbers count Bloom bits: an estimate).  Every partition goes
// through kmx_dist_host in runs of rows that fit the device; all of them add into one table per device, the devices' tables are summed
// on the host.  Every check that needs no GPU comes before kmx_create.
#include <kmx.h>
#include <algorithm>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include "kmx_io.hpp"
#include "kmx_run.hpp"

namespace fs = std::filesystem;
using namespace kmxio;

namespace {

struct DOpt {
  std::string run, out, metric = "shared";
  uint32_t gpus = 1;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
  bool verbose = false;
};

const char* USAGE = "usage: kmx dist --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin, hash:pa:bin or hash:bf:bin> "
                    "[--metric shared|jaccard|braycurtis (braycurtis: count runs only)] [--output FILE] [--gpus INT] [--batch-mb INT] [-v]\n"
                    "  shared: the rows (k-mers, hashes) two samples both hold; jaccard: 1 - shared / union; braycurtis: 1 - 2 * sum of the smaller counts / "
                    "sum of both samples' counts.\n  For a hash:bf:bin run the rows are Bloom filter bits: the numbers are an estimate of the k-mers' (false positives count too).";

DOpt parse(int argc, char** argv)
{
  DOpt o;
  auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + USAGE); return argv[++i]; };
  auto num = [&](int& i) -> unsigned long { const std::string v = need(i); try { size_t n = 0; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = need(i);
    else if (a == "--metric") { o.metric = need(i); if (o.metric != "shared" && o.metric != "jaccard" && o.metric != "braycurtis") die("--metric must be shared, jaccard or braycurtis"); }
    else if (a == "--output") o.out = need(i);
    else if (a == "--gpus") o.gpus = num(i);
    else if (a == "--batch-mb") o.batch_mb = num(i);
    else if (a == "-v" || a == "--verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') i++; }
    else die("unknown option " + a + "\n" + USAGE);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
}

void chk(kmx_ctx* c, int rc, const char* what) { if (rc != KMX_OK) die(std::string(what) + ": " + kmx_last_error(c)); }

// `key=value` of the run's options.txt (cmd/all.hpp:85-125: one line of them)
std::string option_of(const std::string& line, const std::string& key)
{
  const size_t at = line.find(" " + key + "="); if (at == std::string::npos) return "";
  const size_t b = at + key.size() + 2, e = line.find(',', b);
  std::string v = line.substr(b, e == std::string::npos ? std::string::npos : e - b);
  while (!v.empty() && (v.back() == '\n' || v.back() == '\r' || v.back() == ' ')) v.pop_back();
  return v;
}

// what a mode's matrix files look like: extension, header bytes, magic, where the header keeps the column count
struct Kind { const char* ext; size_t hdr; uint64_t magic; size_t cols_at; bool kmer, pa, bf; };

}  // namespace

int kmx_dist_main(int argc, char** argv)
{
  const DOpt o = parse(argc, argv);
  const std::string& run = o.run;
  // ---- the run directory; every check before kmx_create ----
  if (!fs::exists(run + "/kmtricks.fof")) die(run + " is not a kmtricks runtime directory.");
  std::string opt; { std::ifstream f(run + "/options.txt"); if (!f) die("Unable to read at " + run + "/options.txt"); std::getline(f, opt); }
  const std::string mode = option_of(opt, "count_format") + ":" + option_of(opt, "mode") + ":" + option_of(opt, "format");
  Kind kd;
  if (mode == "kmer:count:bin") kd = {"count", 45, MAGIC_MATRIX, 33, true, false, false};
  else if (mode == "kmer:pa:bin") kd = {"pa", 45, MAGIC_PA, 29, true, true, false};
  else if (mode == "hash:count:bin") kd = {"count_hash", 37, MAGIC_MATRIX_HASH, 25, false, false, false};
  else if (mode == "hash:pa:bin") kd = {"pa_hash", 37, MAGIC_PA_HASH, 21, false, true, false};
  else if (mode == "hash:bf:bin") kd = {"cmbf", 49, MAGIC_BITMATRIX, 21, false, true, true};
  else die("kmx dist needs a run made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin, hash:pa:bin or hash:bf:bin; " + run + " was made with " + mode);
  const bool count = !kd.pa;
  if (o.metric == "braycurtis" && !count) die("--metric braycurtis needs a count run (kmer:count:bin or hash:count:bin): " + run + " was made with " + mode + " and has no counts");
  uint32_t k = 0;
  try { k = (uint32_t)std::stoul(option_of(opt, "kmer_size")); } catch (...) { die(run + "/options.txt names no kmer_size"); }
  if (k < 8 || k > 127) die("the run's options.txt names a k-mer size outside [8, 127]");
  uint64_t P = 0, W = 0;
  if (kd.kmer) {
    uint16_t rp = 0;
    read_repartition(run + "/repartition_gatb/repartition.minimRepart", &rp);
    P = rp;
  } else {
    std::vector<uint8_t> hi = slurp(run + "/hash.info");
    if (hi.size() < 36) die(run + "/hash.info: Invalid file format.");
    P = rd<uint64_t>(&hi[8]); W = rd<uint64_t>(&hi[16]);
  }
  if (P == 0 || P > 65535 || (kd.bf && W == 0)) die("the run's partition count and window do not fit together");
  const std::vector<Sample> samples = parse_fof(run + "/kmtricks.fof", 1);
  const uint32_t N = (uint32_t)samples.size();
  if (N == 0) die(run + "/kmtricks.fof names no sample");
  if (N > 32768) die("kmx dist takes at most 32768 samples (a table would be 8 GiB)");
  const uint32_t kw = kd.bf ? 0 : kd.kmer ? (k + 31) / 32 : 1;
  const uint64_t stride = 8ull * kw + (count ? 4ull * N : (N + 7) / 8);
  std::vector<std::string> files(P);
  for (uint64_t p = 0; p < P; p++) {
    const std::string plain = run + "/matrices/matrix_" + std::to_string(p) + "." + kd.ext;
    files[p] = !fs::exists(plain) && fs::exists(plain + ".lz4") ? plain + ".lz4" : plain;
    std::ifstream f(files[p], std::ios::binary);
    uint8_t h[49];
    if (!f || !f.read((char*)h, (std::streamsize)kd.hdr)) die("Unable to read at " + plain);
    if (rd<uint64_t>(&h[0]) != MAGIC_BASE || rd<uint64_t>(&h[13]) != kd.magic) die("Invalid file format: " + files[p]);
    if (kd.kmer && (rd<uint32_t>(&h[21]) != k || rd<uint32_t>(&h[25]) != kw))
      die(files[p] + " was made with k = " + std::to_string(rd<uint32_t>(&h[21])) + " in " + std::to_string(rd<uint32_t>(&h[25])) + " words, the run's options.txt says " + std::to_string(k));
    const uint32_t cols = rd<uint32_t>(&h[kd.cols_at]);
    if (cols != N) die(files[p] + " has rows of " + std::to_string(cols) + " columns, the run's kmtricks.fof has " + std::to_string(N) + " samples");
    if (kd.pa && !kd.bf && rd<uint32_t>(&h[kd.cols_at + 4]) != (N + 7) / 8) die("Invalid file format: " + files[p]);
    if (!kd.kmer && !kd.bf && !kd.pa && rd<uint32_t>(&h[21]) != 4) die(files[p] + " has counts of " + std::to_string(rd<uint32_t>(&h[21])) + " bytes: kmx dist reads 4-byte counts");
    if (kd.bf && (rd<uint64_t>(&h[25]) != W * p || rd<uint64_t>(&h[33]) != W)) die(files[p] + ": its window disagrees with the run's hash.info");
    if (!h[12]) {      // (an lz4 body's size is known once it is unpacked: checked when it is read)
      std::error_code ec;
      const uint64_t body = fs::file_size(files[p], ec) - kd.hdr;
      if (ec || body % stride || (kd.bf && body != W * stride)) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
    }
  }
  FILE* out = o.out.empty() ? stdout : fopen(o.out.c_str(), "w");
  if (!out) die("Unable to write at " + o.out);

  // ---- devices; how many rows a run holds ----
  if (kmx_version() != KMX_VERSION) die("libkmx.so is not the version this driver was built for");
  const uint32_t G = o.gpus, ndev = (uint32_t)std::max(1, kmx_device_count());
  std::vector<kmx_ctx*> ctxs(G, nullptr);
  for (uint32_t g = 0; g < G; g++) if (kmx_create((int)(g % ndev), &ctxs[g]) != KMX_OK) die(std::string("kmx_create: ") + kmx_last_error(nullptr));
  uint64_t budget = o.batch_mb << 20;
  if (!budget) {
    uint64_t fr = 0, tot = 0;
    for (uint32_t g = 0; g < std::min(G, ndev); g++) { uint64_t f = 0; if (kmx_device_memory((int)g, &f, &tot) == KMX_OK && (g == 0 || f < fr)) fr = f; }
    budget = std::max<uint64_t>(fr / 10 * 4 / std::max<uint32_t>(1, (G + ndev - 1) / ndev), 64ull << 20);
  }
  // two runs are on the device at a time (one travels while the other is worked on); a row costs its bytes and its presence bits
  const uint64_t per_row = stride + ((uint64_t)N + 63) / 64 * 8;
  const uint64_t run_rows = std::max<uint64_t>(budget / 2 / per_row, 1);
  const bool want_mins = o.metric == "braycurtis";
  if (o.verbose) fprintf(stderr, "[kmx dist] %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", N, (unsigned long long)P, mode.c_str(),
                         (unsigned long long)stride, (unsigned long long)run_rows, G);

  const uint64_t cells = (uint64_t)N * N;
  std::vector<uint64_t> inter(cells, 0), mins(want_mins ? cells : 0, 0);
  std::mutex mu;
  // shard g: the partitions p with p mod G == g, one after the other, all into the table of the shard's first call
  auto shard = [&](uint32_t g) {
    try {
      kmx_ctx* ctx = ctxs[g];
      kmx_dist_result* first = nullptr;
      struct Flight { kmx_dist_result* r; std::shared_ptr<std::vector<uint8_t>> body; };
      std::deque<Flight> flying;
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
          chk(ctx, kmx_dist_result_wait(f.r), "kmx_dist");
          if (f.r != first) kmx_dist_result_free(f.r);
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        std::vector<uint8_t> raw = slurp(files[p]);
        auto body = std::make_shared<std::vector<uint8_t>>(body_of(raw, kd.hdr, kd.magic, files[p]));
        raw = std::vector<uint8_t>();
        if (body->size() % stride || (kd.bf && body->size() != W * stride)) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
        const uint64_t rows = body->size() / stride;
        for (uint64_t r0 = 0; r0 < rows || (r0 == 0 && !first); r0 += run_rows) {      // (a shard's first call is made even for no rows: it owns the tables)
          kmx_dist_task t; memset(&t, 0, sizeof t);
          t.key_words = kw; t.mode = kd.bf ? KMX_MODE_BF : count ? KMX_MODE_COUNT : KMX_MODE_PA; t.n_cols = N; t.want_mins = want_mins ? 1 : 0;
          t.n_rows = std::min(run_rows, rows - r0);
          t.rows = t.n_rows ? body->data() + r0 * stride : nullptr;
          t.inter = first ? kmx_dist_result_inter_dev(first) : nullptr;
          t.mins = first && want_mins ? kmx_dist_result_mins_dev(first) : nullptr;
          kmx_dist_result* r = nullptr;
          chk(ctx, kmx_dist_host(ctx, &t, &r), "kmx_dist_host");
          if (!first) { first = r; chk(ctx, kmx_dist_result_wait(r), "kmx_dist"); }      // (its tables are asked for by the next call)
          flying.push_back({r, body});
          land(1);      // the run before this one has been worked on; this one travels
          if (rows == 0) break;
        }
      }
      land(0);
      if (!first) return;      // (more shards than partitions)
      std::vector<uint64_t> si(cells), sm(want_mins ? cells : 0);
      chk(ctx, kmx_dist_result_copy_inter(first, si.data(), si.size()), "kmx_dist_result_copy_inter");
      if (want_mins) chk(ctx, kmx_dist_result_copy_mins(first, sm.data(), sm.size()), "kmx_dist_result_copy_mins");
      kmx_dist_result_free(first);
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < si.size(); i++) inter[i] += si[i];
      for (size_t i = 0; i < sm.size(); i++) mins[i] += sm[i];
    } catch (const std::exception& e) { die(e.what()); }
  };
  std::vector<std::thread> workers;
  for (uint32_t g = 1; g < G; g++) workers.emplace_back(shard, g);
  shard(0);
  for (std::thread& w : workers) w.join();

  std::string txt;
  for (const Sample& s : samples) { txt += '\t'; txt += s.id; }
  txt += '\n';
  char num[64];
  for (uint32_t i = 0; i < N; i++) {
    txt += samples[i].id;
    for (uint32_t j = 0; j < N; j++) {
      txt += '\t';
      if (o.metric == "shared") { txt += std::to_string(inter[(uint64_t)i * N + j]); continue; }
      double d = 0.0;
      if (o.metric == "jaccard") {
        const uint64_t ij = inter[(uint64_t)i * N + j], den = inter[(uint64_t)i * N + i] + inter[(uint64_t)j * N + j] - ij;
        if (den) d = 1.0 - (double)ij / (double)den;
      } else {
        const uint64_t ij = mins[(uint64_t)i * N + j], den = mins[(uint64_t)i * N + i] + mins[(uint64_t)j * N + j];
        if (den) d = 1.0 - 2.0 * (double)ij / (double)den;
      }
      snprintf(num, sizeof num, "%.6f", d);
      txt += num;
    }
    txt += '\n';
    if (txt.size() > (1u << 20)) { if (fwrite(txt.data(), 1, txt.size(), out) != txt.size()) die("write failed: " + (o.out.empty() ? std::string("stdout") : o.out)); txt.clear(); }
  }
  if (fwrite(txt.data(), 1, txt.size(), out) != txt.size()) die("write failed: " + (o.out.empty() ? std::string("stdout") : o.out));
  if (out != stdout) { if (fclose(out) != 0) die("write failed: " + o.out); } else fflush(stdout);
  for (uint32_t g = 0; g < G; g++) kmx_destroy(ctxs[g]);
  return 0;
}
