// kmx_select.cpp -- `kmx select`: a smaller run out of a larger one (what MUSET's `kmat_tools filter` does on the text of a kmtricks
// matrix; no counterpart in the kmtricks tree).  Some of the samples, in any order; the rows that enough -- and not too many -- of them
// hold, from an abundance upwards; counts kept, zeroed below the abundance, or turned into presence/absence bits (include/kmx.h, section
// "select").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run or the
// .count_hash / .pa_hash matrices of a hash run.  The output is a run directory of its own that every command reads as it reads the
// source.  Every partition goes through kmx_select_host in runs of rows, two in flight, and the kept rows are written as they land.
// Every check that needs no GPU comes before kmx_create, and before anything is written.
#include <kmx.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <thread>
#include "kmx_io.hpp"
#include "kmx_run.hpp"

namespace fs = std::filesystem;
using namespace kmxio;

namespace {

struct SOpt {
  std::string run, out, samples;
  uint32_t gpus = 1, min_abund = 1, min_rec = 0, max_rec = 0xFFFFFFFFu;
  double min_frac = -1.0, max_frac = -1.0;      // below 0: not given
  bool has_min_rec = false, has_max_rec = false;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
  bool pa = false, zero_below = false, cpr = false, verbose = false;
};

const char* USAGE = "usage: kmx select --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> --output DIR "
                    "[--samples FILE] [--min-abund INT] [--min-rec INT | --min-frac FLOAT] [--max-rec INT | --max-frac FLOAT] [--pa] [--zero-below] "
                    "[--cpr] [--gpus INT] [--batch-mb INT] [-v]\n"
                    "  FILE: one sample id per line, the columns of the output in its order (default: every sample of the run).\n"
                    "  Writes DIR as a run directory with the rows that at least --min-rec and at most --max-rec of those samples hold with a count of "
                    "--min-abund or more (fractions are of the number of selected samples); --pa writes presence/absence matrices, --zero-below writes 0 "
                    "for the counts below --min-abund.";

SOpt parse(int argc, char** argv)
{
  SOpt o;
  auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + USAGE); return argv[++i]; };
  auto num = [&](int& i) -> unsigned long { const std::string v = need(i); try { size_t n = 0; if (v.empty() || v[0] == '-') throw 1; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  auto u32 = [&](int& i) -> uint32_t { const unsigned long x = num(i); if (x > 0xFFFFFFFFul) die(std::string(argv[i - 1]) + " does not fit 32 bits"); return (uint32_t)x; };
  auto frac = [&](int& i) -> double {
    const std::string v = need(i); double x = 0;
    try { size_t n = 0; x = std::stod(v, &n); if (n != v.size()) throw 1; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); }
    if (!(x >= 0.0 && x <= 1.0)) die(std::string(argv[i - 1]) + " must be inside [0, 1]");
    return x;
  };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = need(i);
    else if (a == "--output") o.out = need(i);
    else if (a == "--samples") o.samples = need(i);
    else if (a == "--min-abund") { o.min_abund = u32(i); if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--min-rec") { o.min_rec = u32(i); o.has_min_rec = true; }
    else if (a == "--max-rec") { o.max_rec = u32(i); o.has_max_rec = true; }
    else if (a == "--min-frac") o.min_frac = frac(i);
    else if (a == "--max-frac") o.max_frac = frac(i);
    else if (a == "--pa") o.pa = true;
    else if (a == "--zero-below") o.zero_below = true;
    else if (a == "--cpr") o.cpr = true;
    else if (a == "--gpus") o.gpus = u32(i);
    else if (a == "--batch-mb") o.batch_mb = num(i);
    else if (a == "-v" || a == "--verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') i++; }
    else die("unknown option " + a + "\n" + USAGE);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
  if (o.out.empty()) die(std::string("--output is required\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  if (o.has_min_rec && o.min_frac >= 0.0) die("--min-rec and --min-frac name the same bound: give one of them");
  if (o.has_max_rec && o.max_frac >= 0.0) die("--max-rec and --max-frac name the same bound: give one of them");
  if (o.zero_below && o.pa) die("--zero-below needs counts in the output: it cannot go with --pa");
  return o;
}

void chk(kmx_ctx* c, int rc, const char* what) { if (rc != KMX_OK) die(std::string(what) + ": " + kmx_last_error(c)); }

// `key=value` of the run's options.txt (cmd/all.hpp:85-125: one line of them): where the value lies
bool option_at(const std::string& line, const std::string& key, size_t* b, size_t* e)
{
  const size_t at = line.find(" " + key + "="); if (at == std::string::npos) return false;
  *b = at + key.size() + 2; *e = line.find(',', *b);
  if (*e == std::string::npos) { *e = line.size(); while (*e > *b && (line[*e - 1] == '\n' || line[*e - 1] == '\r' || line[*e - 1] == ' ')) --*e; }
  return true;
}
std::string option_of(const std::string& line, const std::string& key) { size_t b, e; return option_at(line, key, &b, &e) ? line.substr(b, e - b) : ""; }

// what a mode's matrix files look like: extension, header bytes, magic, where the header keeps the column count
struct Kind { const char* ext; size_t hdr; uint64_t magic; size_t cols_at; bool kmer, pa; };

}  // namespace

int kmx_select_main(int argc, char** argv)
{
  const SOpt o = parse(argc, argv);
  const std::string& run = o.run;
  // ---- the run directory; every check before kmx_create ----
  if (!fs::exists(run + "/kmtricks.fof")) die(run + " is not a kmtricks runtime directory.");
  std::string opt; { std::ifstream f(run + "/options.txt"); if (!f) die("Unable to read at " + run + "/options.txt"); std::getline(f, opt); }
  const std::string mode = option_of(opt, "count_format") + ":" + option_of(opt, "mode") + ":" + option_of(opt, "format");
  Kind kd;
  if (mode == "kmer:count:bin") kd = {"count", 45, MAGIC_MATRIX, 33, true, false};
  else if (mode == "kmer:pa:bin") kd = {"pa", 45, MAGIC_PA, 29, true, true};
  else if (mode == "hash:count:bin") kd = {"count_hash", 37, MAGIC_MATRIX_HASH, 25, false, false};
  else if (mode == "hash:pa:bin") kd = {"pa_hash", 37, MAGIC_PA_HASH, 21, false, true};
  else die("kmx select needs a run made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin; " + run + " was made with " + mode);
  const bool count = !kd.pa, out_count = count && !o.pa;
  if (!count && o.min_abund > 1) die("--min-abund above 1 needs counts: " + run + " was made with " + mode);
  if (!count && o.zero_below) die("--zero-below needs counts: " + run + " was made with " + mode);
  uint32_t k = 0;
  try { k = (uint32_t)std::stoul(option_of(opt, "kmer_size")); } catch (...) { die(run + "/options.txt names no kmer_size"); }
  if (k < 8 || k > 127) die("the run's options.txt names a k-mer size outside [8, 127]");
  uint64_t P = 0;
  if (kd.kmer) {
    uint16_t rp = 0;
    read_repartition(run + "/repartition_gatb/repartition.minimRepart", &rp);
    P = rp;
  } else {
    std::vector<uint8_t> hi = slurp(run + "/hash.info");
    if (hi.size() < 36) die(run + "/hash.info: Invalid file format.");
    P = rd<uint64_t>(&hi[8]);
  }
  if (P == 0 || P > 65535) die("the run's partition count is outside [1, 65535]");
  const std::vector<Sample> samples = parse_fof(run + "/kmtricks.fof", 1);
  const uint32_t N = (uint32_t)samples.size();
  if (N == 0) die(run + "/kmtricks.fof names no sample");
  // the fof's lines as they stand, one a sample (parse_fof skips what is empty in the same way)
  std::vector<std::string> fof_lines;
  {
    std::ifstream f(run + "/kmtricks.fof"); std::string line;
    while (std::getline(f, line)) { while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back(); if (!line.empty()) fof_lines.push_back(line); }
    if (fof_lines.size() != N) die("fof: " + run + "/kmtricks.fof changed while it was read");
  }
  // the sample list: one id a line, the output's columns in its order
  std::vector<uint32_t> cols;
  if (!o.samples.empty()) {
    std::ifstream f(o.samples);
    if (!f) die("Unable to read at " + o.samples);
    std::map<std::string, uint32_t> at;
    for (uint32_t i = 0; i < N; i++) at[samples[i].id] = i;
    std::vector<bool> seen(N, false);
    std::string line;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
      std::istringstream is(line);
      std::string id, more;
      if (!(is >> id)) continue;      // an empty line
      const std::string where = o.samples + " line " + std::to_string(ln) + ": ";
      if (is >> more) die(where + "expected one sample id");
      const auto it = at.find(id);
      if (it == at.end()) die(where + "sample " + id + " is not in the run's kmtricks.fof");
      if (seen[it->second]) die(where + "sample " + id + " is named twice");
      seen[it->second] = true;
      cols.push_back(it->second);
    }
    if (cols.empty()) die(o.samples + " names no sample");
  }
  const uint32_t M = o.samples.empty() ? N : (uint32_t)cols.size();
  uint32_t min_rec = o.min_rec, max_rec = o.max_rec;
  if (o.min_frac >= 0.0) min_rec = (uint32_t)std::ceil(o.min_frac * (double)M);
  if (o.max_frac >= 0.0) max_rec = (uint32_t)std::floor(o.max_frac * (double)M);
  const uint32_t kw = kd.kmer ? (k + 31) / 32 : 1;
  const uint64_t stride = 8ull * kw + (count ? 4ull * N : (N + 7) / 8);
  const uint64_t ostride = 8ull * kw + (out_count ? 4ull * M : (M + 7) / 8);
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
    const uint32_t c = rd<uint32_t>(&h[kd.cols_at]);
    if (c != N) die(files[p] + " has rows of " + std::to_string(c) + " columns, the run's kmtricks.fof has " + std::to_string(N) + " samples");
    if (kd.pa && rd<uint32_t>(&h[kd.cols_at + 4]) != (N + 7) / 8) die("Invalid file format: " + files[p]);
    if (!kd.kmer && !kd.pa && rd<uint32_t>(&h[21]) != 4) die(files[p] + " has counts of " + std::to_string(rd<uint32_t>(&h[21])) + " bytes: kmx select reads 4-byte counts");
    if (!h[12]) {      // (an lz4 body's size is known once it is unpacked: checked when it is read)
      std::error_code ec;
      const uint64_t body = fs::file_size(files[p], ec) - kd.hdr;
      if (ec || body % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
    }
  }
  // the place of the output: a directory that is not there yet, or an empty one
  const std::string root = fs::absolute(o.out).string();
  {
    std::error_code ec;
    if (fs::exists(root, ec) && (!fs::is_directory(root, ec) || !fs::is_empty(root, ec))) die(o.out + " exists and is not an empty directory");
  }

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
  // two runs are on the device at a time; a row costs its bytes (the upload), the room for it at its new size, its keep word, its
  // recurrence and its record
  const uint64_t per_row = stride + ostride + 8 + sizeof(kmx_select_rec);
  const uint64_t run_rows = std::min<uint64_t>(std::max<uint64_t>(budget / 2 / per_row, 1), 0xFFFFFF00ull);
  const uint32_t rmode = count ? KMX_MODE_COUNT : KMX_MODE_PA, omode = out_count ? KMX_MODE_COUNT : KMX_MODE_PA;
  const std::string oext = kd.kmer ? (out_count ? "count" : "pa") : (out_count ? "count_hash" : "pa_hash");
  if (o.verbose) fprintf(stderr, "[kmx select] %u of %u samples, %llu partitions (%s), rows of %llu -> %llu bytes, recurrence in [%u, %u], runs of %llu rows, %u shards\n", M, N,
                         (unsigned long long)P, mode.c_str(), (unsigned long long)stride, (unsigned long long)ostride, min_rec, max_rec >= M ? M : max_rec,
                         (unsigned long long)run_rows, G);

  // ---- the run directory of the output ----
  fs::create_directories(root + "/matrices");
  {
    std::ofstream f(root + "/kmtricks.fof");
    for (uint32_t j = 0; j < M; j++) f << fof_lines[o.samples.empty() ? j : cols[j]] << "\n";
    if (!f) die("Unable to write at " + root + "/kmtricks.fof");
  }
  {
    std::string line = opt;
    size_t b, e;
    if (o.pa && option_at(line, "mode", &b, &e)) line.replace(b, e - b, "pa");
    std::ofstream f(root + "/options.txt");
    f << line << "\n";
    if (!f) die("Unable to write at " + root + "/options.txt");
  }
  for (const char* rel : {"repartition_gatb/repartition.minimRepart", "hash.info", "config_gatb/gatb.config"}) {
    const fs::path src = fs::path(run) / rel, dst = fs::path(root) / rel;
    if (!fs::exists(src)) continue;
    fs::create_directories(dst.parent_path());
    fs::copy_file(src, dst);
  }

  auto load = [&](uint64_t p) {
    std::vector<uint8_t> raw = slurp(files[p]);
    auto body = std::make_shared<std::vector<uint8_t>>(body_of(raw, kd.hdr, kd.magic, files[p]));
    if (body->size() % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
    return body;
  };
  std::vector<uint64_t> rows_in(P, 0), rows_kept(P, 0);
  auto shard = [&](uint32_t g) {
    try {
      kmx_ctx* ctx = ctxs[g];
      struct Flight { kmx_select_result* r; std::shared_ptr<std::vector<uint8_t>> body; std::shared_ptr<Out> file; uint64_t p; bool last; };
      std::deque<Flight> flying;
      std::vector<uint8_t> kept;
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
          if (f.r) {
            chk(ctx, kmx_select_result_wait(f.r), "kmx_select");
            const uint64_t n = kmx_select_result_rows(f.r);
            kept.resize(n * ostride);
            chk(ctx, kmx_select_result_copy_body(f.r, kept.data(), kept.size()), "kmx_select_result_copy_body");
            kmx_select_result_free(f.r);
            f.file->raw(kept.data(), kept.size());
            rows_kept[f.p] += n;
          }
          if (f.last) f.file->close();
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        auto body = load(p);
        const uint64_t rows = body->size() / stride;
        rows_in[p] = rows;
        auto file = std::make_shared<Out>(root + "/matrices/matrix_" + std::to_string(p) + "." + oext + (o.cpr ? ".lz4" : ""));
        if (kd.kmer) { if (out_count) matrix_count_header(*file, k, M, (uint32_t)p, o.cpr); else matrix_pa_header(*file, k, M, (uint32_t)p, o.cpr); }
        else { if (out_count) matrix_count_hash_header(*file, M, (uint32_t)p, o.cpr); else matrix_pa_hash_header(*file, M, (uint32_t)p, o.cpr); }
        if (rows == 0) { flying.push_back({nullptr, body, file, p, true}); land(1); continue; }
        for (uint64_t r0 = 0; r0 < rows; r0 += run_rows) {
          kmx_select_task t; memset(&t, 0, sizeof t);
          t.key_words = kw; t.mode = rmode; t.n_cols = N; t.n_out = M;
          t.n_rows = std::min(run_rows, rows - r0);
          t.rows = body->data() + r0 * stride;
          t.cols = o.samples.empty() ? nullptr : cols.data();
          t.min_abund = o.min_abund; t.min_rec = min_rec; t.max_rec = max_rec; t.out_mode = omode;
          t.flags = o.zero_below ? KMX_SELECT_ZERO_BELOW : 0;
          kmx_select_result* r = nullptr;
          chk(ctx, kmx_select_host(ctx, &t, &r), "kmx_select_host");
          flying.push_back({r, body, file, p, r0 + run_rows >= rows});
          land(1);      // the run before this one has been worked on; this one travels
        }
      }
      land(0);
    } catch (const std::exception& e) { die(e.what()); }
  };
  {
    std::vector<std::thread> workers;
    for (uint32_t g = 1; g < G; g++) workers.emplace_back(shard, g);
    shard(0);
    for (std::thread& w : workers) w.join();
  }
  if (o.verbose) {
    uint64_t in = 0, out = 0;
    for (uint64_t p = 0; p < P; p++) {
      fprintf(stderr, "[kmx select] partition %llu: %llu rows in, %llu kept\n", (unsigned long long)p, (unsigned long long)rows_in[p], (unsigned long long)rows_kept[p]);
      in += rows_in[p]; out += rows_kept[p];
    }
    fprintf(stderr, "[kmx select] total: %llu rows in, %llu kept\n", (unsigned long long)in, (unsigned long long)out);
  }
  for (uint32_t g = 0; g < G; g++) kmx_destroy(ctxs[g]);
  return 0;
}
