// kmx_assoc.cpp -- `kmx assoc`: the structure-corrected association test of a run's rows (what kmdiff, EIGENSTRAT and a k-mer GWAS run once
// the samples' principal components are known; no counterpart in the kmtricks tree; include/kmx.h, section "assoc").  A phenotype --
// case/control or quantitative -- is regressed on each row's presence pattern with the covariates (the PCs `kmx pca` writes, or any
// others) in the model.  The design is made on the host (kmx_assoc_math.hpp): the covariates' orthonormal basis and the phenotype's
// residual, in fixed point.  Pass 1 sends every partition through kmx_pan_host for the rows by recurrence: the number of tests is the
// number of rows inside the recurrence window; the threshold follows from --alpha.  Pass 2 sends every partition through kmx_assoc_host
// in runs of rows, two in flight, and prints the kept rows.  `kmx assoc --design FILE --fof FOF ...` writes the design and asks for no
// device.  Every check that needs no GPU comes before kmx_create.
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
#include "kmx_assoc_math.hpp"

namespace fs = std::filesystem;
using namespace kmxio;

namespace {

struct SOpt {
  std::string run, fof, pheno, groups, covar, out, design, correction = "bonferroni";
  double alpha = 0.05;
  uint32_t gpus = 1, min_abund = 1, min_rec = 1, max_rec = 0xFFFFFFFFu, pcs = 0;
  bool has_pcs = false, has_max = false, counts = false, verbose = false;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
};

const char* USAGE = "usage: kmx assoc --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> (--pheno FILE | --groups FILE) "
                    "[--covar FILE] [--pcs INT] [--min-abund INT] [--min-rec INT] [--max-rec INT] [--alpha 0.05] [--correction bonferroni|none] [--counts] "
                    "[--output FILE] [--design FILE] [--gpus INT] [--batch-mb INT] [-v]\n"
                    "       kmx assoc --design FILE --fof FOF (--pheno FILE | --groups FILE) [--covar FILE] [--pcs INT]\n"
                    "  FILE of --pheno: one `sample_id number` per line; of --groups: one `sample_id case|control` per line (case 1, control 0).  The samples "
                    "it names are the ones tested, in the order of the run's kmtricks.fof.\n"
                    "  FILE of --covar: what `kmx pca --output` writes, a header line and then `sample_id v1 ... vk` per line; --pcs uses the first INT columns.\n"
                    "  Prints the rows whose presence pattern (a sample holds a row from a count of --min-abund) is associated with the phenotype once the "
                    "covariates are projected out of both: key, p, the statistic (one degree of freedom), the regression coefficient and the number of tested "
                    "samples that hold the row.  Rows held by fewer than --min-rec (at least 1) or more than --max-rec (default: all but one) tested samples "
                    "are not tested; under --correction bonferroni alpha is divided by the number of rows INSIDE that window (kmx diff divides by all rows), "
                    "which the recurrence spectrum of the first pass gives.  --design writes the fixed-point design the device is given.";

SOpt parse(int argc, char** argv)
{
  SOpt o;
  auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + USAGE); return argv[++i]; };
  auto num = [&](int& i) -> unsigned long { const std::string v = need(i); try { size_t n = 0; if (v.empty() || v[0] == '-') throw 1; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  auto u32 = [&](int& i) -> uint32_t { const unsigned long x = num(i); if (x > 0xFFFFFFFFul) die(std::string(argv[i - 1]) + " does not fit 32 bits"); return (uint32_t)x; };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = need(i);
    else if (a == "--fof") o.fof = need(i);
    else if (a == "--pheno") o.pheno = need(i);
    else if (a == "--groups") o.groups = need(i);
    else if (a == "--covar") o.covar = need(i);
    else if (a == "--design") o.design = need(i);
    else if (a == "--output") o.out = need(i);
    else if (a == "--pcs") { o.pcs = u32(i); o.has_pcs = true; }
    else if (a == "--min-abund") { o.min_abund = u32(i); if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--min-rec") o.min_rec = std::max<uint32_t>(1, u32(i));
    else if (a == "--max-rec") { o.max_rec = u32(i); o.has_max = true; }
    else if (a == "--alpha") {
      const std::string v = need(i);
      try { size_t n = 0; o.alpha = std::stod(v, &n); if (n != v.size()) throw 1; } catch (...) { die("bad number for --alpha: " + v); }
      if (!(o.alpha > 0.0 && o.alpha < 1.0)) die("--alpha must be inside (0, 1)");
    }
    else if (a == "--correction") { o.correction = need(i); if (o.correction != "bonferroni" && o.correction != "none") die("--correction must be bonferroni or none"); }
    else if (a == "--counts") o.counts = true;
    else if (a == "--gpus") o.gpus = u32(i);
    else if (a == "--batch-mb") o.batch_mb = num(i);
    else if (a == "-v" || a == "--verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') i++; }
    else die("unknown option " + a + "\n" + USAGE);
  }
  if (o.run.empty() && (o.design.empty() || o.fof.empty())) die(std::string("--run, or --design with --fof, is required\n") + USAGE);
  if (!o.run.empty() && !o.fof.empty()) die(std::string("--fof goes with --design alone: a run has its own kmtricks.fof\n") + USAGE);
  if (o.pheno.empty() == o.groups.empty()) die(std::string("one of --pheno and --groups is required\n") + USAGE);
  if (o.has_pcs && o.covar.empty()) die("--pcs needs --covar");
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
struct Kind { const char* ext; size_t hdr; uint64_t magic; size_t cols_at; bool kmer, pa; };

double p_of(double stat) { return std::erfc(std::sqrt(stat / 2.0)); }

// the smallest double t in [0, 2000] with erfc(sqrt(t / 2)) <= p (kmx diff's bisection)
double threshold_of(double p)
{
  double lo = 0.0, hi = 2000.0;
  if (!(p_of(hi) <= p)) die("the corrected p-value threshold is below what a statistic of 2000 reaches: raise --alpha or use --correction none");
  if (p_of(lo) <= p) return lo;
  for (int i = 0; i < 200; i++) {
    const double mid = 0.5 * (lo + hi);
    if (p_of(mid) <= p) hi = mid; else lo = mid;
  }
  return hi;
}

std::string kmer_string(const uint8_t* key, uint32_t k)
{
  std::string s(k, 'A');
  for (uint32_t i = 0; i < k; i++) { const uint32_t d = k - 1 - i; uint64_t w; memcpy(&w, key + 8 * (d >> 5), 8); s[i] = "ACTG"[(w >> ((d & 31) * 2)) & 3]; }
  return s;
}

bool number_of(const std::string& s, double* v)
{
  char* end = nullptr;
  *v = strtod(s.c_str(), &end);
  return !s.empty() && !*end && std::isfinite(*v);
}

}  // namespace

int kmx_assoc_main(int argc, char** argv)
{
  const SOpt o = parse(argc, argv);
  const std::string& run = o.run;
  const std::string fof = run.empty() ? o.fof : run + "/kmtricks.fof";
  if (!run.empty() && !fs::exists(fof)) die(run + " is not a kmtricks runtime directory.");
  // ---- the samples, the phenotype, the covariates, the design: no device ----
  const std::vector<Sample> samples = parse_fof(fof, 1);
  const uint32_t N = (uint32_t)samples.size();
  if (N == 0) die(fof + " names no sample");
  std::map<std::string, uint32_t> at;
  for (uint32_t i = 0; i < N; i++) at[samples[i].id] = i;
  std::vector<bool> seen(N, false);
  std::vector<double> y_of(N, 0.0);
  {
    const std::string& path = o.pheno.empty() ? o.groups : o.pheno;
    std::ifstream f(path);
    if (!f) die("Unable to read at " + path);
    std::string line;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
      std::istringstream is(line);
      std::string id, val, more;
      if (!(is >> id)) continue;      // an empty line
      const std::string where = path + " line " + std::to_string(ln) + ": ";
      if (!(is >> val) || (is >> more)) die(where + (o.pheno.empty() ? "expected `sample_id case|control`" : "expected `sample_id number`"));
      const auto it = at.find(id);
      if (it == at.end()) die(where + "sample " + id + " is not in " + fof);
      if (seen[it->second]) die(where + "sample " + id + " is named twice");
      double v = 0;
      if (o.pheno.empty()) {
        if (val != "case" && val != "control") die(where + "the label of " + id + " is " + val + ", neither case nor control");
        v = val == "case" ? 1.0 : 0.0;
      } else if (!number_of(val, &v)) die(where + "the phenotype of " + id + " is " + val + ", not a finite number");
      seen[it->second] = true;
      y_of[it->second] = v;
    }
  }
  std::vector<uint32_t> cols;      // the listed samples, in fof order
  for (uint32_t i = 0; i < N; i++) if (seen[i]) cols.push_back(i);
  const uint32_t M = (uint32_t)cols.size();
  if (M == 0) die((o.pheno.empty() ? o.groups : o.pheno) + " names no sample");
  uint32_t K = 0;
  std::vector<double> cov;
  if (!o.covar.empty()) {
    std::ifstream f(o.covar);
    if (!f) die("Unable to read at " + o.covar);
    std::string line;
    if (!std::getline(f, line)) die(o.covar + ": no header line");
    { std::istringstream is(line); std::string w; uint32_t n = 0; while (is >> w) n++; if (n < 2) die(o.covar + ": the header names no covariate column"); K = n - 1; }
    const uint32_t width = K;
    if (o.has_pcs) { if (o.pcs > width) die("--pcs " + std::to_string(o.pcs) + ": " + o.covar + " has " + std::to_string(width) + " columns"); K = o.pcs; }
    if (K > 31) die("more than 31 covariate columns (" + std::to_string(K) + "): use --pcs");
    std::vector<int64_t> row_of(N, -1);
    std::vector<double> all;
    uint64_t n_lines = 0;
    for (uint64_t ln = 2; std::getline(f, line); ln++) {
      std::istringstream is(line);
      std::string id, w;
      if (!(is >> id)) continue;
      const std::string where = o.covar + " line " + std::to_string(ln) + ": ";
      const auto it = at.find(id);
      if (it == at.end()) die(where + "sample " + id + " is not in " + fof);
      if (row_of[it->second] >= 0) die(where + "sample " + id + " is named twice");
      uint32_t n = 0;
      while (is >> w) {
        double v = 0;
        if (!number_of(w, &v)) die(where + "the value " + w + " of " + id + " is not a finite number");
        if (n < K) all.push_back(v);
        n++;
      }
      if (n != width) die(where + std::to_string(n) + " values, the header has " + std::to_string(width) + " columns");
      row_of[it->second] = (int64_t)n_lines++;
    }
    cov.resize((size_t)M * K);
    for (uint32_t m = 0; m < M; m++) {
      if (row_of[cols[m]] < 0) die("sample " + samples[cols[m]].id + " has a phenotype but is missing from " + o.covar);
      for (uint32_t j = 0; j < K; j++) cov[(size_t)m * K + j] = all[(size_t)row_of[cols[m]] * K + j];
    }
  }
  std::vector<double> y(M);
  for (uint32_t m = 0; m < M; m++) y[m] = y_of[cols[m]];
  const kmxassoc::Design D = kmxassoc::make_design(M, K, y, cov);
  if (!D.ok) die(D.err);
  const uint32_t q = D.q, V = q + 1;
  if (o.verbose) fprintf(stderr, "[kmx assoc] %u of %u samples, %u model columns, F = %u, gain %.17g, ymax %.17g, vmin %.17g (quantisation bound %.17g)\n", M, N, q,
                         kmxassoc::FRAC_BITS, D.gain, D.ymax, D.vmin, kmxassoc::v_bound(M, q));
  if (!o.design.empty()) {
    char num[64];
    std::string t = "# kmx assoc design\nF\t" + std::to_string(kmxassoc::FRAC_BITS) + "\nM\t" + std::to_string(M) + "\nq\t" + std::to_string(q) + "\n";
    snprintf(num, sizeof num, "gain\t%.17g\n", D.gain); t += num;
    snprintf(num, sizeof num, "vmin\t%.17g\n", D.vmin); t += num;
    snprintf(num, sizeof num, "ymax\t%.17g\n", D.ymax); t += num;
    t += "sample\tcolumn";
    for (uint32_t j = 0; j < V; j++) t += "\tv" + std::to_string(j);
    t += '\n';
    for (uint32_t m = 0; m < M; m++) {
      t += samples[cols[m]].id + '\t' + std::to_string(cols[m]);
      for (uint32_t j = 0; j < V; j++) t += '\t' + std::to_string(D.vecs[(size_t)m * V + j]);
      t += '\n';
    }
    FILE* f = fopen(o.design.c_str(), "w");
    if (!f) die("Unable to write at " + o.design);
    if (fwrite(t.data(), 1, t.size(), f) != t.size() || fclose(f) != 0) die("write failed: " + o.design);
  }
  if (run.empty()) return 0;

  // ---- the run directory; every check before kmx_create ----
  std::string opt; { std::ifstream f(run + "/options.txt"); if (!f) die("Unable to read at " + run + "/options.txt"); std::getline(f, opt); }
  const std::string mode = option_of(opt, "count_format") + ":" + option_of(opt, "mode") + ":" + option_of(opt, "format");
  Kind kd;
  if (mode == "kmer:count:bin") kd = {"count", 45, MAGIC_MATRIX, 33, true, false};
  else if (mode == "kmer:pa:bin") kd = {"pa", 45, MAGIC_PA, 29, true, true};
  else if (mode == "hash:count:bin") kd = {"count_hash", 37, MAGIC_MATRIX_HASH, 25, false, false};
  else if (mode == "hash:pa:bin") kd = {"pa_hash", 37, MAGIC_PA_HASH, 21, false, true};
  else die("kmx assoc needs a run made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin; " + run + " was made with " + mode);
  const bool count = !kd.pa;
  if (!count && o.min_abund > 1) die("--min-abund above 1 needs counts: " + run + " was made with " + mode);
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
  const uint32_t lo = std::max<uint32_t>(1, o.min_rec), hi = o.has_max ? std::min(o.max_rec, M) : M - 1;
  if (lo > hi) die("--min-rec " + std::to_string(o.min_rec) + " and --max-rec " + std::to_string(hi) + " leave no recurrence class of " + std::to_string(M) + " samples");
  const uint32_t kw = kd.kmer ? (k + 31) / 32 : 1;
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
    const uint32_t c = rd<uint32_t>(&h[kd.cols_at]);
    if (c != N) die(files[p] + " has rows of " + std::to_string(c) + " columns, the run's kmtricks.fof has " + std::to_string(N) + " samples");
    if (kd.pa && rd<uint32_t>(&h[kd.cols_at + 4]) != (N + 7) / 8) die("Invalid file format: " + files[p]);
    if (!kd.kmer && !kd.pa && rd<uint32_t>(&h[21]) != 4) die(files[p] + " has counts of " + std::to_string(rd<uint32_t>(&h[21])) + " bytes: kmx assoc reads 4-byte counts");
    if (!h[12]) {      // (an lz4 body's size is known once it is unpacked: checked when it is read)
      std::error_code ec;
      const uint64_t body = fs::file_size(files[p], ec) - kd.hdr;
      if (ec || body % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
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
  // two runs are on the device at a time; a row costs its bytes twice (the upload, the room for the kept rows), its keep word and two
  // records (the scratch slot, the room for the kept records)
  const uint64_t per_row = 2 * stride + 4 + 2 * sizeof(kmx_assoc_rec);
  const uint64_t run_rows = std::min<uint64_t>(std::max<uint64_t>(budget / 2 / per_row, 1), 0xFFFFFF00ull);
  const uint32_t rmode = count ? KMX_MODE_COUNT : KMX_MODE_PA;
  const bool all_listed = M == N;
  if (o.verbose) fprintf(stderr, "[kmx assoc] %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", (unsigned long long)P, mode.c_str(),
                         (unsigned long long)stride, (unsigned long long)run_rows, G);

  auto load = [&](uint64_t p) {
    std::vector<uint8_t> raw = slurp(files[p]);
    auto body = std::make_shared<std::vector<uint8_t>>(body_of(raw, kd.hdr, kd.magic, files[p]));
    if (body->size() % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
    return body;
  };
  auto in_shards = [&](const std::function<void(uint32_t)>& shard) {
    std::vector<std::thread> workers;
    for (uint32_t g = 1; g < G; g++) workers.emplace_back(shard, g);
    shard(0);
    for (std::thread& w : workers) w.join();
  };

  // ---- pass 1: the rows by recurrence over the listed samples ----
  const uint64_t M1 = (uint64_t)M + 1;
  std::vector<uint64_t> spec(3 * M1, 0);
  std::mutex mu;
  in_shards([&](uint32_t g) {
    try {
      kmx_ctx* ctx = ctxs[g];
      kmx_pan_result* first = nullptr;
      struct Flight { kmx_pan_result* r; std::shared_ptr<std::vector<uint8_t>> body; };
      std::deque<Flight> flying;
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
          chk(ctx, kmx_pan_result_wait(f.r), "kmx_pan");
          if (f.r != first) kmx_pan_result_free(f.r);
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        auto body = load(p);
        const uint64_t rows = body->size() / stride;
        for (uint64_t r0 = 0; r0 < rows || (r0 == 0 && !first); r0 += run_rows) {      // (a shard's first call is made even for no rows: it owns the table)
          kmx_pan_task t; memset(&t, 0, sizeof t);
          t.key_words = kw; t.mode = rmode; t.n_cols = N; t.n_use = M;
          t.cols = all_listed ? nullptr : cols.data(); t.min_abund = o.min_abund;
          t.n_rows = std::min(run_rows, rows - r0);
          t.rows = t.n_rows ? body->data() + r0 * stride : nullptr;
          t.spectrum = first ? kmx_pan_result_spectrum_dev(first) : nullptr;
          kmx_pan_result* r = nullptr;
          chk(ctx, kmx_pan_host(ctx, &t, &r), "kmx_pan_host");
          if (!first) { first = r; chk(ctx, kmx_pan_result_wait(r), "kmx_pan"); }      // (its table is asked for by the next call)
          flying.push_back({r, body});
          land(1);      // the run before this one has been worked on; this one travels
          if (rows == 0) break;
        }
      }
      land(0);
      if (!first) return;      // (more shards than partitions)
      std::vector<uint64_t> sp(spec.size());
      chk(ctx, kmx_pan_result_copy_spectrum(first, sp.data(), sp.size()), "kmx_pan_result_copy_spectrum");
      kmx_pan_result_free(first);
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < sp.size(); i++) spec[i] += sp[i];
    } catch (const std::exception& e) { die(e.what()); }
  });
  uint64_t n_tests = 0, n_all = 0;
  for (uint64_t r = 0; r <= M; r++) { n_all += spec[r]; if (r >= lo && r <= hi) n_tests += spec[r]; }
  const double p_cut = o.correction == "bonferroni" && n_tests ? o.alpha / (double)n_tests : o.alpha;
  const double thr = threshold_of(p_cut);
  if (o.verbose) fprintf(stderr, "[kmx assoc] %llu of %llu rows tested (recurrence %u ... %u), p <= %.6e, statistic >= %.17g\n", (unsigned long long)n_tests,
                         (unsigned long long)n_all, lo, hi, p_cut, thr);

  // ---- pass 2: the test; a partition's text is kept until every partition before it is out ----
  std::vector<std::string> text(P);
  in_shards([&](uint32_t g) {
    try {
      kmx_ctx* ctx = ctxs[g];
      struct Flight { kmx_assoc_result* r; std::shared_ptr<std::vector<uint8_t>> body; uint64_t p; };
      std::deque<Flight> flying;
      std::vector<uint8_t> kept;
      std::vector<kmx_assoc_rec> recs;
      char num[128];
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
          chk(ctx, kmx_assoc_result_wait(f.r), "kmx_assoc");
          const uint64_t n = kmx_assoc_result_rows(f.r);
          kept.resize(n * stride); recs.resize(n);
          chk(ctx, kmx_assoc_result_copy_body(f.r, kept.data(), kept.size()), "kmx_assoc_result_copy_body");
          chk(ctx, kmx_assoc_result_copy_recs(f.r, recs.data(), recs.size()), "kmx_assoc_result_copy_recs");
          kmx_assoc_result_free(f.r);
          std::string& txt = text[f.p];
          for (uint64_t i = 0; i < n; i++) {
            const uint8_t* row = kept.data() + i * stride;
            const kmx_assoc_rec& c = recs[i];
            txt += kd.kmer ? kmer_string(row, k) : std::to_string(rd<uint64_t>(row));
            snprintf(num, sizeof num, "\t%.6e\t%.6f\t%.6g\t%u", p_of(c.stat), c.stat, c.beta * D.ymax, c.rec);
            txt += num;
            if (o.counts) for (uint32_t s = 0; s < N; s++) {
              txt += '\t';
              txt += count ? std::to_string(rd<uint32_t>(row + 8 * kw + 4ull * s)) : std::to_string((row[8 * kw + (s >> 3)] >> (s & 7)) & 1);
            }
            txt += '\n';
          }
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        auto body = load(p);
        const uint64_t rows = body->size() / stride;
        for (uint64_t r0 = 0; r0 < rows; r0 += run_rows) {
          kmx_assoc_task t; memset(&t, 0, sizeof t);
          t.key_words = kw; t.mode = rmode; t.n_cols = N; t.n_use = M;
          t.cols = all_listed ? nullptr : cols.data(); t.min_abund = o.min_abund;
          t.n_rows = std::min(run_rows, rows - r0);
          t.rows = body->data() + r0 * stride;
          t.vecs = D.vecs.data(); t.n_vec = V; t.frac_bits = kmxassoc::FRAC_BITS;
          t.gain = D.gain; t.vmin = D.vmin; t.threshold = thr; t.min_rec = lo; t.max_rec = hi;
          kmx_assoc_result* r = nullptr;
          chk(ctx, kmx_assoc_host(ctx, &t, &r), "kmx_assoc_host");
          flying.push_back({r, body, p});
          land(1);      // the run before this one has been worked on; this one travels
        }
      }
      land(0);
    } catch (const std::exception& e) { die(e.what()); }
  });

  std::string head = std::string(kd.kmer ? "kmer" : "hash") + "\tpvalue\tstat\tbeta\trec";
  if (o.counts) for (const Sample& s : samples) { head += '\t'; head += s.id; }
  head += '\n';
  const std::string where = o.out.empty() ? std::string("stdout") : o.out;
  if (fwrite(head.data(), 1, head.size(), out) != head.size()) die("write failed: " + where);
  for (uint64_t p = 0; p < P; p++) if (fwrite(text[p].data(), 1, text[p].size(), out) != text[p].size()) die("write failed: " + where);
  if (out != stdout) { if (fclose(out) != 0) die("write failed: " + o.out); } else fflush(stdout);
  for (uint32_t g = 0; g < G; g++) kmx_destroy(ctxs[g]);
  return 0;
}
