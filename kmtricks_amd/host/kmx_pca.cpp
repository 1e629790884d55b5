// kmx_pca.cpp -- `kmx pca`: the principal components of a run's samples (what EIGENSTRAT / smartpca compute from genotypes, here from
// the k-mer x sample matrix: every row centred at its own frequency p and weighted by 1 / (p (1 - p)); no counterpart in the kmtricks
// tree; include/kmx.h, section "gram").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices
// of a kmer run or the .count_hash / .pa_hash matrices of a hash run.  Pass 1 sends every partition through kmx_pan_host (the rows by
// recurrence, and per sample); the class weights in fixed point follow from it (kmx_pca_math.hpp); pass 2 sends every partition through
// kmx_gram_host in runs of rows, two in flight, all into one table per device; the devices' tables are summed on the host, where the
// Gram matrix is centred and diagonalised.  `kmx pca --from-gram FILE` diagonalises a matrix saved with --gram and asks for no device.
// Every check that needs no GPU comes before kmx_create.
#include <kmx.h>
#include <algorithm>
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
#include "kmx_pca_math.hpp"

namespace fs = std::filesystem;
using namespace kmxio;

namespace {

struct AOpt {
  std::string run, out, samples, evals, gram, from, scale = "eigenstrat";
  uint32_t gpus = 1, min_abund = 1, min_rec = 1, max_rec = 0xFFFFFFFFu, pcs = 10;
  bool has_gpus = false, has_abund = false, has_batch = false, has_pcs = false, has_scale = false, has_rec = false;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
  bool verbose = false;
};

const char* USAGE = "usage: kmx pca --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> [--samples FILE] "
                    "[--min-abund INT] [--scale eigenstrat|none] [--min-rec INT] [--max-rec INT] [--pcs INT=10] [--output FILE] [--evals FILE] "
                    "[--gram FILE] [--gpus INT] [--batch-mb INT] [-v]\n"
                    "       kmx pca --from-gram FILE [--pcs INT] [--output FILE] [--evals FILE]\n"
                    "  FILE of --samples: one sample id per line (default: every sample of the run, in the order of its kmtricks.fof).\n"
                    "  Prints, per sample, its coordinates on the first --pcs principal components of the samples' Gram matrix: every row is "
                    "centred at its frequency p among the samples and, with --scale eigenstrat, weighted by 1 / (p (1 - p)); a sample holds a row "
                    "from a count of --min-abund; rows held by fewer than --min-rec or more than --max-rec samples are left out (and so are rows held "
                    "by none or by all).  --evals writes all eigenvalues; --gram writes the matrix itself (--from-gram reads "
                    "it back).";

AOpt parse(int argc, char** argv)
{
  AOpt o;
  auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + USAGE); return argv[++i]; };
  auto num = [&](int& i) -> unsigned long { const std::string v = need(i); try { size_t n = 0; if (v.empty() || v[0] == '-') throw 1; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  auto u32 = [&](int& i) -> uint32_t { const unsigned long x = num(i); if (x > 0xFFFFFFFFul) die(std::string(argv[i - 1]) + " does not fit 32 bits"); return (uint32_t)x; };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = need(i);
    else if (a == "--from-gram") o.from = need(i);
    else if (a == "--output") o.out = need(i);
    else if (a == "--samples") o.samples = need(i);
    else if (a == "--evals") o.evals = need(i);
    else if (a == "--gram") o.gram = need(i);
    else if (a == "--scale") { o.scale = need(i); o.has_scale = true; if (o.scale != "eigenstrat" && o.scale != "none") die("--scale must be eigenstrat or none, not " + o.scale); }
    else if (a == "--min-abund") { o.min_abund = u32(i); o.has_abund = true; if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--min-rec") { o.min_rec = u32(i); o.has_rec = true; }
    else if (a == "--max-rec") { o.max_rec = u32(i); o.has_rec = true; }
    else if (a == "--pcs") { o.pcs = u32(i); o.has_pcs = true; if (o.pcs == 0) die("--pcs must be at least 1"); }
    else if (a == "--gpus") { o.gpus = u32(i); o.has_gpus = true; }
    else if (a == "--batch-mb") { o.batch_mb = num(i); o.has_batch = true; }
    else if (a == "-v" || a == "--verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') i++; }
    else die("unknown option " + a + "\n" + USAGE);
  }
  if (o.run.empty() == o.from.empty()) die(std::string("one of --run and --from-gram is required\n") + USAGE);
  if (!o.from.empty() && (!o.samples.empty() || !o.gram.empty() || o.has_abund || o.has_gpus || o.has_batch || o.has_scale || o.has_rec))
    die(std::string("--from-gram takes --pcs, --output and --evals alone\n") + USAGE);
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

void write_text(const std::string& path, const std::string& txt)      // "": standard output
{
  FILE* f = path.empty() ? stdout : fopen(path.c_str(), "w");
  if (!f) die("Unable to write at " + path);
  if (fwrite(txt.data(), 1, txt.size(), f) != txt.size()) die("write failed: " + (path.empty() ? std::string("stdout") : path));
  if (f != stdout) { if (fclose(f) != 0) die("write failed: " + path); } else fflush(stdout);
}

// the text of --gram: M and the ids in comment lines, then the M x M matrix, a row a line
std::string gram_text(const std::vector<std::string>& ids, const std::vector<double>& G)
{
  const size_t M = ids.size();
  std::string t = "# kmx pca gram\n# samples: " + std::to_string(M) + "\n";
  for (const std::string& s : ids) t += "# id: " + s + "\n";
  char num[64];
  for (size_t i = 0; i < M; i++)
    for (size_t j = 0; j < M; j++) { snprintf(num, sizeof num, "%.17g", G[i * M + j]); t += num; t += j + 1 < M ? '\t' : '\n'; }
  return t;
}

// ... read back: anything but the text above is refused
void read_gram(const std::string& path, std::vector<std::string>* ids, std::vector<double>* G)
{
  std::ifstream f(path);
  if (!f) die("Unable to read at " + path);
  auto bad = [&](uint64_t ln, const std::string& why) { die(path + " line " + std::to_string(ln) + ": " + why + " (not a file written by kmx pca --gram)"); };
  std::string line;
  uint64_t ln = 0, M = 0, next = 0;
  bool has_m = false;
  while (std::getline(f, line)) {
    ln++;
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    if (line[0] == '#') {
      if (next) bad(ln, "a comment inside the matrix");
      if (line.rfind("# samples: ", 0) == 0) {
        const std::string v = line.substr(11);
        if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos) bad(ln, "expected a sample count, found '" + v + "'");
        M = std::stoull(v); has_m = true;
        if (M < 2 || M > 32768) bad(ln, "a sample count outside [2, 32768]");
      } else if (line.rfind("# id: ", 0) == 0) ids->push_back(line.substr(6));
      continue;
    }
    if (!has_m) bad(ln, "the matrix starts before the samples line");
    if (ids->size() != M) bad(ln, std::to_string(ids->size()) + " id lines for " + std::to_string(M) + " samples");
    if (next == 0) G->assign(M * M, 0.0);
    if (next >= M) bad(ln, "more than M rows");
    std::istringstream is(line);
    std::string c;
    uint64_t j = 0;
    while (std::getline(is, c, '\t')) {
      if (j >= M) bad(ln, "more than M columns");
      char* end = nullptr;
      const double v = strtod(c.c_str(), &end);
      if (c.empty() || *end || !std::isfinite(v)) bad(ln, "expected a finite number, found '" + c + "'");
      (*G)[next * M + j++] = v;
    }
    if (j != M) bad(ln, "fewer than M columns");
    next++;
  }
  if (!has_m || next != M) die(path + ": the matrix ends before row M (not a file written by kmx pca --gram)");
  double big = 0.0;
  for (double v : *G) big = std::max(big, std::fabs(v));
  for (uint64_t i = 0; i < M; i++)
    for (uint64_t j = i + 1; j < M; j++) {
      double &a = (*G)[i * M + j], &b = (*G)[j * M + i];
      if (std::fabs(a - b) > 1e-12 * big) die(path + ": the matrix is not symmetric (not a file written by kmx pca --gram)");
      a = b = 0.5 * (a + b);
    }
}

// the eigen-solve and its texts
void solve_and_write(const AOpt& o, const std::vector<std::string>& ids, std::vector<double> G)
{
  const uint32_t M = (uint32_t)ids.size();
  const uint32_t k = o.has_pcs ? o.pcs : std::min<uint32_t>(o.pcs, M - 1);
  std::vector<double> val, vec;
  kmxpca::eigen_sym(M, G, &val, &vec);
  char num[64];
  if (!o.evals.empty()) {
    std::string t;
    for (uint32_t i = 0; i < M; i++) { snprintf(num, sizeof num, "%.17g\n", val[i]); t += num; }
    write_text(o.evals, t);
  }
  std::string t = "sample";
  for (uint32_t c = 1; c <= k; c++) t += "\tPC" + std::to_string(c);
  t += '\n';
  for (uint32_t i = 0; i < M; i++) {
    t += ids[i];
    for (uint32_t c = 0; c < k; c++) { snprintf(num, sizeof num, "\t%.10g", vec[(size_t)c * M + i]); t += num; }
    t += '\n';
  }
  write_text(o.out, t);
}

}  // namespace

int kmx_pca_main(int argc, char** argv)
{
  const AOpt o = parse(argc, argv);
  if (!o.from.empty()) {
    std::vector<std::string> ids; std::vector<double> G;
    read_gram(o.from, &ids, &G);
    if (o.has_pcs && o.pcs > ids.size() - 1) die("--pcs must be in [1, M - 1]: the matrix has " + std::to_string(ids.size()) + " samples");
    solve_and_write(o, ids, G);
    return 0;
  }
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
  else die("kmx pca needs a run made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin; " + run + " was made with " + mode);
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
  const std::vector<Sample> samples = parse_fof(run + "/kmtricks.fof", 1);
  const uint32_t N = (uint32_t)samples.size();
  if (N == 0) die(run + "/kmtricks.fof names no sample");
  if (N > 32768) die("kmx pca takes runs of at most 32768 samples; " + run + " has " + std::to_string(N));
  // the sample list: one id a line
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
  if (M < 2) die("kmx pca needs at least 2 samples; " + std::to_string(M) + " is listed");
  if (o.has_pcs && o.pcs > M - 1) die("--pcs must be in [1, M - 1]: " + std::to_string(M) + " samples are listed");
  const bool eigenstrat = o.scale == "eigenstrat";
  // classes outside [lo, hi] get the weight 0; a row held by none or by all is zero once centred, and p (1 - p) is 0 there
  const uint32_t lo = std::max<uint32_t>(1, o.min_rec), hi = std::min<uint32_t>(M - 1, o.max_rec);
  if (lo > hi) die("--min-rec " + std::to_string(o.min_rec) + " and --max-rec " + std::to_string(o.max_rec) + " leave no recurrence class of " + std::to_string(M) + " samples");
  std::vector<std::string> ids(M);
  for (uint32_t j = 0; j < M; j++) ids[j] = samples[cols.empty() ? j : cols[j]].id;
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
    if (!kd.kmer && !kd.pa && rd<uint32_t>(&h[21]) != 4) die(files[p] + " has counts of " + std::to_string(rd<uint32_t>(&h[21])) + " bytes: kmx pca reads 4-byte counts");
    if (!h[12]) {      // (an lz4 body's size is known once it is unpacked: checked when it is read)
      std::error_code ec;
      const uint64_t body = fs::file_size(files[p], ec) - kd.hdr;
      if (ec || body % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
    }
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
  // two runs are on the device at a time (one travels while the other is worked on); a row costs its bytes, 12 more in pass 1 (its
  // recurrence and place) and in pass 2 its bit in every sample block's slab, its recurrence and its place: 8 ceil(N / 64) + 8, and a
  // little more than that while few rows share the M + 1 classes' last words (left to the pool)
  const uint64_t per_row = stride + std::max<uint64_t>(12, 8ull * ((N + 63) / 64) + 8 + 1);
  const uint64_t run_rows = std::min<uint64_t>(std::max<uint64_t>(budget / 2 / per_row, 1), 0xFFFFFF00ull);
  if (o.verbose) fprintf(stderr, "[kmx pca] %u of %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", M, N, (unsigned long long)P,
                         mode.c_str(), (unsigned long long)stride, (unsigned long long)run_rows, G);

  const uint64_t M1 = (uint64_t)M + 1;
  std::vector<uint64_t> spec(3 * M1, 0), shared(M1 * N, 0), table((uint64_t)N * N, 0);
  std::vector<uint32_t> wt;
  std::mutex mu;
  // shard g: the partitions p with p mod G == g, one after the other, all into the tables of the shard's first call.  pass 1: kmx_pan_host
  // with KMX_PAN_SHARED; pass 2: kmx_gram_host with the weights pass 1 gave
  auto shard = [&](uint32_t g, int pass) {
    try {
      kmx_ctx* ctx = ctxs[g];
      void* first = nullptr;
      struct Flight { void* r; std::shared_ptr<std::vector<uint8_t>> body; };
      std::deque<Flight> flying;
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
          if (pass == 1) { chk(ctx, kmx_pan_result_wait((kmx_pan_result*)f.r), "kmx_pan"); if (f.r != first) kmx_pan_result_free((kmx_pan_result*)f.r); }
          else { chk(ctx, kmx_gram_result_wait((kmx_gram_result*)f.r), "kmx_gram"); if (f.r != first) kmx_gram_result_free((kmx_gram_result*)f.r); }
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        std::vector<uint8_t> raw = slurp(files[p]);
        auto body = std::make_shared<std::vector<uint8_t>>(body_of(raw, kd.hdr, kd.magic, files[p]));
        raw = std::vector<uint8_t>();
        if (body->size() % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
        const uint64_t rows = body->size() / stride;
        for (uint64_t r0 = 0; r0 < rows || (r0 == 0 && !first); r0 += run_rows) {      // (a shard's first call is made even for no rows: it owns the tables)
          const uint64_t nr = std::min(run_rows, rows - r0);
          const void* at = nr ? body->data() + r0 * stride : nullptr;
          void* r = nullptr;
          if (pass == 1) {
            kmx_pan_task t; memset(&t, 0, sizeof t);
            t.key_words = kw; t.mode = count ? KMX_MODE_COUNT : KMX_MODE_PA; t.n_cols = N; t.n_use = M;
            t.cols = cols.empty() ? nullptr : cols.data(); t.min_abund = o.min_abund; t.flags = KMX_PAN_SHARED;
            t.n_rows = nr; t.rows = at;
            t.spectrum = first ? kmx_pan_result_spectrum_dev((kmx_pan_result*)first) : nullptr;
            t.shared = first ? kmx_pan_result_shared_dev((kmx_pan_result*)first) : nullptr;
            kmx_pan_result* pr = nullptr;
            chk(ctx, kmx_pan_host(ctx, &t, &pr), "kmx_pan_host");
            if (!first) chk(ctx, kmx_pan_result_wait(pr), "kmx_pan");      // (its tables are asked for by the next call)
            r = pr;
          } else {
            kmx_gram_task t; memset(&t, 0, sizeof t);
            t.key_words = kw; t.mode = count ? KMX_MODE_COUNT : KMX_MODE_PA; t.n_cols = N; t.n_use = M;
            t.cols = cols.empty() ? nullptr : cols.data(); t.weights = wt.data(); t.min_abund = o.min_abund;
            t.n_rows = nr; t.rows = at;
            t.table = first ? kmx_gram_result_table_dev((kmx_gram_result*)first) : nullptr;
            kmx_gram_result* gr = nullptr;
            chk(ctx, kmx_gram_host(ctx, &t, &gr), "kmx_gram_host");
            if (!first) chk(ctx, kmx_gram_result_wait(gr), "kmx_gram");
            r = gr;
          }
          if (!first) first = r;
          flying.push_back({r, body});
          land(1);      // the run before this one has been worked on; this one travels
          if (rows == 0) break;
        }
      }
      land(0);
      if (!first) return;      // (more shards than partitions)
      if (pass == 1) {
        std::vector<uint64_t> sp(spec.size()), sh(shared.size());
        chk(ctx, kmx_pan_result_copy_spectrum((kmx_pan_result*)first, sp.data(), sp.size()), "kmx_pan_result_copy_spectrum");
        chk(ctx, kmx_pan_result_copy_shared((kmx_pan_result*)first, sh.data(), sh.size()), "kmx_pan_result_copy_shared");
        kmx_pan_result_free((kmx_pan_result*)first);
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < sp.size(); i++) spec[i] += sp[i];
        for (size_t i = 0; i < sh.size(); i++) shared[i] += sh[i];
      } else {
        std::vector<uint64_t> tb(table.size());
        chk(ctx, kmx_gram_result_copy_table((kmx_gram_result*)first, tb.data(), tb.size()), "kmx_gram_result_copy_table");
        kmx_gram_result_free((kmx_gram_result*)first);
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < tb.size(); i++) table[i] += tb[i];
      }
    } catch (const std::exception& e) { die(e.what()); }
  };
  auto pass = [&](int which) {
    std::vector<std::thread> workers;
    for (uint32_t g = 1; g < G; g++) workers.emplace_back(shard, g, which);
    shard(0, which);
    for (std::thread& w : workers) w.join();
  };
  pass(1);
  const kmxpca::Weights w = kmxpca::class_weights(M, spec.data(), lo, hi, eigenstrat);
  if (!w.ok) die("the rows' weights do not fit 63 bits even without a fraction: the run has too many rows for kmx pca");
  uint64_t all_rows = 0;
  for (uint64_t r = 0; r <= M; r++) all_rows += spec[r];
  if (o.verbose) fprintf(stderr, "[kmx pca] scale %s, F = %u, %llu of %llu rows used (recurrence %u ... %u)\n", o.scale.c_str(), w.F, (unsigned long long)w.n_used,
                         (unsigned long long)all_rows, lo, hi);
  if (w.n_used == 0) die("no row of the run has a recurrence in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]: nothing to compute the components from");
  wt = w.wt;
  pass(2);
  for (uint32_t g = 0; g < G; g++) kmx_destroy(ctxs[g]);

  std::vector<double> Gm = kmxpca::gram_matrix(M, N, cols.empty() ? nullptr : cols.data(), w, spec.data(), shared.data(), table.data());
  if (!o.gram.empty()) write_text(o.gram, gram_text(ids, Gm));
  solve_and_write(o, ids, Gm);
  return 0;
}
