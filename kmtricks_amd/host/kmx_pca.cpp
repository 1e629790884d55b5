// kmx_pca.cpp -- `kmx pca`: the principal components of a run's samples (what EIGENSTRAT / smartpca compute from genotypes, here from
// the k-mer x sample matrix: every row centred at its own frequency p and weighted by 1 / (p (1 - p)); no counterpart in the kmtricks
// tree; include/kmx.h, section "gram").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices
// of a kmer run or the .count_hash / .pa_hash matrices of a hash run.  Pass 1 sends every partition through kmx_pan_host (the rows by
// recurrence, and per sample); the class weights in fixed point follow from it (kmx_pca_math.hpp); pass 2 sends every partition through
// kmx_gram_host in runs of rows, two in flight, all into one table per device; the devices' tables are summed on the host, where the
// Gram matrix is centred and diagonalised.  `kmx pca --from-gram FILE` diagonalises a matrix saved with --gram and asks for no device.
// Every check that needs no GPU comes before kmx_create.
#include <sstream>
#include "kmx_driver.hpp"
#include "kmx_pca_math.hpp"

using namespace kmxdrv;

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
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--from-gram") o.from = in.need(i);
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--samples") o.samples = in.need(i);
    else if (a == "--evals") o.evals = in.need(i);
    else if (a == "--gram") o.gram = in.need(i);
    else if (a == "--scale") { o.scale = in.need(i); o.has_scale = true; if (o.scale != "eigenstrat" && o.scale != "none") die("--scale must be eigenstrat or none, not " + o.scale); }
    else if (a == "--min-abund") { o.min_abund = in.u32(i); o.has_abund = true; if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--min-rec") { o.min_rec = in.u32(i); o.has_rec = true; }
    else if (a == "--max-rec") { o.max_rec = in.u32(i); o.has_rec = true; }
    else if (a == "--pcs") { o.pcs = in.u32(i); o.has_pcs = true; if (o.pcs == 0) die("--pcs must be at least 1"); }
    else if (a == "--gpus") { o.gpus = in.u32(i); o.has_gpus = true; }
    else if (a == "--batch-mb") { o.batch_mb = in.num(i); o.has_batch = true; }
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty() == o.from.empty()) die(std::string("one of --run and --from-gram is required\n") + USAGE);
  if (!o.from.empty() && (!o.samples.empty() || !o.gram.empty() || o.has_abund || o.has_gpus || o.has_batch || o.has_scale || o.has_rec))
    die(std::string("--from-gram takes --pcs, --output and --evals alone\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
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
  // ---- the run directory; every check before kmx_create ----
  RunDir dir;
  dir.at("pca", o.run);
  dir.read_mode(MATRIX_KINDS, MATRIX_MODES);
  if (!dir.count() && o.min_abund > 1) die("--min-abund above 1 needs counts: " + dir.run + " was made with " + dir.mode);
  dir.shape();
  const uint32_t N = dir.N;
  if (N > 32768) die("kmx pca takes runs of at most 32768 samples; " + dir.run + " has " + std::to_string(N));
  // the sample list: one id a line
  std::vector<uint32_t> cols;
  if (!o.samples.empty()) cols = read_sample_list(o.samples, dir.samples);
  const uint32_t M = o.samples.empty() ? N : (uint32_t)cols.size();
  if (M < 2) die("kmx pca needs at least 2 samples; " + std::to_string(M) + " is listed");
  if (o.has_pcs && o.pcs > M - 1) die("--pcs must be in [1, M - 1]: " + std::to_string(M) + " samples are listed");
  const bool eigenstrat = o.scale == "eigenstrat";
  // classes outside [lo, hi] get the weight 0; a row held by none or by all is zero once centred, and p (1 - p) is 0 there
  const uint32_t lo = std::max<uint32_t>(1, o.min_rec), hi = std::min<uint32_t>(M - 1, o.max_rec);
  if (lo > hi) die("--min-rec " + std::to_string(o.min_rec) + " and --max-rec " + std::to_string(o.max_rec) + " leave no recurrence class of " + std::to_string(M) + " samples");
  std::vector<std::string> ids(M);
  for (uint32_t j = 0; j < M; j++) ids[j] = dir.samples[cols.empty() ? j : cols[j]].id;
  dir.open_files();

  // ---- devices; how many rows a run holds ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 4);
  // a row costs its bytes, 12 more in pass 1 (its recurrence and place) and in pass 2 its bit in every sample block's slab, its
  // recurrence and its place: 8 ceil(N / 64) + 8, and a little more than that while few rows share the M + 1 classes' last words (left
  // to the pool)
  const uint64_t per_row = dir.stride + std::max<uint64_t>(12, 8ull * ((N + 63) / 64) + 8 + 1);
  const uint64_t rows_a_run = run_rows(dev.budget, per_row);
  if (o.verbose) fprintf(stderr, "[kmx pca] %u of %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", M, N, (unsigned long long)dir.P,
                         dir.mode.c_str(), (unsigned long long)dir.stride, (unsigned long long)rows_a_run, dev.G());

  // ---- pass 1: the rows by recurrence, and per sample (kmx_pan_host with KMX_PAN_SHARED) ----
  std::vector<uint64_t> spec, shared;
  pan_pass(dir, dev, rows_a_run, cols.empty() ? nullptr : cols.data(), M, o.min_abund, &spec, &shared);
  const kmxpca::Weights w = kmxpca::class_weights(M, spec.data(), lo, hi, eigenstrat);
  if (!w.ok) die("the rows' weights do not fit 63 bits even without a fraction: the run has too many rows for kmx pca");
  uint64_t all_rows = 0;
  for (uint64_t r = 0; r <= M; r++) all_rows += spec[r];
  if (o.verbose) fprintf(stderr, "[kmx pca] scale %s, F = %u, %llu of %llu rows used (recurrence %u ... %u)\n", o.scale.c_str(), w.F, (unsigned long long)w.n_used,
                         (unsigned long long)all_rows, lo, hi);
  if (w.n_used == 0) die("no row of the run has a recurrence in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]: nothing to compute the components from");

  // ---- pass 2: kmx_gram_host with the weights pass 1 gave, a shard's partitions into the table of its first call ----
  std::vector<uint64_t> table((uint64_t)N * N, 0);
  std::mutex mu;
  in_shards(dev.G(), [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    kmx_gram_result* first = accumulate_runs<kmx_gram_result>(dir, ctx, g, dev.G(), rows_a_run, [&](const uint8_t* rows, uint64_t n, kmx_gram_result* first) {
      kmx_gram_task t; memset(&t, 0, sizeof t);
      t.key_words = dir.kw; t.mode = dir.rmode(); t.n_cols = N; t.n_use = M;
      t.cols = cols.empty() ? nullptr : cols.data(); t.weights = w.wt.data(); t.min_abund = o.min_abund;
      t.n_rows = n; t.rows = rows;
      t.table = first ? kmx_gram_result_table_dev(first) : nullptr;
      kmx_gram_result* r = nullptr;
      chk(ctx, kmx_gram_host(ctx, &t, &r), "kmx_gram_host");
      return r;
    }, kmx_gram_result_wait, kmx_gram_result_free, "kmx_gram");
    if (!first) return;      // (more shards than partitions)
    std::vector<uint64_t> tb(table.size());
    chk(ctx, kmx_gram_result_copy_table(first, tb.data(), tb.size()), "kmx_gram_result_copy_table");
    kmx_gram_result_free(first);
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < tb.size(); i++) table[i] += tb[i];
  });
  dev.close();

  std::vector<double> Gm = kmxpca::gram_matrix(M, N, cols.empty() ? nullptr : cols.data(), w, spec.data(), shared.data(), table.data());
  if (!o.gram.empty()) write_text(o.gram, gram_text(ids, Gm));
  solve_and_write(o, ids, Gm);
  return 0;
}
