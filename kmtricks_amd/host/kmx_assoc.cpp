// kmx_assoc.cpp -- `kmx assoc`: the structure-corrected association test of a run's rows (what kmdiff, EIGENSTRAT and a k-mer GWAS run once
// the samples' principal components are known; no counterpart in the kmtricks tree; include/kmx.h, section "assoc").  A phenotype --
// case/control or quantitative -- is regressed on each row's presence pattern with the covariates (the PCs `kmx pca` writes, or any
// others) in the model.  The design is made on the host (kmx_assoc_math.hpp): the covariates' orthonormal basis and the phenotype's
// residual, in fixed point.  Pass 1 sends every partition through kmx_pan_host for the rows by recurrence: the number of tests is the
// number of rows inside the recurrence window; the threshold follows from --alpha.  Pass 2 sends every partition through kmx_assoc_host
// in runs of rows, two in flight, and prints the kept rows.  `kmx assoc --design FILE --fof FOF ...` writes the design and asks for no
// device.  Every check that needs no GPU comes before kmx_create.
#include <cmath>
#include <sstream>
#include "kmx_driver.hpp"
#include "kmx_assoc_math.hpp"

using namespace kmxdrv;

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
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--fof") o.fof = in.need(i);
    else if (a == "--pheno") o.pheno = in.need(i);
    else if (a == "--groups") o.groups = in.need(i);
    else if (a == "--covar") o.covar = in.need(i);
    else if (a == "--design") o.design = in.need(i);
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--pcs") { o.pcs = in.u32(i); o.has_pcs = true; }
    else if (a == "--min-abund") { o.min_abund = in.u32(i); if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--min-rec") o.min_rec = std::max<uint32_t>(1, in.u32(i));
    else if (a == "--max-rec") { o.max_rec = in.u32(i); o.has_max = true; }
    else if (a == "--alpha") { o.alpha = in.real(i); if (!(o.alpha > 0.0 && o.alpha < 1.0)) die("--alpha must be inside (0, 1)"); }
    else if (a == "--correction") { o.correction = in.need(i); if (o.correction != "bonferroni" && o.correction != "none") die("--correction must be bonferroni or none"); }
    else if (a == "--counts") o.counts = true;
    else if (a == "--gpus") o.gpus = in.u32(i);
    else if (a == "--batch-mb") o.batch_mb = in.num(i);
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty() && (o.design.empty() || o.fof.empty())) die(std::string("--run, or --design with --fof, is required\n") + USAGE);
  if (!o.run.empty() && !o.fof.empty()) die(std::string("--fof goes with --design alone: a run has its own kmtricks.fof\n") + USAGE);
  if (o.pheno.empty() == o.groups.empty()) die(std::string("one of --pheno and --groups is required\n") + USAGE);
  if (o.has_pcs && o.covar.empty()) die("--pcs needs --covar");
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
}

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
  RunDir dir;
  if (!run.empty()) dir.at("assoc", run);
  // ---- the samples, the phenotype, the covariates, the design: no device ----
  const std::vector<Sample> samples = parse_fof(fof, 1);
  const uint32_t N = (uint32_t)samples.size();
  if (N == 0) die(fof + " names no sample");
  SampleIndex listed(samples);
  const std::vector<bool>& seen = listed.seen;
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
      const uint32_t at = listed.take(id, where, fof);
      double v = 0;
      if (o.pheno.empty()) {
        if (val != "case" && val != "control") die(where + "the label of " + id + " is " + val + ", neither case nor control");
        v = val == "case" ? 1.0 : 0.0;
      } else if (!number_of(val, &v)) die(where + "the phenotype of " + id + " is " + val + ", not a finite number");
      y_of[at] = v;
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
    SampleIndex rows(samples);
    std::vector<int64_t> row_of(N, -1);
    std::vector<double> all;
    uint64_t n_lines = 0;
    for (uint64_t ln = 2; std::getline(f, line); ln++) {
      std::istringstream is(line);
      std::string id, w;
      if (!(is >> id)) continue;
      const std::string where = o.covar + " line " + std::to_string(ln) + ": ";
      const uint32_t at = rows.take(id, where, fof);
      uint32_t n = 0;
      while (is >> w) {
        double v = 0;
        if (!number_of(w, &v)) die(where + "the value " + w + " of " + id + " is not a finite number");
        if (n < K) all.push_back(v);
        n++;
      }
      if (n != width) die(where + std::to_string(n) + " values, the header has " + std::to_string(width) + " columns");
      row_of[at] = (int64_t)n_lines++;
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
    write_text(o.design, t);
  }
  if (run.empty()) return 0;

  // ---- the run directory; every check before kmx_create ----
  dir.read_mode(MATRIX_KINDS, MATRIX_MODES);
  const Kind& kd = dir.kd;
  const bool count = dir.count();
  if (!count && o.min_abund > 1) die("--min-abund above 1 needs counts: " + run + " was made with " + dir.mode);
  dir.shape(samples);
  const uint32_t k = dir.k, kw = dir.kw;
  const uint64_t P = dir.P, stride = dir.stride;
  const uint32_t lo = std::max<uint32_t>(1, o.min_rec), hi = o.has_max ? std::min(o.max_rec, M) : M - 1;
  if (lo > hi) die("--min-rec " + std::to_string(o.min_rec) + " and --max-rec " + std::to_string(hi) + " leave no recurrence class of " + std::to_string(M) + " samples");
  dir.open_files();
  FILE* out = o.out.empty() ? stdout : fopen(o.out.c_str(), "w");
  if (!out) die("Unable to write at " + o.out);

  // ---- devices; how many rows a run holds ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 4);
  const uint32_t G = dev.G();
  // a row costs its bytes twice (the upload, the room for the kept rows), its keep word and two records (the scratch slot, the room for
  // the kept records)
  const uint64_t per_row = 2 * stride + 4 + 2 * sizeof(kmx_assoc_rec);
  const uint64_t rows_a_run = run_rows(dev.budget, per_row);
  const uint32_t rmode = dir.rmode();
  const bool all_listed = M == N;
  if (o.verbose) fprintf(stderr, "[kmx assoc] %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", (unsigned long long)P, dir.mode.c_str(),
                         (unsigned long long)stride, (unsigned long long)rows_a_run, G);

  // ---- pass 1: the rows by recurrence over the listed samples ----
  std::vector<uint64_t> spec;
  pan_pass(dir, dev, rows_a_run, all_listed ? nullptr : cols.data(), M, o.min_abund, &spec, nullptr);
  uint64_t n_tests = 0, n_all = 0;
  for (uint64_t r = 0; r <= M; r++) { n_all += spec[r]; if (r >= lo && r <= hi) n_tests += spec[r]; }
  const double p_cut = o.correction == "bonferroni" && n_tests ? o.alpha / (double)n_tests : o.alpha;
  const double thr = threshold_of(p_cut);
  if (o.verbose) fprintf(stderr, "[kmx assoc] %llu of %llu rows tested (recurrence %u ... %u), p <= %.6e, statistic >= %.17g\n", (unsigned long long)n_tests,
                         (unsigned long long)n_all, lo, hi, p_cut, thr);

  // ---- pass 2: the test; a partition's text is kept until every partition before it is out ----
  std::vector<std::string> text(P);
  in_shards(G, [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    struct Flight { kmx_assoc_result* r; std::shared_ptr<std::vector<uint8_t>> body; uint64_t p; };
    std::vector<uint8_t> kept;
    std::vector<kmx_assoc_rec> recs;
    char num[128];
    auto landed = [&](const Flight& f) {
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
    };
    TwoInFlight<Flight, decltype(landed)> runs(landed);
    for (uint64_t p = g; p < P; p += G) {
      auto body = dir.load(p);
      const uint64_t rows = body->size() / stride;
      for (uint64_t r0 = 0; r0 < rows; r0 += rows_a_run) {
        kmx_assoc_task t; memset(&t, 0, sizeof t);
        t.key_words = kw; t.mode = rmode; t.n_cols = N; t.n_use = M;
        t.cols = all_listed ? nullptr : cols.data(); t.min_abund = o.min_abund;
        t.n_rows = std::min(rows_a_run, rows - r0);
        t.rows = body->data() + r0 * stride;
        t.vecs = D.vecs.data(); t.n_vec = V; t.frac_bits = kmxassoc::FRAC_BITS;
        t.gain = D.gain; t.vmin = D.vmin; t.threshold = thr; t.min_rec = lo; t.max_rec = hi;
        kmx_assoc_result* r = nullptr;
        chk(ctx, kmx_assoc_host(ctx, &t, &r), "kmx_assoc_host");
        runs.put({r, body, p});
      }
    }
    runs.finish();
  });

  std::string head = std::string(kd.kmer ? "kmer" : "hash") + "\tpvalue\tstat\tbeta\trec";
  if (o.counts) for (const Sample& s : samples) { head += '\t'; head += s.id; }
  head += '\n';
  const std::string where = o.out.empty() ? std::string("stdout") : o.out;
  if (fwrite(head.data(), 1, head.size(), out) != head.size()) die("write failed: " + where);
  for (uint64_t p = 0; p < P; p++) if (fwrite(text[p].data(), 1, text[p].size(), out) != text[p].size()) die("write failed: " + where);
  if (out != stdout) { if (fclose(out) != 0) die("write failed: " + o.out); } else fflush(stdout);
  dev.close();
  return 0;
}
