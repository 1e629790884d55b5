// kmx_diff.cpp -- `kmx diff`: differential k-mer analysis of a run whose samples are split into cases and controls (what kmdiff does on
// top of kmtricks; no counterpart in the kmtricks tree).  Which rows (k-mers, hashes) of the run's matrices are significantly over- or
// under-represented in one group: a Poisson likelihood-ratio test per row (include/kmx.h, section "diff").  The input is the run
// directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run or the .count_hash / .pa_hash matrices of a
// hash run.  Pass 1 sends every partition through kmx_colsums_host for the per-sample totals and counts the rows; the threshold
// follows from --alpha (and the number of rows under Bonferroni); pass 2 sends every partition through kmx_diff_host in runs of rows,
// two in flight, and prints the kept rows.  Every check that needs no GPU comes before kmx_create.
#include <cmath>
#include <sstream>
#include "kmx_driver.hpp"

using namespace kmxdrv;

namespace {

struct FOpt {
  std::string run, groups, out, correction = "bonferroni";
  double alpha = 0.05;
  uint32_t gpus = 1, min_rec = 0;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
  bool counts = false, verbose = false;
};

const char* USAGE = "usage: kmx diff --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> --groups FILE "
                    "[--alpha 0.05] [--correction bonferroni|none] [--min-rec INT] [--counts] [--output FILE] [--gpus INT] [--batch-mb INT] [-v]\n"
                    "  FILE: one `sample_id case|control` per line; samples of the run that it does not name are ignored.\n"
                    "  Prints the rows whose counts differ between the groups (Poisson likelihood-ratio test, one degree of freedom): key, the group that "
                    "holds more, p, the statistic, the groups' sums and the numbers of their samples that hold the row.";

FOpt parse(int argc, char** argv)
{
  FOpt o;
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--groups") o.groups = in.need(i);
    else if (a == "--alpha") { o.alpha = in.real(i); if (!(o.alpha > 0.0 && o.alpha < 1.0)) die("--alpha must be inside (0, 1)"); }
    else if (a == "--correction") { o.correction = in.need(i); if (o.correction != "bonferroni" && o.correction != "none") die("--correction must be bonferroni or none"); }
    else if (a == "--min-rec") o.min_rec = in.u32(i);
    else if (a == "--counts") o.counts = true;
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--gpus") o.gpus = in.num(i);
    else if (a == "--batch-mb") o.batch_mb = in.num(i);
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
  if (o.groups.empty()) die(std::string("--groups is required\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
}

double p_of(double stat) { return std::erfc(std::sqrt(stat / 2.0)); }

// the smallest double t in [0, 2000] with erfc(sqrt(t / 2)) <= p
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

}  // namespace

int kmx_diff_main(int argc, char** argv)
{
  const FOpt o = parse(argc, argv);
  // ---- the run directory; every check before kmx_create ----
  RunDir dir;
  dir.at("diff", o.run);
  dir.read_mode(MATRIX_KINDS, MATRIX_MODES);
  dir.shape();
  const Kind& kd = dir.kd;
  const bool count = dir.count();
  const uint32_t N = dir.N, k = dir.k, kw = dir.kw;
  const uint64_t P = dir.P, stride = dir.stride;
  const std::vector<Sample>& samples = dir.samples;
  // the groups file: `id <whitespace> case|control` a line
  std::vector<uint8_t> group(N, 2);
  {
    std::ifstream f(o.groups);
    if (!f) die("Unable to read at " + o.groups);
    SampleIndex index(samples);
    std::string line;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
      std::istringstream is(line);
      std::string id, label, more;
      if (!(is >> id)) continue;      // an empty line
      const std::string where = o.groups + " line " + std::to_string(ln) + ": ";
      if (!(is >> label) || (is >> more)) die(where + "expected `sample_id case|control`");
      const uint32_t at = index.take(id, where);
      if (label != "case" && label != "control") die(where + "the label of " + id + " is " + label + ", neither case nor control");
      group[at] = label == "case" ? 1 : 0;
    }
    if (!std::count(group.begin(), group.end(), 0)) die(o.groups + " names no control sample");
    if (!std::count(group.begin(), group.end(), 1)) die(o.groups + " names no case sample");
  }
  dir.open_files();
  FILE* out = o.out.empty() ? stdout : fopen(o.out.c_str(), "w");
  if (!out) die("Unable to write at " + o.out);

  // ---- devices; how many rows a run holds ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 4);
  const uint32_t G = dev.G();
  // a row costs its bytes twice (the upload, the room for the kept rows), its keep word and two records (the scratch slot, the room for
  // the kept records)
  const uint64_t per_row = 2 * stride + 4 + 2 * sizeof(kmx_diff_rec);
  const uint64_t rows_a_run = run_rows(dev.budget, per_row);
  const uint32_t rmode = dir.rmode();
  if (o.verbose) fprintf(stderr, "[kmx diff] %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", N, (unsigned long long)P, dir.mode.c_str(),
                         (unsigned long long)stride, (unsigned long long)rows_a_run, G);

  // ---- pass 1: the per-sample totals and the number of rows ----
  std::vector<uint64_t> totals(N, 0);
  uint64_t M = 0;
  std::mutex mu;
  in_shards(G, [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    uint64_t m = 0;
    kmx_colsums_result* first = accumulate_runs<kmx_colsums_result>(dir, ctx, g, G, rows_a_run, [&](const uint8_t* rows, uint64_t n, kmx_colsums_result* first) {
      kmx_colsums_task t; memset(&t, 0, sizeof t);
      t.key_words = kw; t.mode = rmode; t.n_cols = N;
      t.n_rows = n; t.rows = rows;
      t.sums = first ? kmx_colsums_result_sums_dev(first) : nullptr;
      kmx_colsums_result* r = nullptr;
      chk(ctx, kmx_colsums_host(ctx, &t, &r), "kmx_colsums_host");
      m += n;
      return r;
    }, kmx_colsums_result_wait, kmx_colsums_result_free, "kmx_colsums");
    if (!first) return;      // (more shards than partitions)
    std::vector<uint64_t> s(N);
    chk(ctx, kmx_colsums_result_copy_sums(first, s.data(), s.size()), "kmx_colsums_result_copy_sums");
    kmx_colsums_result_free(first);
    std::lock_guard<std::mutex> lk(mu);
    for (uint32_t i = 0; i < N; i++) totals[i] += s[i];
    M += m;
  });
  unsigned __int128 t0 = 0, t1 = 0;
  for (uint32_t i = 0; i < N; i++) { if (group[i] == 0) t0 += totals[i]; else if (group[i] == 1) t1 += totals[i]; }
  if (o.verbose) for (uint32_t i = 0; i < N; i++)
    fprintf(stderr, "[kmx diff] %s\t%s\t%llu\n", samples[i].id.c_str(), group[i] == 0 ? "control" : group[i] == 1 ? "case" : "ignored", (unsigned long long)totals[i]);
  if (t0 == 0) die("the control samples hold nothing: no total to compare with");
  if (t1 == 0) die("the case samples hold nothing: no total to compare with");
  if ((t0 + t1) >> 64) die("the samples' totals do not fit 64 bits");
  const double p_cut = o.correction == "bonferroni" && M ? o.alpha / (double)M : o.alpha;
  const double thr = threshold_of(p_cut);
  if (o.verbose) fprintf(stderr, "[kmx diff] %llu rows, totals %llu (control) %llu (case), p <= %.6e, statistic >= %.17g\n", (unsigned long long)M,
                         (unsigned long long)t0, (unsigned long long)t1, p_cut, thr);

  // ---- pass 2: the test; a partition's text is kept until every partition before it is out ----
  std::vector<std::string> text(P);
  in_shards(G, [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    struct Flight { kmx_diff_result* r; std::shared_ptr<std::vector<uint8_t>> body; uint64_t p; };
    std::vector<uint8_t> kept;
    std::vector<kmx_diff_rec> recs;
    char num[96];
    auto landed = [&](const Flight& f) {
      chk(ctx, kmx_diff_result_wait(f.r), "kmx_diff");
      const uint64_t n = kmx_diff_result_rows(f.r);
      kept.resize(n * stride); recs.resize(n);
      chk(ctx, kmx_diff_result_copy_body(f.r, kept.data(), kept.size()), "kmx_diff_result_copy_body");
      chk(ctx, kmx_diff_result_copy_recs(f.r, recs.data(), recs.size()), "kmx_diff_result_copy_recs");
      kmx_diff_result_free(f.r);
      std::string& txt = text[f.p];
      for (uint64_t i = 0; i < n; i++) {
        const uint8_t* row = kept.data() + i * stride;
        const kmx_diff_rec& q = recs[i];
        txt += kd.kmer ? kmer_string(row, k) : std::to_string(rd<uint64_t>(row));
        txt += q.over == 1 ? "\tcase\t" : q.over == 2 ? "\tcontrol\t" : "\tnone\t";
        snprintf(num, sizeof num, "%.6e\t%.6f", p_of(q.stat), q.stat);
        txt += num;
        txt += '\t' + std::to_string(q.sum_ctrl) + '\t' + std::to_string(q.sum_case) + '\t' + std::to_string(q.rec_ctrl) + '\t' + std::to_string(q.rec_case);
        if (o.counts) for (uint32_t c = 0; c < N; c++) {
          txt += '\t';
          txt += count ? std::to_string(rd<uint32_t>(row + 8 * kw + 4ull * c)) : std::to_string((row[8 * kw + (c >> 3)] >> (c & 7)) & 1);
        }
        txt += '\n';
      }
    };
    TwoInFlight<Flight, decltype(landed)> runs(landed);
    for (uint64_t p = g; p < P; p += G) {
      auto body = dir.load(p);
      const uint64_t rows = body->size() / stride;
      for (uint64_t r0 = 0; r0 < rows; r0 += rows_a_run) {
        kmx_diff_task t; memset(&t, 0, sizeof t);
        t.key_words = kw; t.mode = rmode; t.n_cols = N; t.min_rec = o.min_rec;
        t.n_rows = std::min(rows_a_run, rows - r0);
        t.rows = body->data() + r0 * stride;
        t.group = group.data(); t.total_ctrl = (uint64_t)t0; t.total_case = (uint64_t)t1; t.threshold = thr;
        kmx_diff_result* r = nullptr;
        chk(ctx, kmx_diff_host(ctx, &t, &r), "kmx_diff_host");
        runs.put({r, body, p});
      }
    }
    runs.finish();
  });

  std::string head = std::string(kd.kmer ? "kmer" : "hash") + "\tover\tpvalue\tstat\tsum_ctrl\tsum_case\trec_ctrl\trec_case";
  if (o.counts) for (const Sample& s : samples) { head += '\t'; head += s.id; }
  head += '\n';
  const std::string where = o.out.empty() ? std::string("stdout") : o.out;
  if (fwrite(head.data(), 1, head.size(), out) != head.size()) die("write failed: " + where);
  for (uint64_t p = 0; p < P; p++) if (fwrite(text[p].data(), 1, text[p].size(), out) != text[p].size()) die("write failed: " + where);
  if (out != stdout) { if (fclose(out) != 0) die("write failed: " + o.out); } else fflush(stdout);
  dev.close();
  return 0;
}
