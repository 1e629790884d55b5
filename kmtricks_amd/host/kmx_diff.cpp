// kmx_diff.cpp -- `kmx diff`: differential k-mer analysis of a run whose samples are split into cases and controls (what kmdiff does on
// top of kmtricks; no counterpart in the kmtricks tree).  Which rows (k-mers, hashes) of the run's matrices are significantly over- or
// under-represented in one group: a Poisson likelihood-ratio test per row (include/kmx.h, section "diff").  The input is the run
// directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run or the .count_hash / .pa_hash matrices of a
// hash run.  Pass 1 sends every partition through kmx_colsums_host for the per-sample totals and counts the rows; the threshold
// follows from --alpha (and the number of rows under Bonferroni); pass 2 sends every partition through kmx_diff_host in runs of rows,
// two in flight, and prints the kept rows.  Every check that needs no GPU comes before kmx_create.
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
  auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + USAGE); return argv[++i]; };
  auto num = [&](int& i) -> unsigned long { const std::string v = need(i); try { size_t n = 0; if (v.empty() || v[0] == '-') throw 1; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = need(i);
    else if (a == "--groups") o.groups = need(i);
    else if (a == "--alpha") {
      const std::string v = need(i);
      try { size_t n = 0; o.alpha = std::stod(v, &n); if (n != v.size()) throw 1; } catch (...) { die("bad number for --alpha: " + v); }
      if (!(o.alpha > 0.0 && o.alpha < 1.0)) die("--alpha must be inside (0, 1)");
    }
    else if (a == "--correction") { o.correction = need(i); if (o.correction != "bonferroni" && o.correction != "none") die("--correction must be bonferroni or none"); }
    else if (a == "--min-rec") { const unsigned long x = num(i); if (x > 0xFFFFFFFFul) die("--min-rec does not fit 32 bits"); o.min_rec = (uint32_t)x; }
    else if (a == "--counts") o.counts = true;
    else if (a == "--output") o.out = need(i);
    else if (a == "--gpus") o.gpus = num(i);
    else if (a == "--batch-mb") o.batch_mb = num(i);
    else if (a == "-v" || a == "--verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') i++; }
    else die("unknown option " + a + "\n" + USAGE);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
  if (o.groups.empty()) die(std::string("--groups is required\n") + USAGE);
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
  else die("kmx diff needs a run made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin; " + run + " was made with " + mode);
  const bool count = !kd.pa;
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
  // the groups file: `id <whitespace> case|control` a line
  std::vector<uint8_t> group(N, 2);
  {
    std::ifstream f(o.groups);
    if (!f) die("Unable to read at " + o.groups);
    std::map<std::string, uint32_t> at;
    for (uint32_t i = 0; i < N; i++) at[samples[i].id] = i;
    std::vector<bool> seen(N, false);
    std::string line;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
      std::istringstream is(line);
      std::string id, label, more;
      if (!(is >> id)) continue;      // an empty line
      const std::string where = o.groups + " line " + std::to_string(ln) + ": ";
      if (!(is >> label) || (is >> more)) die(where + "expected `sample_id case|control`");
      const auto it = at.find(id);
      if (it == at.end()) die(where + "sample " + id + " is not in the run's kmtricks.fof");
      if (seen[it->second]) die(where + "sample " + id + " is named twice");
      if (label != "case" && label != "control") die(where + "the label of " + id + " is " + label + ", neither case nor control");
      seen[it->second] = true;
      group[it->second] = label == "case" ? 1 : 0;
    }
    if (!std::count(group.begin(), group.end(), 0)) die(o.groups + " names no control sample");
    if (!std::count(group.begin(), group.end(), 1)) die(o.groups + " names no case sample");
  }
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
    const uint32_t cols = rd<uint32_t>(&h[kd.cols_at]);
    if (cols != N) die(files[p] + " has rows of " + std::to_string(cols) + " columns, the run's kmtricks.fof has " + std::to_string(N) + " samples");
    if (kd.pa && rd<uint32_t>(&h[kd.cols_at + 4]) != (N + 7) / 8) die("Invalid file format: " + files[p]);
    if (!kd.kmer && !kd.pa && rd<uint32_t>(&h[21]) != 4) die(files[p] + " has counts of " + std::to_string(rd<uint32_t>(&h[21])) + " bytes: kmx diff reads 4-byte counts");
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
  const uint64_t per_row = 2 * stride + 4 + 2 * sizeof(kmx_diff_rec);
  const uint64_t run_rows = std::min<uint64_t>(std::max<uint64_t>(budget / 2 / per_row, 1), 0xFFFFFF00ull);
  const uint32_t rmode = count ? KMX_MODE_COUNT : KMX_MODE_PA;
  if (o.verbose) fprintf(stderr, "[kmx diff] %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", N, (unsigned long long)P, mode.c_str(),
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

  // ---- pass 1: the per-sample totals and the number of rows ----
  std::vector<uint64_t> totals(N, 0);
  uint64_t M = 0;
  std::mutex mu;
  in_shards([&](uint32_t g) {
    try {
      kmx_ctx* ctx = ctxs[g];
      kmx_colsums_result* first = nullptr;
      struct Flight { kmx_colsums_result* r; std::shared_ptr<std::vector<uint8_t>> body; };
      std::deque<Flight> flying;
      uint64_t m = 0;
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
          chk(ctx, kmx_colsums_result_wait(f.r), "kmx_colsums");
          if (f.r != first) kmx_colsums_result_free(f.r);
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        auto body = load(p);
        const uint64_t rows = body->size() / stride;
        m += rows;
        for (uint64_t r0 = 0; r0 < rows || (r0 == 0 && !first); r0 += run_rows) {      // (a shard's first call is made even for no rows: it owns the table)
          kmx_colsums_task t; memset(&t, 0, sizeof t);
          t.key_words = kw; t.mode = rmode; t.n_cols = N;
          t.n_rows = std::min(run_rows, rows - r0);
          t.rows = t.n_rows ? body->data() + r0 * stride : nullptr;
          t.sums = first ? kmx_colsums_result_sums_dev(first) : nullptr;
          kmx_colsums_result* r = nullptr;
          chk(ctx, kmx_colsums_host(ctx, &t, &r), "kmx_colsums_host");
          if (!first) { first = r; chk(ctx, kmx_colsums_result_wait(r), "kmx_colsums"); }      // (its table is asked for by the next call)
          flying.push_back({r, body});
          land(1);      // the run before this one has been worked on; this one travels
          if (rows == 0) break;
        }
      }
      land(0);
      if (!first) return;      // (more shards than partitions)
      std::vector<uint64_t> s(N);
      chk(ctx, kmx_colsums_result_copy_sums(first, s.data(), s.size()), "kmx_colsums_result_copy_sums");
      kmx_colsums_result_free(first);
      std::lock_guard<std::mutex> lk(mu);
      for (uint32_t i = 0; i < N; i++) totals[i] += s[i];
      M += m;
    } catch (const std::exception& e) { die(e.what()); }
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
  in_shards([&](uint32_t g) {
    try {
      kmx_ctx* ctx = ctxs[g];
      struct Flight { kmx_diff_result* r; std::shared_ptr<std::vector<uint8_t>> body; uint64_t p, r0; };
      std::deque<Flight> flying;
      std::vector<uint8_t> kept;
      std::vector<kmx_diff_rec> recs;
      char num[96];
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
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
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        auto body = load(p);
        const uint64_t rows = body->size() / stride;
        for (uint64_t r0 = 0; r0 < rows; r0 += run_rows) {
          kmx_diff_task t; memset(&t, 0, sizeof t);
          t.key_words = kw; t.mode = rmode; t.n_cols = N; t.min_rec = o.min_rec;
          t.n_rows = std::min(run_rows, rows - r0);
          t.rows = body->data() + r0 * stride;
          t.group = group.data(); t.total_ctrl = (uint64_t)t0; t.total_case = (uint64_t)t1; t.threshold = thr;
          kmx_diff_result* r = nullptr;
          chk(ctx, kmx_diff_host(ctx, &t, &r), "kmx_diff_host");
          flying.push_back({r, body, p, r0});
          land(1);      // the run before this one has been worked on; this one travels
        }
      }
      land(0);
    } catch (const std::exception& e) { die(e.what()); }
  });

  std::string head = std::string(kd.kmer ? "kmer" : "hash") + "\tover\tpvalue\tstat\tsum_ctrl\tsum_case\trec_ctrl\trec_case";
  if (o.counts) for (const Sample& s : samples) { head += '\t'; head += s.id; }
  head += '\n';
  const std::string where = o.out.empty() ? std::string("stdout") : o.out;
  if (fwrite(head.data(), 1, head.size(), out) != head.size()) die("write failed: " + where);
  for (uint64_t p = 0; p < P; p++) if (fwrite(text[p].data(), 1, text[p].size(), out) != text[p].size()) die("write failed: " + where);
  if (out != stdout) { if (fclose(out) != 0) die("write failed: " + o.out); } else fflush(stdout);
  for (uint32_t g = 0; g < G; g++) kmx_destroy(ctxs[g]);
  return 0;
}
