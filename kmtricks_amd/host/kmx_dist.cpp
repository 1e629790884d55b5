// kmx_dist.cpp -- `kmx dist`: how the samples of a run relate to each other -- the sample-by-sample table of shared k-mers and the Jaccard
// and Bray-Curtis distances that follow from it (what Simka computes; no counterpart in the kmtricks tree).  The input is the run
// directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run, the .count_hash / .pa_hash matrices of a
// hash run, or the .cmbf Bloom matrices of a hash:bf:bin run (there the numbers count Bloom bits: an estimate).  Every partition goes
// through kmx_dist_host in runs of rows that fit the device; all of them add into one table per device, the devices' tables are summed
// on the host.  Every check that needs no GPU comes before kmx_create.
#include "kmx_driver.hpp"

using namespace kmxdrv;

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
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--metric") { o.metric = in.need(i); if (o.metric != "shared" && o.metric != "jaccard" && o.metric != "braycurtis") die("--metric must be shared, jaccard or braycurtis"); }
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--gpus") o.gpus = in.num(i);
    else if (a == "--batch-mb") o.batch_mb = in.num(i);
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
}

}  // namespace

int kmx_dist_main(int argc, char** argv)
{
  const DOpt o = parse(argc, argv);
  // ---- the run directory; every check before kmx_create ----
  RunDir dir;
  dir.at("dist", o.run);
  dir.read_mode(ALL_KINDS, "kmer:count:bin, kmer:pa:bin, hash:count:bin, hash:pa:bin or hash:bf:bin");
  if (o.metric == "braycurtis" && !dir.count())
    die("--metric braycurtis needs a count run (kmer:count:bin or hash:count:bin): " + dir.run + " was made with " + dir.mode + " and has no counts");
  dir.shape();
  const uint32_t N = dir.N;
  const std::vector<Sample>& samples = dir.samples;
  if (N > 32768) die("kmx dist takes at most 32768 samples (a table would be 8 GiB)");
  dir.open_files();
  FILE* out = o.out.empty() ? stdout : fopen(o.out.c_str(), "w");
  if (!out) die("Unable to write at " + o.out);

  // ---- devices; how many rows a run holds ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 4);
  // a row costs its bytes and its presence bits
  const uint64_t per_row = dir.stride + ((uint64_t)N + 63) / 64 * 8;
  const uint64_t rows_a_run = run_rows(dev.budget, per_row);
  const bool want_mins = o.metric == "braycurtis";
  if (o.verbose) fprintf(stderr, "[kmx dist] %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", N, (unsigned long long)dir.P, dir.mode.c_str(),
                         (unsigned long long)dir.stride, (unsigned long long)rows_a_run, dev.G());

  const uint64_t cells = (uint64_t)N * N;
  std::vector<uint64_t> inter(cells, 0), mins(want_mins ? cells : 0, 0);
  std::mutex mu;
  // shard g: the partitions p with p mod G == g, one after the other, all into the table of the shard's first call
  in_shards(dev.G(), [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    kmx_dist_result* first = accumulate_runs<kmx_dist_result>(dir, ctx, g, dev.G(), rows_a_run, [&](const uint8_t* rows, uint64_t n, kmx_dist_result* first) {
      kmx_dist_task t; memset(&t, 0, sizeof t);
      t.key_words = dir.kw; t.mode = dir.rmode(); t.n_cols = N; t.want_mins = want_mins ? 1 : 0;
      t.n_rows = n; t.rows = rows;
      t.inter = first ? kmx_dist_result_inter_dev(first) : nullptr;
      t.mins = first && want_mins ? kmx_dist_result_mins_dev(first) : nullptr;
      kmx_dist_result* r = nullptr;
      chk(ctx, kmx_dist_host(ctx, &t, &r), "kmx_dist_host");
      return r;
    }, kmx_dist_result_wait, kmx_dist_result_free, "kmx_dist");
    if (!first) return;      // (more shards than partitions)
    std::vector<uint64_t> si(cells), sm(want_mins ? cells : 0);
    chk(ctx, kmx_dist_result_copy_inter(first, si.data(), si.size()), "kmx_dist_result_copy_inter");
    if (want_mins) chk(ctx, kmx_dist_result_copy_mins(first, sm.data(), sm.size()), "kmx_dist_result_copy_mins");
    kmx_dist_result_free(first);
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < si.size(); i++) inter[i] += si[i];
    for (size_t i = 0; i < sm.size(); i++) mins[i] += sm[i];
  });

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
  dev.close();
  return 0;
}
