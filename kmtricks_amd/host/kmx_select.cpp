// kmx_select.cpp -- `kmx select`: a smaller run out of a larger one (what MUSET's `kmat_tools filter` does on the text of a kmtricks
// matrix; no counterpart in the kmtricks tree).  Some of the samples, in any order; the rows that enough -- and not too many -- of them
// hold, from an abundance upwards; counts kept, zeroed below the abundance, or turned into presence/absence bits (include/kmx.h, section
// "select").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run or the
// .count_hash / .pa_hash matrices of a hash run.  The output is a run directory of its own that every command reads as it reads the
// source.  Every partition goes through kmx_select_host in runs of rows, two in flight, and the kept rows are written as they land.
// Every check that needs no GPU comes before kmx_create, and before anything is written.
#include <cmath>
#include "kmx_driver.hpp"

using namespace kmxdrv;

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
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--samples") o.samples = in.need(i);
    else if (a == "--min-abund") { o.min_abund = in.u32(i); if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--min-rec") { o.min_rec = in.u32(i); o.has_min_rec = true; }
    else if (a == "--max-rec") { o.max_rec = in.u32(i); o.has_max_rec = true; }
    else if (a == "--min-frac") o.min_frac = in.frac(i);
    else if (a == "--max-frac") o.max_frac = in.frac(i);
    else if (a == "--pa") o.pa = true;
    else if (a == "--zero-below") o.zero_below = true;
    else if (a == "--cpr") o.cpr = true;
    else if (a == "--gpus") o.gpus = in.u32(i);
    else if (a == "--batch-mb") o.batch_mb = in.num(i);
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
  if (o.out.empty()) die(std::string("--output is required\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  if (o.has_min_rec && o.min_frac >= 0.0) die("--min-rec and --min-frac name the same bound: give one of them");
  if (o.has_max_rec && o.max_frac >= 0.0) die("--max-rec and --max-frac name the same bound: give one of them");
  if (o.zero_below && o.pa) die("--zero-below needs counts in the output: it cannot go with --pa");
  return o;
}

}  // namespace

int kmx_select_main(int argc, char** argv)
{
  const SOpt o = parse(argc, argv);
  // ---- the run directory; every check before kmx_create ----
  RunDir dir;
  dir.at("select", o.run);
  dir.read_mode(MATRIX_KINDS, MATRIX_MODES);
  const std::string& run = dir.run;
  const Kind& kd = dir.kd;
  const bool count = dir.count(), out_count = count && !o.pa;
  if (!count && o.min_abund > 1) die("--min-abund above 1 needs counts: " + run + " was made with " + dir.mode);
  if (!count && o.zero_below) die("--zero-below needs counts: " + run + " was made with " + dir.mode);
  dir.shape();
  const uint32_t N = dir.N, k = dir.k, kw = dir.kw;
  const uint64_t P = dir.P, stride = dir.stride;
  // the fof's lines as they stand, one a sample (parse_fof skips what is empty in the same way)
  std::vector<std::string> fof_lines;
  {
    std::ifstream f(run + "/kmtricks.fof"); std::string line;
    while (std::getline(f, line)) { while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back(); if (!line.empty()) fof_lines.push_back(line); }
    if (fof_lines.size() != N) die("fof: " + run + "/kmtricks.fof changed while it was read");
  }
  // the sample list: one id a line, the output's columns in its order
  std::vector<uint32_t> cols;
  if (!o.samples.empty()) cols = read_sample_list(o.samples, dir.samples);
  const uint32_t M = o.samples.empty() ? N : (uint32_t)cols.size();
  uint32_t min_rec = o.min_rec, max_rec = o.max_rec;
  if (o.min_frac >= 0.0) min_rec = (uint32_t)std::ceil(o.min_frac * (double)M);
  if (o.max_frac >= 0.0) max_rec = (uint32_t)std::floor(o.max_frac * (double)M);
  const uint64_t ostride = 8ull * kw + (out_count ? 4ull * M : (M + 7) / 8);
  dir.open_files();
  // the place of the output: a directory that is not there yet, or an empty one
  const std::string root = fs::absolute(o.out).string();
  {
    std::error_code ec;
    if (fs::exists(root, ec) && (!fs::is_directory(root, ec) || !fs::is_empty(root, ec))) die(o.out + " exists and is not an empty directory");
  }

  // ---- devices; how many rows a run holds ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 4);
  const uint32_t G = dev.G();
  // a row costs its bytes (the upload), the room for it at its new size, its keep word, its recurrence and its record
  const uint64_t per_row = stride + ostride + 8 + sizeof(kmx_select_rec);
  const uint64_t rows_a_run = run_rows(dev.budget, per_row);
  const uint32_t rmode = count ? KMX_MODE_COUNT : KMX_MODE_PA, omode = out_count ? KMX_MODE_COUNT : KMX_MODE_PA;
  const std::string oext = kd.kmer ? (out_count ? "count" : "pa") : (out_count ? "count_hash" : "pa_hash");
  if (o.verbose) fprintf(stderr, "[kmx select] %u of %u samples, %llu partitions (%s), rows of %llu -> %llu bytes, recurrence in [%u, %u], runs of %llu rows, %u shards\n", M, N,
                         (unsigned long long)P, dir.mode.c_str(), (unsigned long long)stride, (unsigned long long)ostride, min_rec, max_rec >= M ? M : max_rec,
                         (unsigned long long)rows_a_run, G);

  // ---- the run directory of the output ----
  fs::create_directories(root + "/matrices");
  {
    std::ofstream f(root + "/kmtricks.fof");
    for (uint32_t j = 0; j < M; j++) f << fof_lines[o.samples.empty() ? j : cols[j]] << "\n";
    if (!f) die("Unable to write at " + root + "/kmtricks.fof");
  }
  {
    std::string line = dir.opt;
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

  std::vector<uint64_t> rows_in(P, 0), rows_kept(P, 0);
  in_shards(G, [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    // (r null: a partition without a row, which still gets its header and its close)
    struct Flight { kmx_select_result* r; std::shared_ptr<std::vector<uint8_t>> body; std::shared_ptr<Out> file; uint64_t p; bool last; };
    std::vector<uint8_t> kept;
    auto landed = [&](const Flight& f) {
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
    };
    TwoInFlight<Flight, decltype(landed)> runs(landed);
    for (uint64_t p = g; p < P; p += G) {
      auto body = dir.load(p);
      const uint64_t rows = body->size() / stride;
      rows_in[p] = rows;
      auto file = std::make_shared<Out>(root + "/matrices/matrix_" + std::to_string(p) + "." + oext + (o.cpr ? ".lz4" : ""));
      if (kd.kmer) { if (out_count) matrix_count_header(*file, k, M, (uint32_t)p, o.cpr); else matrix_pa_header(*file, k, M, (uint32_t)p, o.cpr); }
      else { if (out_count) matrix_count_hash_header(*file, M, (uint32_t)p, o.cpr); else matrix_pa_hash_header(*file, M, (uint32_t)p, o.cpr); }
      if (rows == 0) { runs.put({nullptr, body, file, p, true}); continue; }
      for (uint64_t r0 = 0; r0 < rows; r0 += rows_a_run) {
        kmx_select_task t; memset(&t, 0, sizeof t);
        t.key_words = kw; t.mode = rmode; t.n_cols = N; t.n_out = M;
        t.n_rows = std::min(rows_a_run, rows - r0);
        t.rows = body->data() + r0 * stride;
        t.cols = o.samples.empty() ? nullptr : cols.data();
        t.min_abund = o.min_abund; t.min_rec = min_rec; t.max_rec = max_rec; t.out_mode = omode;
        t.flags = o.zero_below ? KMX_SELECT_ZERO_BELOW : 0;
        kmx_select_result* r = nullptr;
        chk(ctx, kmx_select_host(ctx, &t, &r), "kmx_select_host");
        runs.put({r, body, file, p, r0 + rows_a_run >= rows});
      }
    }
    runs.finish();
  });
  if (o.verbose) {
    uint64_t in = 0, out = 0;
    for (uint64_t p = 0; p < P; p++) {
      fprintf(stderr, "[kmx select] partition %llu: %llu rows in, %llu kept\n", (unsigned long long)p, (unsigned long long)rows_in[p], (unsigned long long)rows_kept[p]);
      in += rows_in[p]; out += rows_kept[p];
    }
    fprintf(stderr, "[kmx select] total: %llu rows in, %llu kept\n", (unsigned long long)in, (unsigned long long)out);
  }
  dev.close();
  return 0;
}
