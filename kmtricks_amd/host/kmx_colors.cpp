// kmx_colors.cpp -- `kmx colors`: the distinct sample sets of a run's rows and the rows of each (the colour classes of a coloured de
// Bruijn graph; the exclusive regions of the N-way Venn diagram, the bars of an UpSet plot; no counterpart in the kmtricks tree;
// include/kmx.h, section "colors").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a
// kmer run or the .count_hash / .pa_hash matrices of a hash run.  Every partition goes through kmx_colors_host in runs of rows that fit
// the device, two in flight; each call's class table is merged on the host into one map pattern -> (rows, id).  That is fine while
// classes are few beside rows; a matrix in which every row is its own class degrades to a host map of all rows.  Every check that needs
// no GPU comes before kmx_create.
#include <sstream>
#include "kmx_driver.hpp"

using namespace kmxdrv;

namespace {

struct COpt {
  std::string run, out, samples, ids;
  uint32_t gpus = 1, min_abund = 1;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
  uint64_t top = 0; bool has_top = false;
  bool verbose = false;
};

const char* USAGE = "usage: kmx colors --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> [--samples FILE] "
                    "[--min-abund INT] [--top INT] [--output FILE] [--ids DIR] [--gpus INT] [--batch-mb INT] [-v]\n"
                    "  FILE of --samples: one sample id per line, the samples in the order of the pattern's characters (default: every sample of the "
                    "run, in the order of its kmtricks.fof).\n"
                    "  Prints one line per distinct set of samples that holds a row: rank, rows, rec (samples in the set), the set as one character "
                    "0 / 1 a sample, and the ids of its samples; the sets with the most rows first (--top: the first INT only); a sample holds a row "
                    "from a count of --min-abund.  --ids writes DIR/ids_<p>.u32 for every partition: one little-endian u32 a row, its set's rank.";

COpt parse(int argc, char** argv)
{
  COpt o;
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--samples") o.samples = in.need(i);
    else if (a == "--ids") o.ids = in.need(i);
    else if (a == "--top") { o.top = in.num(i); o.has_top = true; }
    else if (a == "--min-abund") { o.min_abund = in.u32(i); if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--gpus") o.gpus = in.u32(i);
    else if (a == "--batch-mb") o.batch_mb = in.num(i);
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
}

typedef std::vector<uint64_t> Pattern;      // W words: ordinal j = bit j & 63 of word j >> 6
struct Class { uint64_t rows; uint32_t id; };

std::string bits_of(const Pattern& p, uint32_t M)
{
  std::string s(M, '0');
  for (uint32_t j = 0; j < M; j++) if ((p[j >> 6] >> (j & 63)) & 1) s[j] = '1';
  return s;
}

}  // namespace

int kmx_colors_main(int argc, char** argv)
{
  const COpt o = parse(argc, argv);
  // ---- the run directory; every check before kmx_create ----
  RunDir dir;
  dir.at("colors", o.run);
  dir.read_mode(MATRIX_KINDS, MATRIX_MODES);
  if (!dir.count() && o.min_abund > 1) die("--min-abund above 1 needs counts: " + dir.run + " was made with " + dir.mode);
  dir.shape();
  const uint32_t N = dir.N;
  const uint64_t P = dir.P;
  // the sample list: one id a line, in the order of the pattern's characters
  std::vector<uint32_t> cols;
  if (!o.samples.empty()) cols = read_sample_list(o.samples, dir.samples);
  const uint32_t M = o.samples.empty() ? N : (uint32_t)cols.size();
  const uint32_t W = (M + 63) / 64;
  std::vector<std::string> ids(M);
  for (uint32_t j = 0; j < M; j++) ids[j] = dir.samples[cols.empty() ? j : cols[j]].id;
  dir.open_files();

  // ---- devices; how many rows a run holds ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 4);
  // a row costs its bytes, the scratch per row at its most (8 W + 40) and what the result keeps per row (8 W + 12): include/kmx.h,
  // section "colors"
  const uint64_t per_row = dir.stride + 16ull * W + 52;
  const uint64_t rows_a_run = run_rows(dev.budget, per_row);
  if (o.verbose) fprintf(stderr, "[kmx colors] %u of %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", M, N, (unsigned long long)P,
                         dir.mode.c_str(), (unsigned long long)dir.stride, (unsigned long long)rows_a_run, dev.G());

  const bool want_ids = !o.ids.empty();
  std::map<Pattern, Class> table;                    // the global class table
  std::vector<std::vector<uint32_t>> part_ids(P);    // --ids: every row's global id, per partition in file order
  uint64_t total_rows = 0;
  std::mutex mu;
  // shard g: the partitions p with p mod G == g, one after the other
  in_shards(dev.G(), [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    struct Flight { kmx_colors_result* r; std::shared_ptr<std::vector<uint8_t>> body; uint64_t part, n_rows; };
    auto landed = [&](const Flight& f) {
      chk(ctx, kmx_colors_result_wait(f.r), "kmx_colors");
      const uint64_t C = kmx_colors_result_n_classes(f.r);
      std::vector<uint32_t> sizes(C), rid(want_ids ? f.n_rows : 0), global(C);
      std::vector<uint64_t> pats(C * W);
      chk(ctx, kmx_colors_result_copy_sizes(f.r, sizes.data(), C), "kmx_colors_result_copy_sizes");
      chk(ctx, kmx_colors_result_copy_patterns(f.r, pats.data(), C * W), "kmx_colors_result_copy_patterns");
      if (want_ids) chk(ctx, kmx_colors_result_copy_ids(f.r, rid.data(), f.n_rows), "kmx_colors_result_copy_ids");
      kmx_colors_result_free(f.r);
      {
        std::lock_guard<std::mutex> lk(mu);
        for (uint64_t c = 0; c < C; c++) {
          const Pattern p(pats.begin() + c * W, pats.begin() + (c + 1) * W);
          auto it = table.find(p);
          if (it == table.end()) {
            if (table.size() >= 0xFFFFFFFFull) die("more than 2^32 - 1 classes");
            it = table.emplace(p, Class{0, (uint32_t)table.size()}).first;
          }
          it->second.rows += sizes[c];
          global[c] = it->second.id;
        }
        total_rows += f.n_rows;
      }
      if (want_ids) for (uint32_t local : rid) {      // (a partition belongs to one shard, its runs land in order)
        if (local >= C) die("kmx_colors: a row's class is outside the call's table");
        part_ids[f.part].push_back(global[local]);
      }
    };
    TwoInFlight<Flight, decltype(landed)> runs(landed);
    for (uint64_t p = g; p < P; p += dev.G()) {
      auto body = dir.load(p);
      const uint64_t rows = body->size() / dir.stride;
      for (uint64_t r0 = 0; r0 < rows; r0 += rows_a_run) {
        kmx_colors_task t; memset(&t, 0, sizeof t);
        t.key_words = dir.kw; t.mode = dir.rmode(); t.n_cols = N; t.n_use = M;
        t.cols = cols.empty() ? nullptr : cols.data(); t.min_abund = o.min_abund;
        t.n_rows = std::min(rows_a_run, rows - r0);
        t.rows = body->data() + r0 * dir.stride;
        kmx_colors_result* r = nullptr;
        chk(ctx, kmx_colors_host(ctx, &t, &r), "kmx_colors_host");
        runs.put({r, body, p, t.n_rows});
      }
    }
    runs.finish();
  });
  dev.close();

  // ---- the table: rows descending, ties by the 0/1 string ascending ----
  struct Line { uint64_t rows; std::string bits; uint32_t id; };
  std::vector<Line> lines;
  lines.reserve(table.size());
  for (const auto& kv : table) lines.push_back({kv.second.rows, bits_of(kv.first, M), kv.second.id});
  std::sort(lines.begin(), lines.end(), [](const Line& a, const Line& b) { return a.rows != b.rows ? a.rows > b.rows : a.bits < b.bits; });
  const uint64_t shown = o.has_top ? std::min<uint64_t>(o.top, lines.size()) : lines.size();
  std::string t = "# kmx colors\n# samples: " + std::to_string(M) + "\n# rows: " + std::to_string(total_rows) + "\n# classes: " + std::to_string(lines.size()) +
                  "\n# min_abund: " + std::to_string(o.min_abund) + "\n# shown: " + std::to_string(shown) + "\nrank\trows\trec\tpattern\tsamples\n";
  for (uint64_t r = 0; r < shown; r++) {
    const Line& l = lines[r];
    std::string held; uint32_t rec = 0;
    for (uint32_t j = 0; j < M; j++) if (l.bits[j] == '1') { if (rec++) held += ','; held += ids[j]; }
    t += std::to_string(r) + "\t" + std::to_string(l.rows) + "\t" + std::to_string(rec) + "\t" + l.bits + "\t" + (rec ? held : std::string("-")) + "\n";
  }
  if (want_ids) {      // the rank in the FULL table, whatever --top says
    std::vector<uint32_t> rank(lines.size());
    for (size_t r = 0; r < lines.size(); r++) rank[lines[r].id] = (uint32_t)r;
    std::error_code ec;
    fs::create_directories(o.ids, ec);
    if (ec) die("Unable to write at " + o.ids);
    for (uint64_t p = 0; p < P; p++) {
      std::vector<uint8_t> le(4 * part_ids[p].size());
      for (size_t i = 0; i < part_ids[p].size(); i++) { const uint32_t v = rank[part_ids[p][i]]; for (int b = 0; b < 4; b++) le[4 * i + b] = (uint8_t)(v >> (8 * b)); }
      write_text(o.ids + "/ids_" + std::to_string(p) + ".u32", le.data(), le.size());
    }
  }
  write_text(o.out, t);
  return 0;
}
