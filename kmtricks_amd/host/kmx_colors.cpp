// kmx_colors.cpp -- `kmx colors`: the distinct sample sets of a run's rows and the rows of each (the colour classes of a coloured de
// Bruijn graph; the exclusive regions of the N-way Venn diagram, the bars of an UpSet plot; no counterpart in the kmtricks tree;
// include/kmx.h, section "colors").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a
// kmer run or the .count_hash / .pa_hash matrices of a hash run.  Every partition goes through kmx_colors_host in runs of rows that fit
// the device, two in flight; each call's class table is merged on the host into one map pattern -> (rows, id).  That is fine while
// classes are few beside rows; a matrix in which every row is its own class degrades to a host map of all rows.  Every check that needs
// no GPU comes before kmx_create.
#include <kmx.h>
#include <algorithm>
#include <cstring>
#include <deque>
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
  auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + USAGE); return argv[++i]; };
  auto num = [&](int& i) -> unsigned long { const std::string v = need(i); try { size_t n = 0; if (v.empty() || v[0] == '-') throw 1; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  auto u32 = [&](int& i) -> uint32_t { const unsigned long x = num(i); if (x > 0xFFFFFFFFul) die(std::string(argv[i - 1]) + " does not fit 32 bits"); return (uint32_t)x; };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = need(i);
    else if (a == "--output") o.out = need(i);
    else if (a == "--samples") o.samples = need(i);
    else if (a == "--ids") o.ids = need(i);
    else if (a == "--top") { o.top = num(i); o.has_top = true; }
    else if (a == "--min-abund") { o.min_abund = u32(i); if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--gpus") o.gpus = u32(i);
    else if (a == "--batch-mb") o.batch_mb = num(i);
    else if (a == "-v" || a == "--verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') i++; }
    else die("unknown option " + a + "\n" + USAGE);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
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

void write_file(const std::string& path, const void* data, size_t n)      // "": standard output
{
  FILE* f = path.empty() ? stdout : fopen(path.c_str(), "wb");
  if (!f) die("Unable to write at " + path);
  if (n && fwrite(data, 1, n, f) != n) die("write failed: " + (path.empty() ? std::string("stdout") : path));
  if (f != stdout) { if (fclose(f) != 0) die("write failed: " + path); } else fflush(stdout);
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
  else die("kmx colors needs a run made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin; " + run + " was made with " + mode);
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
  // the sample list: one id a line, in the order of the pattern's characters
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
  const uint32_t W = (M + 63) / 64;
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
    if (!kd.kmer && !kd.pa && rd<uint32_t>(&h[21]) != 4) die(files[p] + " has counts of " + std::to_string(rd<uint32_t>(&h[21])) + " bytes: kmx colors reads 4-byte counts");
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
  // two runs are on the device at a time (one travels while the other is worked on); a row costs its bytes, the scratch per row at its
  // most (8 W + 40) and what the result keeps per row (8 W + 12): include/kmx.h, section "colors"
  const uint64_t per_row = stride + 16ull * W + 52;
  const uint64_t run_rows = std::min<uint64_t>(std::max<uint64_t>(budget / 2 / per_row, 1), 0xFFFFFF00ull);
  if (o.verbose) fprintf(stderr, "[kmx colors] %u of %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", M, N, (unsigned long long)P,
                         mode.c_str(), (unsigned long long)stride, (unsigned long long)run_rows, G);

  const bool want_ids = !o.ids.empty();
  std::map<Pattern, Class> table;                    // the global class table
  std::vector<std::vector<uint32_t>> part_ids(P);    // --ids: every row's global id, per partition in file order
  uint64_t total_rows = 0;
  std::mutex mu;
  // shard g: the partitions p with p mod G == g, one after the other
  auto shard = [&](uint32_t g) {
    try {
      kmx_ctx* ctx = ctxs[g];
      struct Flight { kmx_colors_result* r; std::shared_ptr<std::vector<uint8_t>> body; uint64_t part, n_rows; };
      std::deque<Flight> flying;
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
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
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        std::vector<uint8_t> raw = slurp(files[p]);
        auto body = std::make_shared<std::vector<uint8_t>>(body_of(raw, kd.hdr, kd.magic, files[p]));
        raw = std::vector<uint8_t>();
        if (body->size() % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
        const uint64_t rows = body->size() / stride;
        for (uint64_t r0 = 0; r0 < rows; r0 += run_rows) {
          kmx_colors_task t; memset(&t, 0, sizeof t);
          t.key_words = kw; t.mode = count ? KMX_MODE_COUNT : KMX_MODE_PA; t.n_cols = N; t.n_use = M;
          t.cols = cols.empty() ? nullptr : cols.data(); t.min_abund = o.min_abund;
          t.n_rows = std::min(run_rows, rows - r0);
          t.rows = body->data() + r0 * stride;
          kmx_colors_result* r = nullptr;
          chk(ctx, kmx_colors_host(ctx, &t, &r), "kmx_colors_host");
          flying.push_back({r, body, p, t.n_rows});
          land(1);      // the run before this one has been worked on; this one travels
        }
      }
      land(0);
    } catch (const std::exception& e) { die(e.what()); }
  };
  std::vector<std::thread> workers;
  for (uint32_t g = 1; g < G; g++) workers.emplace_back(shard, g);
  shard(0);
  for (std::thread& w : workers) w.join();
  for (uint32_t g = 0; g < G; g++) kmx_destroy(ctxs[g]);

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
      write_file(o.ids + "/ids_" + std::to_string(p) + ".u32", le.data(), le.size());
    }
  }
  write_file(o.out, t.data(), t.size());
  return 0;
}
