// kmx_spectra.cpp -- `kmx spectra`: the abundance spectrum of every listed sample of a run and the joint spectrum of pairs of samples (what
// KAT `hist` / `comp` and Merqury's spectra-cn tabulate; no counterpart in the kmtricks tree; include/kmx.h, section "spectra"), and what
// follows from them: rows held, singletons, volume, valley and peak a sample; shared and exclusive rows, Jaccard index, k-mer completeness
// and consensus quality a pair (kmx_spectra_stats.hpp).  The input is the run directory as `kmx pipeline` / kmtricks leave it.  Every
// partition goes through kmx_spectra_host in runs of rows that fit the device, two in flight; all of them add into one pair of tables per
// device, the devices' tables are summed on the host.  `kmx spectra --from-tables` prints the statistics of tables saved with --hist /
// --joint and asks for no device.  Every check that needs no GPU comes before kmx_create.
#include <sstream>
#include "kmx_driver.hpp"
#include "kmx_spectra_stats.hpp"

using namespace kmxdrv;

namespace {

struct SOpt {
  std::string run, out, samples, pairs, against, hist, joint, from;
  uint32_t gpus = 1, cap = 255, joint_cap = 63, solid = 1, k = 0;
  bool all_pairs = false, has_gpus = false, has_batch = false, has_cap = false, has_jcap = false, has_solid = false, has_k = false;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
  bool verbose = false;
};

const char* USAGE = "usage: kmx spectra --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> [--samples FILE] "
                    "[--cap INT=255] [--pairs FILE | --against ID | --all-pairs] [--joint-cap INT=63] [--solid INT=1] [--hist FILE] [--joint FILE] "
                    "[--output FILE] [--gpus INT] [--batch-mb INT] [-v]\n"
                    "       kmx spectra --from-tables HIST_FILE [--joint JOINT_FILE --kmer-size K] [--solid INT] [--output FILE]\n"
                    "  FILE of --samples: one sample id per line (default: every sample of the run, in the order of its kmtricks.fof).  FILE of "
                    "--pairs: two sample ids per line, x then y; --against ID: (ID, s) for every listed s other than ID; --all-pairs: every "
                    "unordered pair of the list.\n"
                    "  Prints, per listed sample: the rows it holds, its singletons, its volume (the sum of its counts) and the part of it in "
                    "counts of --cap and more, the valley and the peak of its abundance spectrum; per pair: the rows in both, in x only, in y only, "
                    "the Jaccard index, the completeness of y against the rows x holds at least --solid times, and for a kmer run the consensus "
                    "quality of y against x over distinct k-mers.  --hist and --joint write the tables themselves (--from-tables reads them back).";

SOpt parse(int argc, char** argv)
{
  SOpt o;
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--from-tables") o.from = in.need(i);
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--samples") o.samples = in.need(i);
    else if (a == "--pairs") o.pairs = in.need(i);
    else if (a == "--against") o.against = in.need(i);
    else if (a == "--all-pairs") o.all_pairs = true;
    else if (a == "--hist") o.hist = in.need(i);
    else if (a == "--joint") o.joint = in.need(i);
    else if (a == "--cap") { o.cap = in.u32(i); o.has_cap = true; if (o.cap < 1 || o.cap > 65535) die("--cap must be in [1, 65535]"); }
    else if (a == "--joint-cap") { o.joint_cap = in.u32(i); o.has_jcap = true; if (o.joint_cap < 1 || o.joint_cap > 255) die("--joint-cap must be in [1, 255]"); }
    else if (a == "--solid") { o.solid = in.u32(i); o.has_solid = true; if (o.solid < 1) die("--solid must be at least 1"); }
    else if (a == "--kmer-size") { o.k = in.u32(i); o.has_k = true; if (o.k < 8 || o.k > 127) die("--kmer-size must be in [8, 127]"); }
    else if (a == "--gpus") { o.gpus = in.u32(i); o.has_gpus = true; }
    else if (a == "--batch-mb") { o.batch_mb = in.num(i); o.has_batch = true; }
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty() == o.from.empty()) die(std::string("one of --run and --from-tables is required\n") + USAGE);
  const int ways = (int)!o.pairs.empty() + (int)!o.against.empty() + (int)o.all_pairs;
  if (!o.from.empty()) {
    if (!o.samples.empty() || ways || !o.hist.empty() || o.has_cap || o.has_jcap || o.has_gpus || o.has_batch)
      die(std::string("--from-tables takes --joint, --kmer-size, --solid and --output alone\n") + USAGE);
    if (o.joint.empty() && (o.has_k || o.has_solid)) die("--kmer-size and --solid need the --joint table");
  } else {
    if (o.has_k) die("--kmer-size goes with --from-tables: a run names its own");
    if (ways > 1) die("--pairs, --against and --all-pairs exclude each other");
    if (!ways && (!o.joint.empty() || o.has_jcap || o.has_solid)) die("--joint, --joint-cap and --solid need pairs: one of --pairs, --against and --all-pairs");
    if (ways && o.solid > o.joint_cap) die("--solid must be in [1, --joint-cap]");
  }
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
}

typedef std::vector<std::pair<std::string, std::string>> IdPairs;

// the text of --hist: M, C1 and the ids in comment lines, then a line a bin (0 ... C1, then the volume of the last) with a column a sample
std::string hist_text(const std::vector<std::string>& ids, uint32_t C1, const std::vector<uint64_t>& hist)
{
  const size_t M = ids.size(), W = (size_t)C1 + 2;
  std::string t = "# kmx spectra hist\n# samples: " + std::to_string(M) + "\n# cap: " + std::to_string(C1) + "\n";
  for (const std::string& s : ids) t += "# id: " + s + "\n";
  t += "bin";
  for (size_t j = 0; j < M; j++) t += "\t" + std::to_string(j);
  t += "\n";
  for (size_t b = 0; b < W; b++) {
    t += b <= C1 ? std::to_string(b) : std::string("volume");
    for (size_t j = 0; j < M; j++) { t += '\t'; t += std::to_string(hist[j * W + b]); }
    t += '\n';
  }
  return t;
}

// the text of --joint: P, C2 and the pairs in comment lines, then the non-zero cells in the order of (pair, a, b)
std::string joint_text(const IdPairs& pairs, uint32_t C2, const std::vector<uint64_t>& joint)
{
  const size_t W = (size_t)C2 + 1;
  std::string t = "# kmx spectra joint\n# pairs: " + std::to_string(pairs.size()) + "\n# cap: " + std::to_string(C2) + "\n";
  for (const auto& p : pairs) t += "# pair: " + p.first + "\t" + p.second + "\n";
  t += "pair\ta\tb\trows\n";
  for (size_t p = 0; p < pairs.size(); p++)
    for (size_t a = 0; a < W; a++)
      for (size_t b = 0; b < W; b++) {
        const uint64_t n = joint[(p * W + a) * W + b];
        if (n) t += std::to_string(p) + "\t" + std::to_string(a) + "\t" + std::to_string(b) + "\t" + std::to_string(n) + "\n";
      }
  return t;
}

// ... read back: anything but the texts above is refused
struct TableReader {
  std::string path, kind;      // kind: "--hist" / "--joint", for the refusal
  uint64_t ln = 0;
  [[noreturn]] void bad(const std::string& why) const { die(path + (ln ? " line " + std::to_string(ln) : std::string()) + ": " + why + " (not a file written by kmx spectra " + kind + ")"); }
  uint64_t number(const std::string& v) const
  {
    if (v.empty() || v.size() > 20 || v.find_first_not_of("0123456789") != std::string::npos) bad("expected a number, found '" + v + "'");
    try { return std::stoull(v); } catch (...) { bad("a number that does not fit 64 bits"); }
  }
  static std::vector<std::string> cells(const std::string& line)
  {
    std::vector<std::string> c; std::istringstream is(line); std::string x;
    while (std::getline(is, x, '\t')) c.push_back(x);
    if (!line.empty() && line.back() == '\t') c.push_back("");
    return c;
  }
  uint64_t add(uint64_t a, uint64_t b) const { if (a + b < a) bad("the rows do not fit 64 bits"); return a + b; }
};

// -> the rows every column of the table counts
uint64_t read_hist(const std::string& path, std::vector<std::string>* ids, uint32_t* C1, std::vector<uint64_t>* hist)
{
  std::ifstream f(path);
  if (!f) die("Unable to read at " + path);
  TableReader rd{path, "--hist"};
  std::string line;
  uint64_t M = 0, cap = 0, next = 0, W = 0;
  bool has_m = false, has_c = false, in_table = false;
  while (std::getline(f, line)) {
    rd.ln++;
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    if (rd.ln == 1 && line != "# kmx spectra hist") rd.bad("expected the line '# kmx spectra hist'");
    if (line[0] == '#') {
      if (in_table) rd.bad("a comment inside the table");
      if (line.rfind("# samples: ", 0) == 0) { M = rd.number(line.substr(11)); has_m = true; if (M == 0 || M > 0xFFFFFFFFull) rd.bad("a sample count outside [1, 2^32 - 1]"); }
      else if (line.rfind("# cap: ", 0) == 0) { cap = rd.number(line.substr(7)); has_c = true; if (cap < 1 || cap > 65535) rd.bad("a cap outside [1, 65535]"); }
      else if (line.rfind("# id: ", 0) == 0) ids->push_back(line.substr(6));
      continue;
    }
    const std::vector<std::string> c = TableReader::cells(line);
    if (!in_table) {
      if (!has_m || !has_c) rd.bad("the table starts before the samples and cap lines");
      if (ids->size() != M) rd.bad(std::to_string(ids->size()) + " id lines for " + std::to_string(M) + " samples");
      if (M * (cap + 2) >= (1ull << 30)) rd.bad("a table of 8 GiB and more");
      if (c.size() != M + 1 || c[0] != "bin") rd.bad("expected the column line bin, 0 ... M - 1");
      for (uint64_t j = 0; j < M; j++) if (c[j + 1] != std::to_string(j)) rd.bad("expected the column line bin, 0 ... M - 1");
      in_table = true; W = cap + 2;
      hist->assign(M * W, 0);
      continue;
    }
    if (next >= W) rd.bad("more than cap + 2 lines");
    if (c.size() != M + 1) rd.bad("expected " + std::to_string(M + 1) + " columns");
    if (c[0] != (next <= cap ? std::to_string(next) : std::string("volume"))) rd.bad(next <= cap ? "expected bin " + std::to_string(next) : std::string("expected the volume line"));
    for (uint64_t j = 0; j < M; j++) (*hist)[j * W + next] = rd.number(c[j + 1]);
    next++;
  }
  rd.ln = 0;
  if (!in_table || next != W) rd.bad("the table ends before the volume line");
  // what every table obeys: the columns count the same rows; a count of the last bin is cap at the least, and none means no volume
  uint64_t rows = 0;
  for (uint64_t j = 0; j < M; j++) {
    uint64_t s = 0;
    for (uint64_t b = 0; b <= cap; b++) s = rd.add(s, (*hist)[j * W + b]);
    if (j && s != rows) rd.bad("the columns do not count the same rows");
    rows = s;
    const uint64_t last = (*hist)[j * W + cap], vol = (*hist)[j * W + cap + 1];
    if ((last == 0) != (vol == 0) || vol / cap < last) rd.bad("the volume of a last bin is below what its rows hold");
    unsigned __int128 v = vol;
    for (uint64_t b = 1; b < cap; b++) v += (unsigned __int128)b * (*hist)[j * W + b];
    if (v >> 64) rd.bad("a volume that does not fit 64 bits");
  }
  *C1 = (uint32_t)cap;
  return rows;
}

void read_joint(const std::string& path, uint64_t rows, IdPairs* pairs, uint32_t* C2, std::vector<uint64_t>* joint)
{
  std::ifstream f(path);
  if (!f) die("Unable to read at " + path);
  TableReader rd{path, "--joint"};
  std::string line;
  uint64_t P = 0, cap = 0, W = 0, last_at = 0;
  bool has_p = false, has_c = false, in_table = false, any = false;
  while (std::getline(f, line)) {
    rd.ln++;
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    if (rd.ln == 1 && line != "# kmx spectra joint") rd.bad("expected the line '# kmx spectra joint'");
    if (line[0] == '#') {
      if (in_table) rd.bad("a comment inside the table");
      if (line.rfind("# pairs: ", 0) == 0) { P = rd.number(line.substr(9)); has_p = true; if (P == 0 || P > 0xFFFFFFFFull) rd.bad("a pair count outside [1, 2^32 - 1]"); }
      else if (line.rfind("# cap: ", 0) == 0) { cap = rd.number(line.substr(7)); has_c = true; if (cap < 1 || cap > 255) rd.bad("a cap outside [1, 255]"); }
      else if (line.rfind("# pair: ", 0) == 0) {
        const std::vector<std::string> c = TableReader::cells(line.substr(8));
        if (c.size() != 2 || c[0].empty() || c[1].empty()) rd.bad("expected two sample ids");
        pairs->push_back({c[0], c[1]});
      }
      continue;
    }
    if (!in_table) {
      if (!has_p || !has_c) rd.bad("the table starts before the pairs and cap lines");
      if (pairs->size() != P) rd.bad(std::to_string(pairs->size()) + " pair lines for " + std::to_string(P) + " pairs");
      if (line != "pair\ta\tb\trows") rd.bad("expected the column line pair, a, b, rows");
      W = cap + 1;
      if (P * W * W >= (1ull << 30)) rd.bad("a table of 8 GiB and more");
      in_table = true;
      joint->assign(P * W * W, 0);
      continue;
    }
    const std::vector<std::string> c = TableReader::cells(line);
    if (c.size() != 4) rd.bad("expected four columns");
    const uint64_t p = rd.number(c[0]), a = rd.number(c[1]), b = rd.number(c[2]), n = rd.number(c[3]);
    if (p >= P || a > cap || b > cap) rd.bad("a cell outside the table");
    if (n == 0) rd.bad("a cell of no rows");
    const uint64_t at = (p * W + a) * W + b;
    if (any && at <= last_at) rd.bad("the cells are not in the order of (pair, a, b)");
    any = true; last_at = at;
    (*joint)[at] = n;
  }
  rd.ln = 0;
  if (!in_table) rd.bad("no table");
  for (uint64_t p = 0; p < P; p++) {
    uint64_t s = 0;
    for (uint64_t i = 0; i < W * W; i++) s = rd.add(s, (*joint)[p * W * W + i]);
    if (s != rows) rd.bad("pair " + std::to_string(p) + " does not count the rows the --hist table counts");
  }
  *C2 = (uint32_t)cap;
}

// the report: k = 0 where no k-mer size is known (a hash run; --from-tables without --kmer-size)
std::string report_text(const std::vector<std::string>& ids, uint32_t C1, const std::vector<uint64_t>& hist, const IdPairs& pairs, uint32_t C2, const std::vector<uint64_t>& joint,
                        uint32_t solid, uint32_t k)
{
  const size_t M = ids.size(), P = pairs.size();
  std::string t = "# kmx spectra\n# samples: " + std::to_string(M) + "\n# cap: " + std::to_string(C1) + "\n# pairs: " + std::to_string(P) + "\n";
  t += "# joint_cap: " + (P ? std::to_string(C2) : std::string("NA")) + "\n# solid: " + (P ? std::to_string(solid) : std::string("NA")) + "\n";
  t += "# kmer_size: " + (P && k ? std::to_string(k) : std::string("NA")) + "\n";
  t += "sample\trows\tsingletons\tvolume\ttail_volume\tvalley\tpeak\n";
  for (size_t j = 0; j < M; j++) {
    const kmxspectra::SampleStats s = kmxspectra::sample_stats(&hist[j * ((size_t)C1 + 2)], C1);
    t += ids[j] + "\t" + std::to_string(s.rows) + "\t" + std::to_string(s.singletons) + "\t" + std::to_string(s.volume) + "\t" + std::to_string(s.tail_volume) + "\t" +
         std::to_string(s.valley) + "\t" + std::to_string(s.peak) + "\n";
  }
  if (!P) return t;
  t += "x\ty\tboth\tx_only\ty_only\tjaccard\tcompleteness\tqv\n";
  const size_t cells = ((size_t)C2 + 1) * ((size_t)C2 + 1);
  for (size_t p = 0; p < P; p++) {
    const kmxspectra::PairStats s = kmxspectra::pair_stats(&joint[p * cells], C2, solid);
    t += pairs[p].first + "\t" + pairs[p].second + "\t" + std::to_string(s.both) + "\t" + std::to_string(s.x_only) + "\t" + std::to_string(s.y_only) + "\t" +
         kmxspectra::ratio(s.both, s.both + s.x_only + s.y_only) + "\t" + kmxspectra::ratio(s.solid_held, s.solid_all) + "\t" + (k ? kmxspectra::qv(s, k) : std::string("NA")) + "\n";
  }
  return t;
}

// id -> column of the fof; an id may come any number of times
uint32_t column_of(const std::map<std::string, uint32_t>& at, const std::string& id, const std::string& where)
{
  const auto it = at.find(id);
  if (it == at.end()) die(where + "sample " + id + " is not in the run's kmtricks.fof");
  return it->second;
}

}  // namespace

int kmx_spectra_main(int argc, char** argv)
{
  const SOpt o = parse(argc, argv);
  if (!o.from.empty()) {
    std::vector<std::string> ids; uint32_t C1 = 0, C2 = 0; std::vector<uint64_t> hist, joint; IdPairs pairs;
    const uint64_t rows = read_hist(o.from, &ids, &C1, &hist);
    if (!o.joint.empty()) {
      read_joint(o.joint, rows, &pairs, &C2, &joint);
      if (o.solid > C2) die("--solid must be in [1, the cap of the --joint table]");
    }
    write_text(o.out, report_text(ids, C1, hist, pairs, C2, joint, o.solid, o.k));
    return 0;
  }
  // ---- the run directory; every check before kmx_create ----
  RunDir dir;
  dir.at("spectra", o.run);
  dir.read_mode(MATRIX_KINDS, MATRIX_MODES);
  dir.shape();
  const uint32_t N = dir.N;
  std::vector<uint32_t> cols;
  if (!o.samples.empty()) cols = read_sample_list(o.samples, dir.samples);
  const uint32_t M = o.samples.empty() ? N : (uint32_t)cols.size();
  std::vector<std::string> ids(M);
  for (uint32_t j = 0; j < M; j++) ids[j] = dir.samples[cols.empty() ? j : cols[j]].id;
  if ((uint64_t)M * ((uint64_t)o.cap + 2) >= (1ull << 30)) die("--cap: a table of M x (cap + 2) entries would be 8 GiB and more");
  // the pairs, as input columns
  std::vector<uint32_t> pairs; IdPairs id_pairs;
  auto col_at = [&](uint32_t j) { return cols.empty() ? j : cols[j]; };
  auto put = [&](uint32_t x, uint32_t y) { pairs.push_back(x); pairs.push_back(y); id_pairs.push_back({dir.samples[x].id, dir.samples[y].id}); };
  std::map<std::string, uint32_t> at;
  for (uint32_t i = 0; i < N; i++) at[dir.samples[i].id] = i;
  const uint64_t cells = ((uint64_t)o.joint_cap + 1) * (o.joint_cap + 1);
  if (o.all_pairs) {
    if ((uint64_t)M * (M - 1) / 2 * cells >= (1ull << 30)) die("--all-pairs: the tables of " + std::to_string((uint64_t)M * (M - 1) / 2) + " pairs would be 8 GiB and more (fewer samples, or a smaller --joint-cap)");
    for (uint32_t i = 0; i < M; i++) for (uint32_t j = i + 1; j < M; j++) put(col_at(i), col_at(j));
    if (pairs.empty()) die("--all-pairs needs two listed samples");
  } else if (!o.against.empty()) {
    const uint32_t x = column_of(at, o.against, "--against: ");
    for (uint32_t j = 0; j < M; j++) if (col_at(j) != x) put(x, col_at(j));
    if (pairs.empty()) die("--against " + o.against + ": no other sample is listed");
  } else if (!o.pairs.empty()) {
    std::ifstream f(o.pairs);
    if (!f) die("Unable to read at " + o.pairs);
    std::string line;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
      std::istringstream is(line);
      std::string x, y, more;
      if (!(is >> x)) continue;      // an empty line
      const std::string where = o.pairs + " line " + std::to_string(ln) + ": ";
      if (!(is >> y) || (is >> more)) die(where + "expected two sample ids");
      put(column_of(at, x, where), column_of(at, y, where));
    }
    if (pairs.empty()) die(o.pairs + " names no pair");
  }
  const uint32_t P = (uint32_t)id_pairs.size();
  if ((uint64_t)id_pairs.size() * cells >= (1ull << 30)) die("the tables of " + std::to_string(id_pairs.size()) + " pairs would be 8 GiB and more (fewer pairs, or a smaller --joint-cap)");
  dir.open_files();

  // ---- devices; how many rows a run holds ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 4);
  const uint64_t rows_a_run = run_rows(dev.budget, dir.stride);
  if (o.verbose) fprintf(stderr, "[kmx spectra] %u of %u samples, %u pairs, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", M, N, P,
                         (unsigned long long)dir.P, dir.mode.c_str(), (unsigned long long)dir.stride, (unsigned long long)rows_a_run, dev.G());

  // every partition's rows, a shard's into the tables of its first call; the devices' tables summed
  std::vector<uint64_t> hist((uint64_t)M * ((uint64_t)o.cap + 2), 0), joint(P * cells, 0);
  std::mutex mu;
  in_shards(dev.G(), [&](uint32_t g) {
    kmx_ctx* ctx = dev.ctxs[g];
    kmx_spectra_result* first = accumulate_runs<kmx_spectra_result>(dir, ctx, g, dev.G(), rows_a_run, [&](const uint8_t* rows, uint64_t n, kmx_spectra_result* first) {
      kmx_spectra_task t; memset(&t, 0, sizeof t);
      t.key_words = dir.kw; t.mode = dir.rmode(); t.n_cols = N; t.n_use = M;
      t.cols = cols.empty() ? nullptr : cols.data(); t.cap1 = o.cap; t.flags = KMX_SPECTRA_HIST;
      if (P) { t.pairs = pairs.data(); t.n_pairs = P; t.cap2 = o.joint_cap; t.flags |= KMX_SPECTRA_JOINT; }
      t.n_rows = n; t.rows = rows;
      t.hist = first ? kmx_spectra_result_hist_dev(first) : nullptr;
      t.joint = first && P ? kmx_spectra_result_joint_dev(first) : nullptr;
      kmx_spectra_result* r = nullptr;
      chk(ctx, kmx_spectra_host(ctx, &t, &r), "kmx_spectra_host");
      return r;
    }, kmx_spectra_result_wait, kmx_spectra_result_free, "kmx_spectra");
    if (!first) return;      // (more shards than partitions)
    std::vector<uint64_t> h(hist.size()), j(joint.size());
    chk(ctx, kmx_spectra_result_copy_hist(first, h.data(), h.size()), "kmx_spectra_result_copy_hist");
    if (P) chk(ctx, kmx_spectra_result_copy_joint(first, j.data(), j.size()), "kmx_spectra_result_copy_joint");
    kmx_spectra_result_free(first);
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < h.size(); i++) hist[i] += h[i];
    for (size_t i = 0; i < j.size(); i++) joint[i] += j[i];
  });
  dev.close();

  if (!o.hist.empty()) write_text(o.hist, hist_text(ids, o.cap, hist));
  if (!o.joint.empty()) write_text(o.joint, joint_text(id_pairs, o.joint_cap, joint));
  write_text(o.out, report_text(ids, o.cap, hist, id_pairs, o.joint_cap, joint, o.solid, dir.kd.kmer ? dir.k : 0));
  return 0;
}
