// kmx_pan.cpp -- `kmx pan`: the recurrence spectrum of a run and the pangenome growth and core curves that follow from it (what
// pangrowth and Panacus `hist` / `histgrowth` / `ordered-histgrowth` compute; no counterpart in the kmtricks tree; include/kmx.h, section
// "pan").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run or the
// .count_hash / .pa_hash matrices of a hash run.  Every partition goes through kmx_pan_host in runs of rows that fit the device, two in
// flight; all of them add into one pair of tables per device, the devices' tables are summed on the host, and the curves are worked out
// there in closed form (kmx_pan_curves.hpp).  `kmx pan --from-spectrum FILE` prints the curves of a spectrum saved with --spectrum and
// asks for no device.  Every check that needs no GPU comes before kmx_create.
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
#include "kmx_pan_curves.hpp"

namespace fs = std::filesystem;
using namespace kmxio;

namespace {

struct POpt {
  std::string run, out, samples, shared, spectrum, from;
  uint32_t gpus = 1, min_abund = 1;
  bool has_gpus = false, has_abund = false, has_batch = false;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
  bool verbose = false;
};

const char* USAGE = "usage: kmx pan --run <run dir made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin> [--samples FILE] "
                    "[--min-abund INT] [--shared FILE] [--spectrum FILE] [--output FILE] [--gpus INT] [--batch-mb INT] [-v]\n"
                    "       kmx pan --from-spectrum FILE [--output FILE]\n"
                    "  FILE of --samples: one sample id per line, the samples in the order they are added (default: every sample of the run, in the "
                    "order of its kmtricks.fof).\n"
                    "  Prints, for m = 1 ... M samples: the sample added at m, pan_mean, core_mean and new_mean (the rows met after m samples, held by "
                    "all m, and brought by the m-th, averaged over every order of adding the samples), pan_order and core_order (the same in the "
                    "order given); a sample holds a row from a count of --min-abund.  --spectrum writes the rows by recurrence, by first and by "
                    "first missing sample (--from-spectrum reads it back); --shared writes, per recurrence, how many rows each sample holds.";

POpt parse(int argc, char** argv)
{
  POpt o;
  auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + USAGE); return argv[++i]; };
  auto num = [&](int& i) -> unsigned long { const std::string v = need(i); try { size_t n = 0; if (v.empty() || v[0] == '-') throw 1; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  auto u32 = [&](int& i) -> uint32_t { const unsigned long x = num(i); if (x > 0xFFFFFFFFul) die(std::string(argv[i - 1]) + " does not fit 32 bits"); return (uint32_t)x; };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = need(i);
    else if (a == "--from-spectrum") o.from = need(i);
    else if (a == "--output") o.out = need(i);
    else if (a == "--samples") o.samples = need(i);
    else if (a == "--shared") o.shared = need(i);
    else if (a == "--spectrum") o.spectrum = need(i);
    else if (a == "--min-abund") { o.min_abund = u32(i); o.has_abund = true; if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--gpus") { o.gpus = u32(i); o.has_gpus = true; }
    else if (a == "--batch-mb") { o.batch_mb = num(i); o.has_batch = true; }
    else if (a == "-v" || a == "--verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') i++; }
    else die("unknown option " + a + "\n" + USAGE);
  }
  if (o.run.empty() == o.from.empty()) die(std::string("one of --run and --from-spectrum is required\n") + USAGE);
  if (!o.from.empty() && (!o.samples.empty() || !o.shared.empty() || !o.spectrum.empty() || o.has_abund || o.has_gpus || o.has_batch))
    die(std::string("--from-spectrum takes --output alone\n") + USAGE);
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

// the text of --spectrum: M, a and the ids in comment lines, then r, rows, first and gap for r = 0 ... M
std::string spectrum_text(const std::vector<std::string>& ids, uint32_t a, const std::vector<uint64_t>& spec)
{
  const size_t M = ids.size();
  std::string t = "# kmx pan spectrum\n# samples: " + std::to_string(M) + "\n# min_abund: " + std::to_string(a) + "\n";
  for (const std::string& s : ids) t += "# id: " + s + "\n";
  t += "r\trows\tfirst\tgap\n";
  for (size_t r = 0; r <= M; r++)
    t += std::to_string(r) + "\t" + std::to_string(spec[r]) + "\t" + std::to_string(spec[M + 1 + r]) + "\t" + std::to_string(spec[2 * (M + 1) + r]) + "\n";
  return t;
}

// ... read back: anything but the text above is refused
void read_spectrum(const std::string& path, std::vector<std::string>* ids, uint32_t* a, std::vector<uint64_t>* spec)
{
  std::ifstream f(path);
  if (!f) die("Unable to read at " + path);
  auto bad = [&](uint64_t ln, const std::string& why) { die(path + " line " + std::to_string(ln) + ": " + why + " (not a file written by kmx pan --spectrum)"); };
  auto number = [&](const std::string& v, uint64_t ln) -> uint64_t {
    if (v.empty() || v.size() > 20 || v.find_first_not_of("0123456789") != std::string::npos) bad(ln, "expected a number, found '" + v + "'");
    try { return std::stoull(v); } catch (...) { bad(ln, "a number that does not fit 64 bits"); }
    return 0;
  };
  std::string line;
  uint64_t ln = 0, M = 0;
  bool has_m = false, has_a = false, in_table = false;
  uint64_t next = 0;
  while (std::getline(f, line)) {
    ln++;
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
    if (line.empty()) continue;
    if (line[0] == '#') {
      if (in_table) bad(ln, "a comment inside the table");
      if (line.rfind("# samples: ", 0) == 0) { M = number(line.substr(11), ln); has_m = true; if (M == 0 || M > 0xFFFFFFFEull) bad(ln, "a sample count outside [1, 2^32 - 2]"); }
      else if (line.rfind("# min_abund: ", 0) == 0) { const uint64_t v = number(line.substr(13), ln); if (v == 0 || v > 0xFFFFFFFFull) bad(ln, "a min_abund outside [1, 2^32 - 1]"); *a = (uint32_t)v; has_a = true; }
      else if (line.rfind("# id: ", 0) == 0) ids->push_back(line.substr(6));
      continue;
    }
    if (!in_table) {
      if (line != "r\trows\tfirst\tgap") bad(ln, "expected the column line r, rows, first, gap");
      if (!has_m || !has_a) bad(ln, "the table starts before the samples and min_abund lines");
      if (ids->size() != M) bad(ln, std::to_string(ids->size()) + " id lines for " + std::to_string(M) + " samples");
      in_table = true;
      spec->assign(3 * (M + 1), 0);
      continue;
    }
    std::vector<std::string> cell;
    { std::istringstream is(line); std::string c; while (std::getline(is, c, '\t')) cell.push_back(c); }
    if (cell.size() != 4) bad(ln, "expected four columns");
    if (next > M) bad(ln, "more than M + 1 rows");
    if (number(cell[0], ln) != next) bad(ln, "expected r = " + std::to_string(next));
    for (int t = 0; t < 3; t++) (*spec)[t * (M + 1) + next] = number(cell[1 + t], ln);
    next++;
  }
  if (!in_table || next != M + 1) die(path + ": the table ends before r = M (not a file written by kmx pan --spectrum)");
  // what every spectrum obeys: the three tables count the same rows; no holder means no first, no gap means every holder
  uint64_t s[3] = {0, 0, 0};
  for (int t = 0; t < 3; t++) for (uint64_t r = 0; r <= M; r++) { const uint64_t v = (*spec)[t * (M + 1) + r]; if (s[t] + v < s[t]) die(path + ": the rows do not fit 64 bits"); s[t] += v; }
  if (s[0] != s[1] || s[0] != s[2] || (*spec)[M + 1 + M] != (*spec)[0] || (*spec)[2 * (M + 1) + M] != (*spec)[M])
    die(path + ": the three columns do not count the same rows (not a file written by kmx pan --spectrum)");
}

// the curves' text
std::string curves_text(const std::vector<std::string>& ids, uint32_t a, const std::vector<uint64_t>& spec)
{
  const uint32_t M = (uint32_t)ids.size();
  const kmxpan::Curves c = kmxpan::curves(M, &spec[0], &spec[(size_t)M + 1], &spec[2 * ((size_t)M + 1)]);
  uint64_t rows = 0;
  for (uint32_t r = 0; r <= M; r++) rows += spec[r];
  char num[128];
  std::string t = "# kmx pan\n# samples: " + std::to_string(M) + "\n# rows: " + std::to_string(rows) + "\n# min_abund: " + std::to_string(a) + "\n";
  if (c.has_alpha) { snprintf(num, sizeof num, "%.6f", std::fabs(c.heaps_alpha) < 5e-7 ? 0.0 : c.heaps_alpha); t += std::string("# heaps_alpha: ") + num + "\n"; }      // (no "-0.000000")
  else t += "# heaps_alpha: NA\n";
  t += "m\tsample\tpan_mean\tcore_mean\tnew_mean\tpan_order\tcore_order\n";
  for (uint32_t m = 1; m <= M; m++) {
    snprintf(num, sizeof num, "\t%.6f\t%.6f\t%.6f\t", c.pan_mean[m], c.core_mean[m], c.new_mean[m]);
    t += std::to_string(m) + "\t" + ids[m - 1] + num + std::to_string(c.pan_order[m]) + "\t" + std::to_string(c.core_order[m]) + "\n";
  }
  return t;
}

}  // namespace

int kmx_pan_main(int argc, char** argv)
{
  const POpt o = parse(argc, argv);
  if (!o.from.empty()) {
    std::vector<std::string> ids; uint32_t a = 1; std::vector<uint64_t> spec;
    read_spectrum(o.from, &ids, &a, &spec);
    write_text(o.out, curves_text(ids, a, spec));
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
  else die("kmx pan needs a run made with --mode kmer:count:bin, kmer:pa:bin, hash:count:bin or hash:pa:bin; " + run + " was made with " + mode);
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
  // the sample list: one id a line, in the order the samples are added
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
  const bool want_shared = !o.shared.empty();
  if (want_shared && ((uint64_t)M + 1) * N >= (1ull << 30)) die("--shared: a table of (M + 1) x N entries would be 8 GiB and more");
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
    if (!kd.kmer && !kd.pa && rd<uint32_t>(&h[21]) != 4) die(files[p] + " has counts of " + std::to_string(rd<uint32_t>(&h[21])) + " bytes: kmx pan reads 4-byte counts");
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
  // two runs are on the device at a time (one travels while the other is worked on); a row costs its bytes and, with --shared, 12 more
  const uint64_t per_row = stride + (want_shared ? 12 : 0);
  const uint64_t run_rows = std::min<uint64_t>(std::max<uint64_t>(budget / 2 / per_row, 1), 0xFFFFFF00ull);
  if (o.verbose) fprintf(stderr, "[kmx pan] %u of %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", M, N, (unsigned long long)P,
                         mode.c_str(), (unsigned long long)stride, (unsigned long long)run_rows, G);

  const uint64_t M1 = (uint64_t)M + 1;
  std::vector<uint64_t> spec(3 * M1, 0), shared(want_shared ? M1 * N : 0, 0);
  std::mutex mu;
  // shard g: the partitions p with p mod G == g, one after the other, all into the tables of the shard's first call
  auto shard = [&](uint32_t g) {
    try {
      kmx_ctx* ctx = ctxs[g];
      kmx_pan_result* first = nullptr;
      struct Flight { kmx_pan_result* r; std::shared_ptr<std::vector<uint8_t>> body; };
      std::deque<Flight> flying;
      auto land = [&](size_t keep) {
        while (flying.size() > keep) {
          Flight f = flying.front(); flying.pop_front();
          chk(ctx, kmx_pan_result_wait(f.r), "kmx_pan");
          if (f.r != first) kmx_pan_result_free(f.r);
        }
      };
      for (uint64_t p = g; p < P; p += G) {
        std::vector<uint8_t> raw = slurp(files[p]);
        auto body = std::make_shared<std::vector<uint8_t>>(body_of(raw, kd.hdr, kd.magic, files[p]));
        raw = std::vector<uint8_t>();
        if (body->size() % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
        const uint64_t rows = body->size() / stride;
        for (uint64_t r0 = 0; r0 < rows || (r0 == 0 && !first); r0 += run_rows) {      // (a shard's first call is made even for no rows: it owns the tables)
          kmx_pan_task t; memset(&t, 0, sizeof t);
          t.key_words = kw; t.mode = count ? KMX_MODE_COUNT : KMX_MODE_PA; t.n_cols = N; t.n_use = M;
          t.cols = cols.empty() ? nullptr : cols.data(); t.min_abund = o.min_abund; t.flags = want_shared ? KMX_PAN_SHARED : 0;
          t.n_rows = std::min(run_rows, rows - r0);
          t.rows = t.n_rows ? body->data() + r0 * stride : nullptr;
          t.spectrum = first ? kmx_pan_result_spectrum_dev(first) : nullptr;
          t.shared = first && want_shared ? kmx_pan_result_shared_dev(first) : nullptr;
          kmx_pan_result* r = nullptr;
          chk(ctx, kmx_pan_host(ctx, &t, &r), "kmx_pan_host");
          if (!first) { first = r; chk(ctx, kmx_pan_result_wait(r), "kmx_pan"); }      // (its tables are asked for by the next call)
          flying.push_back({r, body});
          land(1);      // the run before this one has been worked on; this one travels
          if (rows == 0) break;
        }
      }
      land(0);
      if (!first) return;      // (more shards than partitions)
      std::vector<uint64_t> sp(spec.size()), sh(shared.size());
      chk(ctx, kmx_pan_result_copy_spectrum(first, sp.data(), sp.size()), "kmx_pan_result_copy_spectrum");
      if (want_shared) chk(ctx, kmx_pan_result_copy_shared(first, sh.data(), sh.size()), "kmx_pan_result_copy_shared");
      kmx_pan_result_free(first);
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < sp.size(); i++) spec[i] += sp[i];
      for (size_t i = 0; i < sh.size(); i++) shared[i] += sh[i];
    } catch (const std::exception& e) { die(e.what()); }
  };
  std::vector<std::thread> workers;
  for (uint32_t g = 1; g < G; g++) workers.emplace_back(shard, g);
  shard(0);
  for (std::thread& w : workers) w.join();
  for (uint32_t g = 0; g < G; g++) kmx_destroy(ctxs[g]);

  if (!o.spectrum.empty()) write_text(o.spectrum, spectrum_text(ids, o.min_abund, spec));
  if (want_shared) {      // the (M + 1) x M table in list order: column j is input column cols[j]
    std::string t = "r";
    for (const std::string& s : ids) { t += '\t'; t += s; }
    t += '\n';
    for (uint64_t r = 0; r <= M; r++) {
      t += std::to_string(r);
      for (uint32_t j = 0; j < M; j++) { t += '\t'; t += std::to_string(shared[r * N + (cols.empty() ? j : cols[j])]); }
      t += '\n';
    }
    write_text(o.shared, t);
  }
  write_text(o.out, curves_text(ids, o.min_abund, spec));
  return 0;
}
