// kmx_pan.cpp -- `kmx pan`: the recurrence spectrum of a run and the pangenome growth and core curves that follow from it (what
// pangrowth and Panacus `hist` / `histgrowth` / `ordered-histgrowth` compute; no counterpart in the kmtricks tree; include/kmx.h, section
// "pan").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run or the
// .count_hash / .pa_hash matrices of a hash run.  Every partition goes through kmx_pan_host in runs of rows that fit the device, two in
// flight; all of them add into one pair of tables per device, the devices' tables are summed on the host, and the curves are worked out
// there in closed form (kmx_pan_curves.hpp).  `kmx pan --from-spectrum FILE` prints the curves of a spectrum saved with --spectrum and
// asks for no device.  Every check that needs no GPU comes before kmx_create.
#include <sstream>
#include "kmx_driver.hpp"
#include "kmx_pan_curves.hpp"

using namespace kmxdrv;

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
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--from-spectrum") o.from = in.need(i);
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--samples") o.samples = in.need(i);
    else if (a == "--shared") o.shared = in.need(i);
    else if (a == "--spectrum") o.spectrum = in.need(i);
    else if (a == "--min-abund") { o.min_abund = in.u32(i); o.has_abund = true; if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--gpus") { o.gpus = in.u32(i); o.has_gpus = true; }
    else if (a == "--batch-mb") { o.batch_mb = in.num(i); o.has_batch = true; }
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty() == o.from.empty()) die(std::string("one of --run and --from-spectrum is required\n") + USAGE);
  if (!o.from.empty() && (!o.samples.empty() || !o.shared.empty() || !o.spectrum.empty() || o.has_abund || o.has_gpus || o.has_batch))
    die(std::string("--from-spectrum takes --output alone\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
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
  // ---- the run directory; every check before kmx_create ----
  RunDir dir;
  dir.at("pan", o.run);
  dir.read_mode(MATRIX_KINDS, MATRIX_MODES);
  if (!dir.count() && o.min_abund > 1) die("--min-abund above 1 needs counts: " + dir.run + " was made with " + dir.mode);
  dir.shape();
  const uint32_t N = dir.N;
  // the sample list: one id a line, in the order the samples are added
  std::vector<uint32_t> cols;
  if (!o.samples.empty()) cols = read_sample_list(o.samples, dir.samples);
  const uint32_t M = o.samples.empty() ? N : (uint32_t)cols.size();
  const bool want_shared = !o.shared.empty();
  if (want_shared && ((uint64_t)M + 1) * N >= (1ull << 30)) die("--shared: a table of (M + 1) x N entries would be 8 GiB and more");
  std::vector<std::string> ids(M);
  for (uint32_t j = 0; j < M; j++) ids[j] = dir.samples[cols.empty() ? j : cols[j]].id;
  dir.open_files();

  // ---- devices; how many rows a run holds ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 4);
  // a row costs its bytes and, with --shared, 12 more
  const uint64_t per_row = dir.stride + (want_shared ? 12 : 0);
  const uint64_t rows_a_run = run_rows(dev.budget, per_row);
  if (o.verbose) fprintf(stderr, "[kmx pan] %u of %u samples, %llu partitions (%s), rows of %llu bytes, runs of %llu rows, %u shards\n", M, N, (unsigned long long)dir.P,
                         dir.mode.c_str(), (unsigned long long)dir.stride, (unsigned long long)rows_a_run, dev.G());

  // every partition's rows, a shard's into the tables of its first call; the devices' tables summed
  std::vector<uint64_t> spec, shared;
  pan_pass(dir, dev, rows_a_run, cols.empty() ? nullptr : cols.data(), M, o.min_abund, &spec, want_shared ? &shared : nullptr);
  dev.close();

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
