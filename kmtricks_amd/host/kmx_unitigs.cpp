// kmx_unitigs.cpp -- `kmx unitigs`: a run's k-mers (all of them, or those a `kmx diff` / `kmx assoc` output lists) compacted into unitigs
// and, per unitig and sample, the abundance of its k-mers (what MUSET does behind `kmat_tools filter` with ggcat and `kmat_tools unitig`,
// what kmdiff does when it merges its significant k-mers; no counterpart in the kmtricks tree; include/kmx.h, sections "unitigs" and
// "groupsum").  The input is the run directory as `kmx pipeline` / kmtricks leave it: the .count / .pa matrices of a kmer run.  The nodes
// are the run's rows in (partition ascending, file order); their keys are copied out of the bodies as they are read.  The graph is built
// by one kmx_unitigs_host call on one device; the table comes from kmx_groupsum_host over every partition, the device tables
// accumulating, in windows of unitigs that fit --batch-mb.  Every check that needs no GPU comes before kmx_create.
#include "kmx_driver.hpp"

using namespace kmxdrv;

namespace {

struct UOpt {
  std::string run, kmers, out, table, value, samples;
  uint32_t gpus = 1, min_abund = 1;
  uint64_t batch_mb = 0;      // 0: 256
  bool verbose = false;
};

const char* USAGE = "usage: kmx unitigs --run <run dir made with --mode kmer:count:bin or kmer:pa:bin, plain or --cpr> [--kmers FILE] [--output FILE] "
                    "[--table FILE [--value mean|frac|sum|present]] [--samples FILE] [--min-abund INT] [--batch-mb INT] [--gpus INT] [-v]\n"
                    "  Compacts the run's k-mers into unitigs.  --kmers keeps only the rows whose k-mer stands in the first tab-separated field of a "
                    "line of FILE (what kmx diff and kmx assoc --output write; # lines and their header line `kmer ...` are skipped, either strand is accepted).\n"
                    "  --output: FASTA in unitig id order, >{id} LN:i:{bases} KM:i:{kmers}, a cycle's header ends in CL:Z:circular.\n"
                    "  --table: one line per unitig -- unitig, kmers, then per sample (--samples: one id per line; default every sample) the sum of "
                    "its k-mers' counts (sum), the k-mers the sample holds from --min-abund (present), or these divided by kmers (mean, frac; %.2f).  "
                    "A count run's default is mean, a presence/absence run's frac.  The table is made in windows of unitigs whose device tables fit "
                    "--batch-mb (default 256); every window after the first reads the partitions again.  --gpus shards the table pass by partition.";

UOpt parse(int argc, char** argv)
{
  UOpt o;
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--run") o.run = in.need(i);
    else if (a == "--kmers") o.kmers = in.need(i);
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--table") o.table = in.need(i);
    else if (a == "--value") o.value = in.need(i);
    else if (a == "--samples") o.samples = in.need(i);
    else if (a == "--min-abund") { o.min_abund = in.u32(i); if (o.min_abund == 0) die("--min-abund must be at least 1"); }
    else if (a == "--gpus") o.gpus = in.u32(i);
    else if (a == "--batch-mb") o.batch_mb = in.num(i);
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.run.empty()) die(std::string("--run is required\n") + USAGE);
  if (o.out.empty() && o.table.empty()) die(std::string("one of --output and --table is required\n") + USAGE);
  if (!o.value.empty() && o.table.empty()) die("--value needs --table");
  if (!o.value.empty() && o.value != "mean" && o.value != "frac" && o.value != "sum" && o.value != "present") die("--value must be mean, frac, sum or present");
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  return o;
}

// a k-mer as the matrices' keys hold it: digit i is base k - 1 - i, A0 C1 T2 G3; kw words, low word first
typedef std::vector<uint64_t> Key;
bool key_less(const uint64_t* a, const uint64_t* b, uint32_t kw) { for (uint32_t w = kw; w-- > 0;) if (a[w] != b[w]) return a[w] < b[w]; return false; }

// the canonical key of the string s (k characters of ACGT, either case); false: a character that is none of them
bool canonical_key(const std::string& s, uint32_t kw, Key& out)
{
  const size_t k = s.size();
  Key f(kw, 0), r(kw, 0);
  for (size_t j = 0; j < k; j++) {
    uint64_t d;
    switch (s[j]) { case 'A': case 'a': d = 0; break; case 'C': case 'c': d = 1; break; case 'T': case 't': d = 2; break; case 'G': case 'g': d = 3; break; default: return false; }
    const size_t fi = k - 1 - j, ri = j;      // base j is digit k - 1 - j forward, and its complement digit j of the reverse complement
    f[fi >> 5] |= d << (2 * (fi & 31));
    r[ri >> 5] |= (d ^ 2) << (2 * (ri & 31));
  }
  out = key_less(r.data(), f.data(), kw) ? r : f;
  return true;
}

}  // namespace

int kmx_unitigs_main(int argc, char** argv)
{
  const UOpt o = parse(argc, argv);
  // ---- the run directory; every check before kmx_create ----
  RunDir dir;
  dir.at("unitigs", o.run);
  dir.read_mode(KMER_KINDS, "kmer:count:bin or kmer:pa:bin (the keys of hash and Bloom filter runs are not k-mers)");
  const std::string& run = dir.run;
  const bool count = dir.count();
  if (!count && o.min_abund > 1) die("--min-abund above 1 needs counts: " + run + " was made with " + dir.mode);
  const std::string value = !o.value.empty() ? o.value : count ? "mean" : "frac";
  if (!count && (value == "sum" || value == "mean")) die("--value " + value + " needs counts: " + run + " was made with " + dir.mode);
  dir.shape();
  const uint32_t N = dir.N, k = dir.k, kw = dir.kw;
  const uint64_t P = dir.P, stride = dir.stride;
  const std::vector<Sample>& samples = dir.samples;
  std::vector<uint32_t> cols;
  if (!o.samples.empty()) cols = read_sample_list(o.samples, samples);
  const uint32_t M = o.samples.empty() ? N : (uint32_t)cols.size();
  // the list of k-mers: canonical keys, sorted
  const bool listed = !o.kmers.empty();
  std::vector<Key> want;
  if (listed) {
    std::ifstream f(o.kmers);
    if (!f) die("Unable to read at " + o.kmers);
    std::string line;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty() || line[0] == '#') continue;
      const std::string s = line.substr(0, line.find('\t'));
      if (s == "kmer") continue;      // the header line of kmx diff / kmx assoc
      const std::string where = o.kmers + " line " + std::to_string(ln) + ": ";
      if (s.size() != k) die(where + "a k-mer of " + std::to_string(s.size()) + " characters, the run's k is " + std::to_string(k));
      Key key;
      if (!canonical_key(s, kw, key)) die(where + "malformed k-mer " + s);
      want.push_back(key);
    }
    std::sort(want.begin(), want.end(), [&](const Key& a, const Key& b) { return key_less(a.data(), b.data(), kw); });
    want.erase(std::unique(want.begin(), want.end()), want.end());
  }
  dir.open_files();

  // ---- the nodes: the kept rows' keys, and per partition which node a row is (0xFFFFFFFF: none) ----
  std::vector<uint64_t> keys;
  std::vector<std::vector<uint32_t>> node_of(P);
  std::vector<bool> found(want.size(), false);
  for (uint64_t p = 0; p < P; p++) {
    const auto loaded = dir.load(p);
    const std::vector<uint8_t>& body = *loaded;
    const uint64_t rows = body.size() / stride;
    node_of[p].assign(rows, 0xFFFFFFFFu);
    std::vector<uint64_t> rk(kw);
    auto row_key = [&](uint64_t r) { memcpy(rk.data(), &body[r * stride], 8ull * kw); return rk.data(); };
    auto take = [&](uint64_t r) {
      if (keys.size() / kw >= 0x7FFFFFFEull) die("more than 2^31 - 2 k-mers: kmx unitigs builds the graph in one call");
      node_of[p][r] = (uint32_t)(keys.size() / kw);
      const uint64_t* q = row_key(r);
      keys.insert(keys.end(), q, q + kw);
    };
    if (!listed) for (uint64_t r = 0; r < rows; r++) take(r);
    else {
      std::vector<uint64_t> hits;
      for (size_t i = 0; i < want.size(); i++) {      // the partition's keys ascend: a binary search a listed k-mer
        uint64_t lo = 0, hi = rows;
        while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (key_less(row_key(mid), want[i].data(), kw)) lo = mid + 1; else hi = mid; }
        if (lo < rows && !key_less(want[i].data(), row_key(lo), kw)) { found[i] = true; hits.push_back(lo); }
      }
      std::sort(hits.begin(), hits.end());
      for (uint64_t r : hits) take(r);
    }
  }
  const uint64_t n = keys.size() / kw;
  if (listed) {
    const uint64_t missing = (uint64_t)std::count(found.begin(), found.end(), false);
    if (missing || o.verbose) fprintf(stderr, "[kmx unitigs] %llu of the %llu listed k-mers are not in the run: dropped\n", (unsigned long long)missing, (unsigned long long)want.size());
  }

  // ---- the graph, on one device ----
  Devices dev = open_devices(o.gpus, o.batch_mb ? o.batch_mb : 256, 4);      // (the table's budget is given: the devices' memory is not asked)
  const uint32_t G = dev.G();
  kmx_ctx* c0 = dev.ctxs[0];
  kmx_unitigs_task ut; memset(&ut, 0, sizeof ut);
  ut.keys = keys.data(); ut.n = n; ut.kmer_size = k; ut.key_words = kw;
  kmx_unitigs_result* ur = nullptr;
  chk(c0, kmx_unitigs_host(c0, &ut, &ur), "kmx_unitigs_host");
  chk(c0, kmx_unitigs_result_wait(ur), "kmx_unitigs");
  const uint64_t U = kmx_unitigs_result_n_unitigs(ur);
  std::vector<uint32_t> unitig(n), len(U);
  std::vector<uint8_t> circ(U);
  std::vector<uint64_t> seq_off(U + 1);
  chk(c0, kmx_unitigs_result_copy_unitig(ur, unitig.data(), n), "kmx_unitigs_result_copy_unitig");
  chk(c0, kmx_unitigs_result_copy_len(ur, len.data(), U), "kmx_unitigs_result_copy_len");
  chk(c0, kmx_unitigs_result_copy_circ(ur, circ.data(), U), "kmx_unitigs_result_copy_circ");
  chk(c0, kmx_unitigs_result_copy_seq_off(ur, seq_off.data(), U + 1), "kmx_unitigs_result_copy_seq_off");
  if (o.verbose) fprintf(stderr, "[kmx unitigs] %llu k-mers of %llu partitions (%s), k = %u: %llu unitigs\n", (unsigned long long)n, (unsigned long long)P, dir.mode.c_str(), k,
                         (unsigned long long)U);
  if (!o.out.empty()) {
    std::vector<uint8_t> seqs(kmx_unitigs_result_seq_bytes(ur));
    chk(c0, kmx_unitigs_result_copy_seqs(ur, seqs.data(), seqs.size()), "kmx_unitigs_result_copy_seqs");
    std::string t;
    t.reserve(seqs.size() + 48 * U);
    for (uint64_t u = 0; u < U; u++) {
      t += ">" + std::to_string(u) + " LN:i:" + std::to_string(seq_off[u + 1] - seq_off[u]) + " KM:i:" + std::to_string(len[u]) + (circ[u] ? " CL:Z:circular\n" : "\n");
      t.append((const char*)&seqs[seq_off[u]], seq_off[u + 1] - seq_off[u]);
      t += '\n';
    }
    write_text(o.out, t);
  }
  kmx_unitigs_result_free(ur);
  keys = std::vector<uint64_t>();

  // ---- the table: windows of unitigs, every partition through kmx_groupsum_host, a shard's device tables accumulating ----
  if (!o.table.empty()) {
    const bool sums = value == "sum" || value == "mean";
    std::string t = "unitig\tkmers";
    for (uint32_t j = 0; j < M; j++) t += "\t" + samples[cols.empty() ? j : cols[j]].id;
    t += "\n";
    for (uint64_t p = 0; p < P; p++) for (uint32_t& v : node_of[p]) if (v != 0xFFFFFFFFu) v = unitig[v];      // a row's label: its unitig
    const uint64_t per_group = 4 + 4ull * M + (sums ? 8ull * M : 0);
    const uint64_t win = std::min<uint64_t>(std::max<uint64_t>(dev.budget / per_group, 1), std::min<uint64_t>(std::max<uint64_t>(U, 1), (1ull << 32) / M));
    if (o.verbose) fprintf(stderr, "[kmx unitigs] table: %u of %u samples, value %s, windows of %llu unitigs, %u shards\n", M, N, value.c_str(), (unsigned long long)win, G);
    for (uint64_t g0 = 0; g0 < U; g0 += win) {
      const uint32_t Gw = (uint32_t)std::min<uint64_t>(win, U - g0);
      std::vector<uint32_t> size(Gw, 0), present((uint64_t)Gw * M, 0);
      std::vector<uint64_t> sum(sums ? (uint64_t)Gw * M : 0, 0);
      std::mutex mu;
      in_shards(G, [&](uint32_t g) {
        kmx_ctx* ctx = dev.ctxs[g];
        kmx_groupsum_result* first = nullptr;
        for (uint64_t p = g; p < P; p += G) {
          const auto body = dir.load(p);
          kmx_groupsum_task gt; memset(&gt, 0, sizeof gt);
          gt.key_words = kw; gt.mode = dir.rmode(); gt.n_cols = N; gt.n_use = M;
          gt.rows = body->data(); gt.n_rows = body->size() / stride; gt.cols = cols.empty() ? nullptr : cols.data(); gt.groups = node_of[p].data();
          gt.min_abund = o.min_abund; gt.flags = sums ? KMX_GROUPSUM_SUMS : 0; gt.g0 = (uint32_t)g0; gt.n_groups = Gw;
          if (first) { gt.present = kmx_groupsum_result_present_dev(first); gt.size = kmx_groupsum_result_size_dev(first); gt.sums = sums ? kmx_groupsum_result_sums_dev(first) : nullptr; }
          kmx_groupsum_result* r = nullptr;
          chk(ctx, kmx_groupsum_host(ctx, &gt, &r), "kmx_groupsum_host");
          chk(ctx, kmx_groupsum_result_wait(r), "kmx_groupsum");      // (the body goes at the end of this trip)
          if (first) kmx_groupsum_result_free(r); else first = r;
        }
        if (!first) return;
        std::vector<uint32_t> sz(Gw), pr((uint64_t)Gw * M);
        std::vector<uint64_t> sm(sum.size());
        chk(ctx, kmx_groupsum_result_copy_size(first, sz.data(), sz.size()), "kmx_groupsum_result_copy_size");
        chk(ctx, kmx_groupsum_result_copy_present(first, pr.data(), pr.size()), "kmx_groupsum_result_copy_present");
        if (sums) chk(ctx, kmx_groupsum_result_copy_sums(first, sm.data(), sm.size()), "kmx_groupsum_result_copy_sums");
        kmx_groupsum_result_free(first);
        std::lock_guard<std::mutex> lk(mu);
        for (size_t i = 0; i < sz.size(); i++) size[i] += sz[i];
        for (size_t i = 0; i < pr.size(); i++) present[i] += pr[i];
        for (size_t i = 0; i < sm.size(); i++) sum[i] += sm[i];
      });
      char buf[64];
      for (uint32_t u = 0; u < Gw; u++) {
        if (size[u] != len[g0 + u]) die("kmx_groupsum: a unitig's rows are not its k-mers");
        t += std::to_string(g0 + u) + "\t" + std::to_string(size[u]);
        for (uint32_t j = 0; j < M; j++) {
          const uint64_t i = (uint64_t)u * M + j;
          if (value == "sum") snprintf(buf, sizeof buf, "\t%llu", (unsigned long long)sum[i]);
          else if (value == "present") snprintf(buf, sizeof buf, "\t%u", present[i]);
          else if (value == "mean") snprintf(buf, sizeof buf, "\t%.2f", (double)sum[i] / (double)size[u]);
          else snprintf(buf, sizeof buf, "\t%.2f", (double)present[i] / (double)size[u]);
          t += buf;
        }
        t += "\n";
      }
    }
    write_text(o.table, t);
  }
  dev.close();
  return 0;
}
