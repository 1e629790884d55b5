// kmx_match.cpp -- `kmx match`: the reads that hold the k-mers of a set (kmdiff's map-back, the read fetch of a k-mer GWAS, what the
// kmtricks authors ship back_to_sequences for; no counterpart in the kmtricks tree; include/kmx.h, sections "kset" and "match").  The set
// comes from a list of k-mers (--kmers: a `kmx diff` / `kmx assoc` output), from the k-mers of sequences (--seqs: a `kmx unitigs --output`)
// or from the row keys of a run (--run); it is canonicalised here and handed over WITH its duplicates: the device dedups.  Every device
// builds the set once (kmx_kset_host); the reads go through kmx_match_host in batches cut between reads, round-robin over the devices, the
// outputs in input order; a device's occurrence table accumulates across its batches and the devices' tables are added here at the end.
// Every check that needs no GPU comes before kmx_create.
#include "kmx_driver.hpp"

using namespace kmxdrv;

namespace {

struct MOpt {
  std::string kmers, seqs, run, out, extract, counts, positions;
  std::vector<std::string> reads;
  uint32_t gpus = 1, k = 0, min_hits = 1;
  double min_frac = -1, min_cover = -1;      // < 0: not given
  bool invert = false, filters = false, verbose = false;
  uint64_t batch_mb = 0;      // 0: 256
};

const char* USAGE = "usage: kmx match (--kmers FILE | --seqs FILE --kmer-size K | --run RUN) --reads FILE [--reads FILE ...] [--output FILE] [--extract FILE] "
                    "[--min-hits INT] [--min-frac F] [--min-cover F] [--invert] [--kmer-counts FILE] [--positions FILE] [--batch-mb INT] [--gpus INT] [-v]\n"
                    "  Finds the reads (FASTA / FASTQ, plain or gz) that hold the k-mers of a set.  The set: --kmers, the first tab-separated field of each "
                    "line of FILE (what kmx diff and kmx assoc --output write; # lines and their header line `kmer ...` are skipped, either strand is accepted, "
                    "k is the first k-mer's length); --seqs, every k-mer of every record of a FASTA (what kmx unitigs --output writes); --run, every row key "
                    "of a run made with --mode kmer:count:bin or kmer:pa:bin, plain or --cpr.  The set must fit one device.\n"
                    "  --output: one line per read in input order -- read, name, length, kmers, hits, fwd, covered, first, last (- for none).\n"
                    "  --extract: the reads with hits >= --min-hits (default 1), hits >= F * kmers (--min-frac) and covered >= F * length (--min-cover), "
                    "or with --invert the others, in their input format; the header line gains KM:i:{kmers} HT:i:{hits} FW:i:{fwd} CV:i:{covered}.\n"
                    "  --kmer-counts: kmer, count per distinct k-mer of the set, in the order of first appearance.  --positions: read, pos, kmer_index, strand "
                    "per hit.\n"
                    "  The reads go to the devices in batches of --batch-mb (default 256) cut between reads.  Paired reads, approximate matching and "
                    "per-read distinct counts are not done.";

MOpt parse(int argc, char** argv)
{
  MOpt o;
  const Args in{argc, argv, USAGE};
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--kmers") o.kmers = in.need(i);
    else if (a == "--seqs") o.seqs = in.need(i);
    else if (a == "--run") o.run = in.need(i);
    else if (a == "--kmer-size") o.k = in.u32(i);
    else if (a == "--reads") o.reads.push_back(in.need(i));
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--extract") o.extract = in.need(i);
    else if (a == "--min-hits") { o.min_hits = in.u32(i); o.filters = true; }
    else if (a == "--min-frac") { o.min_frac = in.frac(i); o.filters = true; }
    else if (a == "--min-cover") { o.min_cover = in.frac(i); o.filters = true; }
    else if (a == "--invert") { o.invert = true; o.filters = true; }
    else if (a == "--kmer-counts") o.counts = in.need(i);
    else if (a == "--positions") o.positions = in.need(i);
    else if (a == "--gpus") o.gpus = in.u32(i);
    else if (a == "--batch-mb") o.batch_mb = in.num(i);
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if ((int)!o.kmers.empty() + (int)!o.seqs.empty() + (int)!o.run.empty() != 1) die(std::string("exactly one of --kmers, --seqs and --run is required\n") + USAGE);
  if (!o.seqs.empty() && o.k == 0) die("--seqs needs --kmer-size");
  if (o.seqs.empty() && o.k != 0) die("--kmer-size goes with --seqs (a list's k is its first k-mer's length, a run's is the run's)");
  if (!o.seqs.empty() && (o.k < 8 || o.k > 127)) die("--kmer-size must be in [8, 127]");
  if (o.reads.empty()) die(std::string("--reads is required\n") + USAGE);
  if (o.out.empty() && o.extract.empty() && o.counts.empty() && o.positions.empty())
    die(std::string("one of --output, --extract, --kmer-counts and --positions is required\n") + USAGE);
  if (o.filters && o.extract.empty()) die("--min-hits, --min-frac, --min-cover and --invert need --extract");
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  if (o.batch_mb > 4095) die("--batch-mb must be below 4096 (a call takes fewer than 2^32 bases)");
  return o;
}

bool key_less(const uint64_t* a, const uint64_t* b, uint32_t kw) { for (uint32_t w = kw; w-- > 0;) if (a[w] != b[w]) return a[w] < b[w]; return false; }

// the canonical key of the k characters at s (ACGT, either case) behind `keys`; fwd: the characters show the key itself (a palindrome does).
// false, and nothing appended: a character that is none of them
bool push_canonical(const char* s, uint32_t k, uint32_t kw, std::vector<uint64_t>& keys, bool* fwd = nullptr)
{
  uint64_t f[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
  for (uint32_t j = 0; j < k; j++) {
    uint64_t d;
    switch (s[j]) { case 'A': case 'a': d = 0; break; case 'C': case 'c': d = 1; break; case 'T': case 't': d = 2; break; case 'G': case 'g': d = 3; break; default: return false; }
    const uint32_t fi = k - 1 - j, ri = j;      // base j is digit k - 1 - j forward, and its complement digit j of the reverse complement
    f[fi >> 5] |= d << (2 * (fi & 31));
    r[ri >> 5] |= (d ^ 2) << (2 * (ri & 31));
  }
  const bool rev = key_less(r, f, kw);
  if (fwd) *fwd = !rev;
  keys.insert(keys.end(), rev ? r : f, (rev ? r : f) + kw);
  return true;
}

std::string key_string(const uint64_t* key, uint32_t k)
{
  std::string s(k, 'A');
  for (uint32_t j = 0; j < k; j++) { const uint32_t d = k - 1 - j; s[j] = "ACTG"[(key[d >> 5] >> (2 * (d & 31))) & 3]; }
  return s;
}

// one batch of reads on its way through a device
struct Batch {
  uint64_t first_read = 0;
  std::string bases;
  std::vector<uint64_t> offs{0};
  std::vector<std::string> names, headers, quals;      // headers, quals: with --extract
  std::vector<uint8_t> fastq;
  std::vector<kmx_match_rec> recs;
  std::vector<uint32_t> ids;                           // with --positions
  size_t n() const { return offs.size() - 1; }
  void clear() { bases.clear(); offs.assign(1, 0); names.clear(); headers.clear(); quals.clear(); fastq.clear(); recs.clear(); ids.clear(); }
};

struct Sink {
  std::string path; FILE* f = nullptr;
  void open(const std::string& p) { path = p; if (p.empty()) return; f = fopen(p.c_str(), "w"); if (!f) die("Unable to write at " + p); }
  void put(const std::string& t) { if (f && !t.empty() && fwrite(t.data(), 1, t.size(), f) != t.size()) die("write failed: " + path); }
  void close() { if (f && fclose(f) != 0) die("write failed: " + path); f = nullptr; }
};

}  // namespace

int kmx_match_main(int argc, char** argv)
{
  const MOpt o = parse(argc, argv);
  // ---- the set, canonical and with its duplicates; every check before kmx_create ----
  uint32_t k = o.k, kw = (o.k + 31) / 32;
  std::vector<uint64_t> keys;
  if (!o.kmers.empty()) {
    std::ifstream f(o.kmers);
    if (!f) die("Unable to read at " + o.kmers);
    std::string line;
    for (uint64_t ln = 1; std::getline(f, line); ln++) {
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty() || line[0] == '#') continue;
      const std::string s = line.substr(0, line.find('\t'));
      if (s == "kmer") continue;      // the header line of kmx diff / kmx assoc
      const std::string where = o.kmers + " line " + std::to_string(ln) + ": ";
      if (k == 0) {
        k = (uint32_t)std::min<size_t>(s.size(), 1000); kw = (k + 31) / 32;
        if (k < 8 || k > 127) die(where + "a k-mer of " + std::to_string(s.size()) + " characters: k must be in [8, 127]");
      }
      if (s.size() != k) die(where + "a k-mer of " + std::to_string(s.size()) + " characters, the first has " + std::to_string(k));
      if (!push_canonical(s.data(), k, kw, keys)) die(where + "malformed k-mer " + s);
    }
    if (k == 0) die(o.kmers + " names no k-mer");
  } else if (!o.seqs.empty()) {
    SeqReader rd(o.seqs);
    std::string seq;
    while (rd.next(seq)) for (size_t i = 0; i + k <= seq.size(); i++) (void)push_canonical(seq.data() + i, k, kw, keys);
  } else {
    RunDir dir;
    dir.at("match", o.run);
    dir.read_mode(KMER_KINDS, "kmer:count:bin or kmer:pa:bin (the keys of hash and Bloom filter runs are not k-mers)");
    dir.shape();
    dir.open_files();
    k = dir.k; kw = dir.kw;
    for (uint64_t p = 0; p < dir.P; p++) {
      const auto body = dir.load(p);
      const uint64_t rows = body->size() / dir.stride;
      const size_t at = keys.size();
      keys.resize(at + rows * kw);
      for (uint64_t r = 0; r < rows; r++) memcpy(&keys[at + r * kw], body->data() + r * dir.stride, 8ull * kw);
    }
  }
  const uint64_t n = keys.size() / kw;
  if (n > (1ull << 31)) die("more than 2^31 k-mers: a set is built in one call");
  for (const std::string& p : o.reads) { SeqReader probe(p); (void)probe; }      // (Unable to read at ...)

  // ---- the devices: every one builds the set ----
  Devices dev = open_devices(o.gpus, o.batch_mb ? o.batch_mb : 256, 4);
  const uint32_t G = dev.G();
  const uint64_t batch_bytes = dev.budget;
  const bool want_occ = !o.counts.empty(), want_ids = !o.positions.empty(), want_records = !o.extract.empty();
  std::vector<kmx_kset*> sets(G, nullptr);
  for (uint32_t g = 0; g < G; g++) {
    kmx_kset_task st; memset(&st, 0, sizeof st);
    st.keys = keys.data(); st.n = n; st.kmer_size = k; st.key_words = kw;
    chk(dev.ctxs[g], kmx_kset_host(dev.ctxs[g], &st, &sets[g]), "kmx_kset_host");
  }
  for (uint32_t g = 0; g < G; g++) chk(dev.ctxs[g], kmx_kset_wait(sets[g]), "kmx_kset");
  const uint64_t n_distinct = kmx_kset_n_distinct(sets[0]);
  if (o.verbose) fprintf(stderr, "[kmx match] a set of %llu k-mers (%llu distinct), k = %u, on %u device contexts; batches of %llu MB\n", (unsigned long long)n,
                         (unsigned long long)n_distinct, k, G, (unsigned long long)(batch_bytes >> 20));
  Sink out, ext, pos;
  out.open(o.out); ext.open(o.extract); pos.open(o.positions);
  out.put("read\tname\tlength\tkmers\thits\tfwd\tcovered\tfirst\tlast\n");
  pos.put("read\tpos\tkmer_index\tstrand\n");

  // ---- the reads: G batches at a time, one a device; the results written in input order ----
  std::vector<Batch> batch(G);
  std::vector<kmx_match_result*> first(G, nullptr);      // owns the device's occurrence table
  uint64_t n_reads = 0, total_kmers = 0, total_hits = 0, kept_reads = 0, n_batches = 0;
  auto run_batches = [&](uint32_t filled) {
    in_shards(filled, [&](uint32_t g) {
      kmx_ctx* ctx = dev.ctxs[g];
      Batch& b = batch[g];
      kmx_match_task t; memset(&t, 0, sizeof t);
      t.set = sets[g]; t.bases = b.bases.data(); t.offsets = b.offs.data(); t.n_seqs = b.n();
      t.flags = (want_ids ? KMX_MATCH_IDS : 0) | (want_occ ? KMX_MATCH_OCC : 0);
      t.occ = want_occ && first[g] ? kmx_match_result_occ_dev(first[g]) : nullptr;
      kmx_match_result* r = nullptr;
      chk(ctx, kmx_match_host(ctx, &t, &r), "kmx_match_host");
      chk(ctx, kmx_match_result_wait(r), "kmx_match");
      b.recs.resize(b.n());
      chk(ctx, kmx_match_result_copy_recs(r, b.recs.data(), b.recs.size()), "kmx_match_result_copy_recs");
      if (want_ids) { b.ids.resize(b.bases.size()); chk(ctx, kmx_match_result_copy_ids(r, b.ids.data(), b.ids.size()), "kmx_match_result_copy_ids"); }
      if (want_occ && !first[g]) first[g] = r; else kmx_match_result_free(r);
    });
    for (uint32_t g = 0; g < filled; g++) {
      const Batch& b = batch[g];
      std::string to, te, tp;
      char buf[160];
      for (size_t q = 0; q < b.n(); q++) {
        const kmx_match_rec& r = b.recs[q];
        const uint64_t len = b.offs[q + 1] - b.offs[q], read = b.first_read + q;
        total_kmers += r.n_kmers; total_hits += r.hits;
        if (out.f) {
          to += std::to_string(read) + "\t" + b.names[q] + "\t" + std::to_string(len);
          snprintf(buf, sizeof buf, "\t%u\t%u\t%u\t%u\t", r.n_kmers, r.hits, r.fwd, r.covered);
          to += buf;
          to += r.first == 0xFFFFFFFFu ? std::string("-\t-\n") : std::to_string(r.first) + "\t" + std::to_string(r.last) + "\n";
        }
        if (ext.f) {
          bool keep = r.hits >= o.min_hits;
          if (o.min_frac >= 0) keep = keep && (double)r.hits >= o.min_frac * (double)r.n_kmers;
          if (o.min_cover >= 0) keep = keep && (double)r.covered >= o.min_cover * (double)len;
          if (o.min_frac >= 0 || o.min_cover >= 0) keep = keep && r.n_kmers > 0;
          if (keep != o.invert) {
            kept_reads++;
            snprintf(buf, sizeof buf, " KM:i:%u HT:i:%u FW:i:%u CV:i:%u\n", r.n_kmers, r.hits, r.fwd, r.covered);
            te += b.headers[q]; te += buf;
            te.append(b.bases, b.offs[q], len); te += '\n';
            if (b.fastq[q]) { te += "+\n"; te += b.quals[q]; te += '\n'; }
          }
        }
        if (pos.f && r.hits) {
          std::vector<uint64_t> scratch;
          for (uint64_t i = r.first; i <= r.last; i++) {
            const uint32_t j = b.ids[b.offs[q] + i];
            if (j == 0xFFFFFFFFu) continue;
            bool fwd = true;
            scratch.clear();
            (void)push_canonical(b.bases.data() + b.offs[q] + i, k, kw, scratch, &fwd);
            tp += std::to_string(read) + "\t" + std::to_string(i) + "\t" + std::to_string(j) + (fwd ? "\t+\n" : "\t-\n");
          }
        }
      }
      out.put(to); ext.put(te); pos.put(tp);
      n_batches++;
      batch[g].clear();
    }
  };
  uint32_t cur = 0;
  batch[0].first_read = 0;
  for (const std::string& path : o.reads) {
    SeqReader rd(path);
    rd.keep_records();
    std::string seq;
    while (rd.next(seq)) {
      Batch* b = &batch[cur];
      // a batch is cut between reads: when the next one would take it past --batch-mb (a read larger than a batch goes alone) or past 2^32 - 1 bases
      if (b->n() && (b->bases.size() + seq.size() > batch_bytes || b->bases.size() + seq.size() > 0xFFFFFFFFull)) {
        if (++cur == G) { run_batches(G); cur = 0; }
        b = &batch[cur];
        b->first_read = n_reads;
      }
      b->bases += seq; b->offs.push_back(b->bases.size()); b->names.push_back(rd.name());
      if (want_records) { b->headers.push_back(rd.header()); b->quals.push_back(rd.quality()); b->fastq.push_back(rd.fastq() ? 1 : 0); }
      n_reads++;
    }
  }
  if (batch[cur].n()) cur++;
  if (cur) run_batches(cur);
  out.close(); ext.close(); pos.close();

  // ---- the occurrences: the devices' tables added, one line per distinct k-mer in id order ----
  if (want_occ) {
    std::vector<uint64_t> occ(n, 0), part(n);
    for (uint32_t g = 0; g < G; g++) {
      if (!first[g]) continue;
      chk(dev.ctxs[g], kmx_match_result_copy_occ(first[g], part.data(), n), "kmx_match_result_copy_occ");
      for (uint64_t v = 0; v < n; v++) occ[v] += part[v];
      kmx_match_result_free(first[g]);
    }
    std::vector<uint32_t> ids(n);
    chk(dev.ctxs[0], kmx_kset_copy_ids(sets[0], ids.data(), n), "kmx_kset_copy_ids");
    std::string t = "kmer\tcount\n";
    for (uint64_t v = 0; v < n; v++) if (ids[v] == v) t += key_string(&keys[v * kw], k) + "\t" + std::to_string(occ[v]) + "\n";
    write_text(o.counts, t);
  }
  if (o.verbose) fprintf(stderr, "[kmx match] %llu reads in %llu batches: %llu k-mers, %llu hits%s\n", (unsigned long long)n_reads, (unsigned long long)n_batches,
                         (unsigned long long)total_kmers, (unsigned long long)total_hits,
                         ext.path.empty() ? "" : (", " + std::to_string(kept_reads) + " reads kept").c_str());
  for (uint32_t g = 0; g < G; g++) kmx_kset_free(sets[g]);
  dev.close();
  return 0;
}
