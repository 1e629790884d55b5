// kmx_query.cpp -- `kmx query`: which samples of a `--mode hash:bf:bin` run hold the k-mers of a set of sequences (what kmtricks 1.0
// shipped as `kmtricks query`, doc/changelogs/v1.0.0.md, and kmindex does today; no counterpart in the 1.6.0 tree).  The index is the
// run directory as `kmx pipeline` / kmtricks leave it; the queries go through kmx_query_host in batches, the partitions' matrices in
// groups that fit the device, a group's hits added on the device to the table of the groups before it.  Every check that needs no
// GPU comes before kmx_create.  `--kmer-index` asks the same of the k-mer matrices of a kmer:count:bin / kmer:pa:bin run (kquery_main).
// `--z Z` asks the Bloom index for (k + Z)-mers (the findere trick: kmx_zquery_host, one bits table a batch across its partition groups).
// `--index` of a `--mode hash:bfc:bin` run (a counting Bloom index: fields of --bitw bits a sample) goes through kmx_cquery_host: hits are
// the k-mers whose abundance class is at least --min-class, `--format sums` prints the sums of the classes' least counts.
#include "kmx_driver.hpp"

using namespace kmxdrv;

namespace {

struct QOpt {
  std::string index, kmer_index, query, out, format = "matrix";
  double threshold = 0.7;
  uint32_t gpus = 1, threads = 8;
  uint64_t batch_mb = 0;      // 0: sized from the device's free memory
  int64_t z = -1;             // --z: (k + z)-mers, the findere trick (zquery_batch); < 0: not given
  int64_t min_class = -1;     // --min-class: a counting Bloom index's hit is a class of at least this; < 0: not given (1)
  bool verbose = false;
};

const char* USAGE = "usage: kmx query (--index <run dir made with --mode hash:bf:bin or hash:bfc:bin> | --kmer-index <run dir made with --mode kmer:count:bin or kmer:pa:bin>) "
                    "--query <fasta|fastq[.gz]> [--output FILE] [--threshold FLOAT] [--format matrix|list|sums (sums: --kmer-index of a count run, --index of a hash:bfc:bin run)] "
                    "[--z INT (--index of a hash:bf:bin run only: ask for (k + z)-mers, 0 ... 8)] [--min-class INT (--index of a hash:bfc:bin run only: a hit is an abundance class of at least this, default 1)] "
                    "[--gpus INT] [--query-batch-mb INT] [-t INT (accepted, no effect)] [-v]";

QOpt parse(int argc, char** argv)
{
  QOpt o;
  const Args in{argc, argv, USAGE};
  // (a number may carry a sign here: `--z -1` wraps and is told its range, not that it is no number)
  auto num = [&](int& i) -> unsigned long { const std::string v = in.need(i); try { size_t n = 0; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--index") o.index = in.need(i);
    else if (a == "--kmer-index") o.kmer_index = in.need(i);
    else if (a == "--query") o.query = in.need(i);
    else if (a == "--output") o.out = in.need(i);
    else if (a == "--threshold") o.threshold = in.real(i);
    else if (a == "--format") { o.format = in.need(i); if (o.format != "matrix" && o.format != "list" && o.format != "sums") die("--format must be matrix, list or sums"); }
    else if (a == "--gpus") o.gpus = num(i);
    else if (a == "--z") { const unsigned long v = num(i); if (v > 8) die("--z must be in [0, 8]"); o.z = (int64_t)v; }
    else if (a == "--min-class") o.min_class = (int64_t)std::min<unsigned long>(num(i), 0xFFFFFFFFul);
    else if (a == "--query-batch-mb") o.batch_mb = num(i);
    else if (a == "-t" || a == "--threads") o.threads = num(i);
    else if (in.verbose(a, i)) o.verbose = true;
    else in.unknown(a);
  }
  if (o.index.empty() == o.kmer_index.empty()) die(std::string("exactly one of --index and --kmer-index is required\n") + USAGE);
  if (o.query.empty()) die(std::string("--query is required\n") + USAGE);
  if (o.gpus < 1 || o.gpus > 16) die("--gpus must be in [1, 16]");
  if (o.threshold < 0.0 || o.threshold > 1.0) die("--threshold must be in [0, 1]");
  if (o.z >= 0 && !o.kmer_index.empty()) die("--z removes Bloom false positives: an exact index (--kmer-index) has none");
  if (o.min_class >= 0 && !o.kmer_index.empty()) die("--min-class is for a counting Bloom index (--index of a run made with --mode hash:bfc:bin): an exact index has counts, not classes");
  if (o.z >= 0 && o.gpus > 1) die("--z with --gpus above 1 is not supported: shards own partitions, a window's k-mers lie in several shards, and the shards' tables are not joined across devices");
  return o;
}

constexpr size_t CMBF_HEADER = 49, KMATRIX_HEADER = 45;

// ---- `kmx query --kmer-index`: the same questions asked of the .count / .pa k-mer matrices of a kmer:count:bin / kmer:pa:bin run --
//      exact, and in count mode with abundances (kmx_kquery_host).  Partition groups, query batches and shards as above. ----
int kquery_main(const QOpt& o)
{
  const std::string& run = o.kmer_index;
  // ---- the index: a run directory of --mode kmer:count:bin or kmer:pa:bin; every check before kmx_create ----
  if (!fs::exists(run + "/kmtricks.fof")) die(run + " is not a kmtricks runtime directory.");
  std::string opt; { std::ifstream f(run + "/options.txt"); if (!f) die("Unable to read at " + run + "/options.txt"); std::getline(f, opt); }
  const std::string mode = option_of(opt, "count_format") + ":" + option_of(opt, "mode") + ":" + option_of(opt, "format");
  if (mode != "kmer:count:bin" && mode != "kmer:pa:bin")
    die("kmx query --kmer-index needs a run made with --mode kmer:count:bin or kmer:pa:bin; " + run + " was made with " + mode + (mode == "hash:bf:bin" ? " (a Bloom index: --index)" : ""));
  const bool pa = mode == "kmer:pa:bin";
  if (o.format == "sums" && pa) die("--format sums needs a run made with --mode kmer:count:bin: presence/absence rows have no counts to sum");
  uint32_t k = 0;
  try { k = (uint32_t)std::stoul(option_of(opt, "kmer_size")); } catch (...) { die(run + "/options.txt names no kmer_size"); }
  GatbConfig gc;
  if (!GatbConfig::load(run + "/config_gatb/gatb.config", gc)) die("Unable to read at " + run + "/config_gatb/gatb.config");
  uint16_t rp = 0;
  const std::vector<uint16_t> table = read_repartition(run + "/repartition_gatb/repartition.minimRepart", &rp);
  const uint32_t msize = (uint32_t)gc.minim_size, kw = (k + 31) / 32;
  const uint64_t P = rp;
  if (k < 8 || k > 127 || gc.kmer_size != k || msize < 4 || msize > 15 || msize >= k || table.size() != ((size_t)1 << (2 * msize)) || P == 0)
    die("the index's options.txt, gatb.config and repartition table do not fit together");
  for (uint16_t t : table) if (t >= P) die("the index's repartition table names a partition the run does not have");
  const std::vector<Sample> samples = parse_fof(run + "/kmtricks.fof", 1);
  const uint32_t N = (uint32_t)samples.size();
  const uint64_t stride = 8ull * kw + (pa ? (N + 7) / 8 : 4ull * N);
  std::vector<std::string> files(P);
  std::vector<uint64_t> n_rows(P, 0);
  for (uint64_t p = 0; p < P; p++) {
    const std::string plain = run + "/matrices/matrix_" + std::to_string(p) + (pa ? ".pa" : ".count");
    const bool lz = !fs::exists(plain) && fs::exists(plain + ".lz4");
    files[p] = lz ? plain + ".lz4" : plain;
    std::ifstream f(files[p], std::ios::binary);
    uint8_t h[KMATRIX_HEADER];
    if (!f || !f.read((char*)h, KMATRIX_HEADER)) die("Unable to read at " + plain);
    if (rd<uint64_t>(&h[0]) != MAGIC_BASE || rd<uint64_t>(&h[13]) != (pa ? MAGIC_PA : MAGIC_MATRIX)) die("Invalid file format: " + files[p]);
    if (rd<uint32_t>(&h[21]) != k || rd<uint32_t>(&h[25]) != kw)
      die(files[p] + " was made with k = " + std::to_string(rd<uint32_t>(&h[21])) + " in " + std::to_string(rd<uint32_t>(&h[25])) + " words, the index's options.txt says " + std::to_string(k));
    const uint32_t cols = rd<uint32_t>(&h[pa ? 29 : 33]);
    if (cols != N) die(files[p] + " has rows of " + std::to_string(cols) + " columns, the index's kmtricks.fof has " + std::to_string(N) + " samples");
    if (pa && rd<uint32_t>(&h[33]) != (N + 7) / 8) die("Invalid file format: " + files[p]);
    uint64_t body = 0;
    if (h[12]) {      // lz4: the body's size is known once it is unpacked (read_matrix checks that it is whole rows)
      uint32_t fk = 0, fn = 0;
      body = read_matrix(files[p], pa, 4, &fk, &fn).size();
    } else {
      std::error_code ec;
      body = fs::file_size(files[p], ec) - KMATRIX_HEADER;
      if (ec || body % stride) die("truncated matrix (its body is no whole number of rows of " + std::to_string(stride) + " bytes): " + files[p]);
    }
    n_rows[p] = body / stride;
    if (n_rows[p] > 0xFFFFFF00ull) die(files[p] + " has more than 2^32 - 256 rows");
  }

  // ---- the queries ----
  std::string bases; std::vector<uint64_t> offs{0}; std::vector<std::string> names;
  { SeqReader rd(o.query); rd.keep_names(); std::string seq; while (rd.next(seq)) { bases += seq; offs.push_back(bases.size()); names.push_back(rd.name()); } }
  const uint64_t Q = names.size();
  FILE* out = o.out.empty() ? stdout : fopen(o.out.c_str(), "w");
  if (!out) die("Unable to write at " + o.out);

  // ---- devices; how many bases a batch of queries holds and which partitions a group ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 6);
  const uint32_t G = dev.G();
  const uint64_t budget = dev.budget;
  const bool want_sums = o.format == "sums";
  // half for a group's matrices, half for a batch: 11 + 8 * key words bytes a base (the bases and the call's scratch) and a row of the
  // tables a query
  const uint64_t group_bytes = std::max<uint64_t>(budget / 2, 1), batch_bytes = std::max<uint64_t>(budget / 2, 1);
  const uint64_t per_base = 11 + 8ull * kw, per_query = (want_sums ? 12ull : 4ull) * N + 12;
  std::vector<uint64_t> cut{0};      // batch b = queries [cut[b], cut[b + 1])
  { uint64_t used = 0;
    for (uint64_t q = 0; q < Q; q++) {
      const uint64_t len = offs[q + 1] - offs[q], cost = per_base * len + per_query;
      if (len > 0xFFFFFFFFull) die("query " + names[q] + " has 2^32 bases or more");
      if (q > cut.back() && (used + cost > batch_bytes || offs[q + 1] - offs[cut.back()] > 0xFFFFFFFFull)) { cut.push_back(q); used = 0; }
      used += cost;
    }
    cut.push_back(Q); if (Q == 0) cut.pop_back(); }
  std::vector<std::vector<std::vector<uint32_t>>> groups(G);      // per shard: its partitions (p mod G) in groups of at most group_bytes
  size_t n_groups = 0;
  { std::vector<uint64_t> fill(G, 0);
    for (uint64_t p = 0; p < P; p++) {
      auto& gs = groups[p % G]; const uint64_t b = n_rows[p] * stride;
      if (gs.empty() || (fill[p % G] + b > group_bytes && !gs.back().empty())) { gs.emplace_back(); fill[p % G] = 0; }
      gs.back().push_back((uint32_t)p); fill[p % G] += b;
    } }
  for (auto& gs : groups) n_groups = std::max(n_groups, gs.size());
  if (o.verbose) fprintf(stderr, "[kmx query] %llu queries, %zu bases, k %u, %u samples, %llu partitions of k-mer rows (%s): %zu query batches, %zu partition groups a shard, %u shards\n",
                         (unsigned long long)Q, bases.size(), k, N, (unsigned long long)P, pa ? "pa" : "count", cut.size() - 1, n_groups, G);

  if (o.format != "list") { std::string h = "query\tn_kmers"; for (const Sample& s : samples) { h += '\t'; h += s.id; } h += '\n'; fwrite(h.data(), 1, h.size(), out); }
  // a shard whose partitions fit one group reads its matrices once; a shard with several groups reads every group again for every
  // batch of queries
  std::vector<std::vector<std::vector<uint8_t>>> kept(G);
  for (size_t b = 0; b + 1 < cut.size(); b++) {
    const uint64_t q0 = cut[b], nq = cut[b + 1] - q0;
    std::vector<uint64_t> boffs(nq + 1);
    for (uint64_t i = 0; i <= nq; i++) boffs[i] = offs[q0 + i] - offs[q0];
    std::vector<uint32_t> hits(nq * N, 0), kmers(nq, 0);
    std::vector<uint64_t> sums(want_sums ? nq * N : 0, 0);
    std::mutex mu;
    // every shard sees all queries of the batch; its groups add up on its device, the shards' tables on the host
    auto shard = [&](uint32_t g) {
      kmx_ctx* ctx = dev.ctxs[g];
      kmx_kquery_result* first = nullptr;
      std::vector<std::vector<uint8_t>> own;
      const bool keep = groups[g].size() == 1;
      std::vector<std::vector<uint8_t>>& bodies = keep ? kept[g] : own;
      std::vector<const uint8_t*> rows(P);
      std::vector<uint32_t> sk(nq);
      static const uint8_t no_rows[8] = {0};      // a partition without a row is still part of the call
      for (size_t gi = 0; gi < groups[g].size(); gi++) {
        std::fill(rows.begin(), rows.end(), nullptr);
        const bool loaded = keep && bodies.size() == groups[g][gi].size();
        if (!loaded) bodies.assign(groups[g][gi].size(), std::vector<uint8_t>());
        for (size_t i = 0; i < groups[g][gi].size(); i++) {
          const uint32_t p = groups[g][gi][i];
          if (!loaded) {
            uint32_t fk = 0, fn = 0;
            bodies[i] = read_matrix(files[p], pa, 4, &fk, &fn);
            if (fk != k || fn != N || bodies[i].size() != n_rows[p] * stride) die("changed while it was read: " + files[p]);
          }
          rows[p] = bodies[i].empty() ? no_rows : bodies[i].data();
        }
        kmx_kquery_task t; memset(&t, 0, sizeof t);
        t.bases = bases.data() + offs[q0]; t.offsets = boffs.data(); t.n_seqs = nq;
        t.kmer_size = k; t.minim_size = msize; t.repart = table.data(); t.nb_parts = (uint32_t)P; t.n_cols = N;
        t.key_words = kw; t.mode = pa ? KMX_MODE_PA : KMX_MODE_COUNT; t.n_rows = n_rows.data(); t.rows = rows.data();
        t.want_sums = want_sums ? 1 : 0;
        t.hits = first ? kmx_kquery_result_hits_dev(first) : nullptr;
        t.sums = first && want_sums ? kmx_kquery_result_sums_dev(first) : nullptr;
        kmx_kquery_result* r = nullptr;
        chk(ctx, kmx_kquery_host(ctx, &t, &r), "kmx_kquery_host");
        chk(ctx, kmx_kquery_result_wait(r), "kmx_kquery");      // (the bodies are reused by the next group)
        if (!first) first = r; else kmx_kquery_result_free(r);
      }
      if (!first) return;      // (more shards than partitions)
      std::vector<uint32_t> sh(nq * N);
      std::vector<uint64_t> ss(want_sums ? nq * N : 0);
      chk(ctx, kmx_kquery_result_copy_hits(first, sh.data(), sh.size()), "kmx_kquery_result_copy_hits");
      if (want_sums) chk(ctx, kmx_kquery_result_copy_sums(first, ss.data(), ss.size()), "kmx_kquery_result_copy_sums");
      chk(ctx, kmx_kquery_result_copy_kmers(first, sk.data(), sk.size()), "kmx_kquery_result_copy_kmers");
      kmx_kquery_result_free(first);
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < sh.size(); i++) hits[i] += sh[i];
      for (size_t i = 0; i < ss.size(); i++) sums[i] += ss[i];
      kmers = sk;      // (every shard walks every query: the same numbers)
    };
    in_shards(G, shard);
    std::string txt;
    for (uint64_t i = 0; i < nq; i++) {
      const std::string& name = names[q0 + i];
      if (o.format != "list") {
        txt += name; txt += '\t'; txt += std::to_string(kmers[i]);
        for (uint32_t c = 0; c < N; c++) { txt += '\t'; txt += want_sums ? std::to_string(sums[i * N + c]) : std::to_string(hits[i * N + c]); }
        txt += '\n';
      } else if (kmers[i] > 0) {
        for (uint32_t c = 0; c < N; c++)
          if ((double)hits[i * N + c] >= o.threshold * (double)kmers[i])
            txt += name + '\t' + samples[c].id + '\t' + std::to_string(hits[i * N + c]) + '\t' + std::to_string(kmers[i]) + '\n';
      }
    }
    if (fwrite(txt.data(), 1, txt.size(), out) != txt.size()) die("write failed: " + (o.out.empty() ? std::string("stdout") : o.out));
  }
  if (out != stdout) { if (fclose(out) != 0) die("write failed: " + o.out); } else fflush(stdout);
  dev.close();
  return 0;
}

}  // namespace

int kmx_query_main(int argc, char** argv)
{
  const QOpt o = parse(argc, argv);
  if (!o.kmer_index.empty()) return kquery_main(o);
  // ---- the index: a run directory of --mode hash:bf:bin or hash:bfc:bin ----
  if (!fs::exists(o.index + "/kmtricks.fof")) die(o.index + " is not a kmtricks runtime directory.");
  std::string opt; { std::ifstream f(o.index + "/options.txt"); if (!f) die("Unable to read at " + o.index + "/options.txt"); std::getline(f, opt); }
  const std::string mode = option_of(opt, "count_format") + ":" + option_of(opt, "mode") + ":" + option_of(opt, "format");
  const bool bfc = mode == "hash:bfc:bin";
  if (mode != "hash:bf:bin" && !bfc) die("kmx query --index needs a run made with --mode hash:bf:bin or hash:bfc:bin; " + o.index + " was made with " + mode + (mode == "kmer:count:bin" || mode == "kmer:pa:bin" ? " (a k-mer run: --kmer-index)" : ""));
  if (o.format == "sums" && !bfc) die("--format sums needs --kmer-index with a run made with --mode kmer:count:bin");
  if (o.min_class >= 0 && !bfc) die("--min-class is for a counting Bloom index: " + o.index + " was made with --mode hash:bf:bin, whose rows hold one bit a sample");
  if (o.z >= 0 && bfc) die("--z is not built for counting Bloom indexes: " + o.index + " was made with --mode hash:bfc:bin");
  uint32_t w = 1;      // bits of a sample's field in a row
  if (bfc) {
    try { w = (uint32_t)std::stoul(option_of(opt, "bwidth")); } catch (...) { die(o.index + "/options.txt names no bwidth"); }
    if (w < 1 || w > 32) die(o.index + "/options.txt: bwidth must be in [1, 32]");
    if (w > 8) die(o.index + " was made with --bitw " + std::to_string(w) + ": kmx query reads counting Bloom indexes of --bitw 1 ... 8 (a class never exceeds 32: --bitw 6 holds every class)");
  }
  const uint32_t min_class = o.min_class < 0 ? 1u : (uint32_t)o.min_class;
  if (bfc && (min_class < 1 || min_class > (1u << w) - 1u)) die("--min-class must be in [1, " + std::to_string((1u << w) - 1u) + "] for an index made with --bitw " + std::to_string(w));
  uint32_t k = 0;
  try { k = (uint32_t)std::stoul(option_of(opt, "kmer_size")); } catch (...) { die(o.index + "/options.txt names no kmer_size"); }
  if (o.z >= (int64_t)k) die("--z must be below the index's k-mer size (" + std::to_string(k) + ")");
  uint64_t W = 0, P = 0; uint32_t msize = 0;
  { std::vector<uint8_t> hi = slurp(o.index + "/hash.info");
    if (hi.size() < 36) die(o.index + "/hash.info: Invalid file format.");
    P = rd<uint64_t>(&hi[8]); W = rd<uint64_t>(&hi[16]); msize = rd<uint32_t>(&hi[32]); }
  uint16_t rp = 0;
  const std::vector<uint16_t> table = read_repartition(o.index + "/repartition_gatb/repartition.minimRepart", &rp);
  if (k < 8 || k > 127 || msize < 4 || msize > 15 || msize >= k || table.size() != ((size_t)1 << (2 * msize)) || P == 0 || P != rp || W == 0)
    die("the index's options.txt, hash.info and repartition table do not fit together");
  for (uint16_t t : table) if (t >= P) die("the index's repartition table names a partition the run does not have");
  const std::vector<Sample> samples = parse_fof(o.index + "/kmtricks.fof", 1);
  const uint32_t N = (uint32_t)samples.size();
  const uint64_t row_bits = (uint64_t)N * w, nb = (row_bits + 7) / 8;      // (w = 1 for a Bloom index: a bit a sample)
  if (row_bits > 0xFFFFFFFFull) die("rows of 2^32 bits and more");
  const uint64_t body = W * nb;
  std::vector<std::string> files(P);
  for (uint64_t p = 0; p < P; p++) {
    files[p] = o.index + "/matrices/matrix_" + std::to_string(p) + ".cmbf";
    std::ifstream f(files[p], std::ios::binary);
    uint8_t h[CMBF_HEADER];
    if (!f || !f.read((char*)h, CMBF_HEADER)) die("Unable to read at " + files[p]);
    if (rd<uint64_t>(&h[0]) != MAGIC_BASE || rd<uint64_t>(&h[13]) != MAGIC_BITMATRIX) die("Invalid file format: " + files[p]);
    if (rd<uint32_t>(&h[21]) != row_bits) die(files[p] + " has rows of " + std::to_string(rd<uint32_t>(&h[21])) + " bits, the index's kmtricks.fof has " + std::to_string(N) + " samples" + (bfc ? " of " + std::to_string(w) + " bits" : ""));
    if (rd<uint64_t>(&h[25]) != W * p || rd<uint64_t>(&h[33]) != W) die(files[p] + ": its window disagrees with the index's hash.info");
    std::error_code ec;
    if (fs::file_size(files[p], ec) != CMBF_HEADER + body || ec) die("truncated matrix (its body is not " + std::to_string(W) + " rows): " + files[p]);
  }

  // ---- the queries ----
  std::string bases; std::vector<uint64_t> offs{0}; std::vector<std::string> names;
  { SeqReader rd(o.query); rd.keep_names(); std::string seq; while (rd.next(seq)) { bases += seq; offs.push_back(bases.size()); names.push_back(rd.name()); } }
  const uint64_t Q = names.size();
  FILE* out = o.out.empty() ? stdout : fopen(o.out.c_str(), "w");
  if (!out) die("Unable to write at " + o.out);

  // ---- devices; how many bases a batch of queries holds and how many partitions a group (kmx_device_memory, or --query-batch-mb) ----
  Devices dev = open_devices(o.gpus, o.batch_mb, 6);
  const uint32_t G = dev.G();
  const uint64_t budget = dev.budget;
  // half for a group's matrices, half for a batch: 17 bytes a base (the bases, 16 of scratch) and a row of the table a query.  A
  // call's scratch and uploads go back to the context's pool when it has been waited for, so the accumulating first result of a
  // batch holds its table and n_kmers only while the later groups run
  const uint64_t group_parts = std::max<uint64_t>(1, (budget / 2) / std::max<uint64_t>(body, 1));
  const uint64_t batch_bytes = std::max<uint64_t>(budget / 2, 1);
  // (--z: and a row of the position-major bits table a base, kept from a batch's first group to its last)
  // (a counting index: two table rows a query, u32 hits and u64 sums)
  const uint64_t per_base = 17 + (o.z >= 0 ? kmx_zquery_bits_bytes(1, N) : 0), per_query = (bfc ? 12ull : 4ull) * N + 12;
  std::vector<uint64_t> cut{0};      // batch b = queries [cut[b], cut[b + 1])
  { uint64_t used = 0;
    for (uint64_t q = 0; q < Q; q++) {
      const uint64_t len = offs[q + 1] - offs[q], cost = per_base * len + per_query;
      if (len > 0xFFFFFFFFull) die("query " + names[q] + " has 2^32 bases or more");
      if (q > cut.back() && (used + cost > batch_bytes || offs[q + 1] - offs[cut.back()] > 0xFFFFFFFFull)) { cut.push_back(q); used = 0; }
      used += cost;
    }
    cut.push_back(Q); if (Q == 0) cut.pop_back(); }
  std::vector<std::vector<std::vector<uint32_t>>> groups(G);      // per shard: its partitions (p mod G) in groups
  size_t n_groups = 0;
  for (uint64_t p = 0; p < P; p++) { auto& gs = groups[p % G]; if (gs.empty() || gs.back().size() >= group_parts) gs.emplace_back(); gs.back().push_back((uint32_t)p); }
  for (auto& gs : groups) n_groups = std::max(n_groups, gs.size());
  if (o.verbose) fprintf(stderr, "[kmx query] %llu queries, %zu bases, k %u, %u samples, %llu partitions of %llu rows: %zu query batches, %zu partition groups a shard, %u shards\n",
                         (unsigned long long)Q, bases.size(), k, N, (unsigned long long)P, (unsigned long long)W, cut.size() - 1, n_groups, G);

  const bool want_sums = o.format == "sums";
  if (o.format != "list") { std::string h = "query\tn_kmers"; for (const Sample& s : samples) { h += '\t'; h += s.id; } h += '\n'; fwrite(h.data(), 1, h.size(), out); }
  // a shard whose partitions fit one group reads its matrices once; a shard with several groups reads every group again for every
  // batch of queries (the index does not fit the device, and is not assumed to fit the host either: DESIGN section 11)
  std::vector<std::vector<std::vector<uint8_t>>> kept(G);
  for (size_t b = 0; b + 1 < cut.size(); b++) {
    const uint64_t q0 = cut[b], nq = cut[b + 1] - q0;
    std::vector<uint64_t> boffs(nq + 1);
    for (uint64_t i = 0; i <= nq; i++) boffs[i] = offs[q0 + i] - offs[q0];
    std::vector<uint32_t> hits(nq * N, 0), kmers(nq, 0);
    std::vector<uint64_t> sums(bfc ? nq * N : 0, 0);
    std::mutex mu;
    // a counting index: the same walk through kmx_cquery_host, the groups adding into the first result's two tables
    auto cshard = [&](uint32_t g) {
      kmx_ctx* ctx = dev.ctxs[g];
      kmx_cquery_result* first = nullptr;
      std::vector<std::vector<uint8_t>> own;
      const bool keep = groups[g].size() == 1;
      std::vector<std::vector<uint8_t>>& bodies = keep ? kept[g] : own;
      std::vector<const uint8_t*> rows(P);
      std::vector<uint32_t> sk(nq);
      for (size_t gi = 0; gi < groups[g].size(); gi++) {
        std::fill(rows.begin(), rows.end(), nullptr);
        const bool loaded = keep && bodies.size() == groups[g][gi].size();
        if (!loaded) bodies.assign(groups[g][gi].size(), std::vector<uint8_t>());
        for (size_t i = 0; i < groups[g][gi].size(); i++) {
          const uint32_t p = groups[g][gi][i];
          if (!loaded) {
            std::ifstream f(files[p], std::ios::binary);
            bodies[i].resize(body);
            if (!f.seekg(CMBF_HEADER) || !f.read((char*)bodies[i].data(), (std::streamsize)body)) die("short read: " + files[p]);
          }
          rows[p] = bodies[i].data();
        }
        kmx_cquery_task t; memset(&t, 0, sizeof t);
        t.bases = bases.data() + offs[q0]; t.offsets = boffs.data(); t.n_seqs = nq;
        t.kmer_size = k; t.minim_size = msize; t.repart = table.data(); t.nb_parts = (uint32_t)P; t.n_cols = N; t.window = W;
        t.rows = rows.data(); t.bitw = w; t.min_class = min_class;
        t.hits = first ? kmx_cquery_result_hits_dev(first) : nullptr;
        t.sums = first ? kmx_cquery_result_sums_dev(first) : nullptr;
        kmx_cquery_result* r = nullptr;
        chk(ctx, kmx_cquery_host(ctx, &t, &r), "kmx_cquery_host");
        chk(ctx, kmx_cquery_result_wait(r), "kmx_cquery");      // (the bodies are reused by the next group)
        if (!first) first = r; else kmx_cquery_result_free(r);
      }
      if (!first) return;      // (more shards than partitions)
      std::vector<uint32_t> sh(nq * N);
      std::vector<uint64_t> ss(nq * N);
      chk(ctx, kmx_cquery_result_copy_hits(first, sh.data(), sh.size()), "kmx_cquery_result_copy_hits");
      chk(ctx, kmx_cquery_result_copy_sums(first, ss.data(), ss.size()), "kmx_cquery_result_copy_sums");
      chk(ctx, kmx_cquery_result_copy_kmers(first, sk.data(), sk.size()), "kmx_cquery_result_copy_kmers");
      kmx_cquery_result_free(first);
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < sh.size(); i++) hits[i] += sh[i];
      for (size_t i = 0; i < ss.size(); i++) sums[i] += ss[i];
      kmers = sk;      // (every shard walks every query: the same numbers)
    };
    // every shard sees all queries of the batch; its groups add up on its device, the shards' tables on the host
    auto shard = [&](uint32_t g) {
      kmx_ctx* ctx = dev.ctxs[g];
      kmx_query_result* first = nullptr;
      std::vector<std::vector<uint8_t>> own;
      const bool keep = groups[g].size() == 1;
      std::vector<std::vector<uint8_t>>& bodies = keep ? kept[g] : own;
      std::vector<const uint8_t*> rows(P);
      std::vector<uint32_t> sk(nq);
      for (size_t gi = 0; gi < groups[g].size(); gi++) {
        std::fill(rows.begin(), rows.end(), nullptr);
        const bool loaded = keep && bodies.size() == groups[g][gi].size();
        if (!loaded) bodies.assign(groups[g][gi].size(), std::vector<uint8_t>());
        for (size_t i = 0; i < groups[g][gi].size(); i++) {
          const uint32_t p = groups[g][gi][i];
          if (!loaded) {
            std::ifstream f(files[p], std::ios::binary);
            bodies[i].resize(body);
            if (!f.seekg(CMBF_HEADER) || !f.read((char*)bodies[i].data(), (std::streamsize)body)) die("short read: " + files[p]);
          }
          rows[p] = bodies[i].data();
        }
        kmx_query_task t; memset(&t, 0, sizeof t);
        t.bases = bases.data() + offs[q0]; t.offsets = boffs.data(); t.n_seqs = nq;
        t.kmer_size = k; t.minim_size = msize; t.repart = table.data(); t.nb_parts = (uint32_t)P; t.n_cols = N; t.window = W;
        t.rows = rows.data(); t.hits = first ? kmx_query_result_hits_dev(first) : nullptr;
        kmx_query_result* r = nullptr;
        chk(ctx, kmx_query_host(ctx, &t, &r), "kmx_query_host");
        chk(ctx, kmx_query_result_wait(r), "kmx_query");      // (the bodies are reused by the next group)
        if (!first) first = r; else kmx_query_result_free(r);
      }
      if (!first) return;      // (more shards than partitions)
      std::vector<uint32_t> sh(nq * N);
      chk(ctx, kmx_query_result_copy_hits(first, sh.data(), sh.size()), "kmx_query_result_copy_hits");
      chk(ctx, kmx_query_result_copy_kmers(first, sk.data(), sk.size()), "kmx_query_result_copy_kmers");
      kmx_query_result_free(first);
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < sh.size(); i++) hits[i] += sh[i];
      kmers = sk;      // (every shard walks every query: the same numbers)
    };
    // --z: one shard; the groups of a batch fill one bits table on the device, the batch's last group runs the window pass.
    // n_kmers are K-positions
    auto zshard = [&](uint32_t) {
      kmx_ctx* ctx = dev.ctxs[0];
      kmx_zquery_result* first = nullptr;
      std::vector<std::vector<uint8_t>> own;
      const bool keep = groups[0].size() == 1;
      std::vector<std::vector<uint8_t>>& bodies = keep ? kept[0] : own;
      std::vector<const uint8_t*> rows(P);
      for (size_t gi = 0; gi < groups[0].size(); gi++) {
        std::fill(rows.begin(), rows.end(), nullptr);
        const bool loaded = keep && bodies.size() == groups[0][gi].size();
        if (!loaded) bodies.assign(groups[0][gi].size(), std::vector<uint8_t>());
        for (size_t i = 0; i < groups[0][gi].size(); i++) {
          const uint32_t p = groups[0][gi][i];
          if (!loaded) {
            std::ifstream f(files[p], std::ios::binary);
            bodies[i].resize(body);
            if (!f.seekg(CMBF_HEADER) || !f.read((char*)bodies[i].data(), (std::streamsize)body)) die("short read: " + files[p]);
          }
          rows[p] = bodies[i].data();
        }
        const bool last = gi + 1 == groups[0].size();
        kmx_zquery_task t; memset(&t, 0, sizeof t);
        t.bases = bases.data() + offs[q0]; t.offsets = boffs.data(); t.n_seqs = nq;
        t.kmer_size = k; t.minim_size = msize; t.repart = table.data(); t.nb_parts = (uint32_t)P; t.n_cols = N; t.window = W;
        t.rows = rows.data(); t.z = (uint32_t)o.z; t.last = last ? 1 : 0;
        t.bits = first ? kmx_zquery_result_bits_dev(first) : nullptr;
        kmx_zquery_result* r = nullptr;
        chk(ctx, kmx_zquery_host(ctx, &t, &r), "kmx_zquery_host");
        chk(ctx, kmx_zquery_result_wait(r), "kmx_zquery");      // (the bodies are reused by the next group)
        if (last) {
          chk(ctx, kmx_zquery_result_copy_hits(r, hits.data(), hits.size()), "kmx_zquery_result_copy_hits");
          chk(ctx, kmx_zquery_result_copy_kmers(r, kmers.data(), kmers.size()), "kmx_zquery_result_copy_kmers");
        }
        if (!first) first = r; else kmx_zquery_result_free(r);      // (the first result owns the table)
      }
      kmx_zquery_result_free(first);
    };
    if (o.z >= 0) in_shards(1, zshard);
    else if (bfc) in_shards(G, cshard);
    else in_shards(G, shard);
    std::string txt;
    for (uint64_t i = 0; i < nq; i++) {
      const std::string& name = names[q0 + i];
      if (o.format != "list") {
        txt += name; txt += '\t'; txt += std::to_string(kmers[i]);
        for (uint32_t c = 0; c < N; c++) { txt += '\t'; txt += want_sums ? std::to_string(sums[i * N + c]) : std::to_string(hits[i * N + c]); }
        txt += '\n';
      } else if (kmers[i] > 0) {
        for (uint32_t c = 0; c < N; c++)
          if ((double)hits[i * N + c] >= o.threshold * (double)kmers[i])
            txt += name + '\t' + samples[c].id + '\t' + std::to_string(hits[i * N + c]) + '\t' + std::to_string(kmers[i]) + '\n';
      }
    }
    if (fwrite(txt.data(), 1, txt.size(), out) != txt.size()) die("write failed: " + (o.out.empty() ? std::string("stdout") : o.out));
  }
  if (out != stdout) { if (fclose(out) != 0) die("write failed: " + o.out); } else fflush(stdout);
  dev.close();
  return 0;
}
