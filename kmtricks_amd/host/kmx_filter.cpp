// kmx_filter.cpp -- `kmx filter`: an existing k-mer matrix queried with one new sample (kmtricks filter: src/cli.cpp:777-857,
// main_filter include/kmtricks/cmd.hpp:609-724, km::FilterTask / km::MatrixFilter include/kmtricks/matrix.hpp:23-393).
// The key sample is split and counted on the GPU (kmx_count_reads_dev) and stays there; every partition's matrix goes through
// kmx_filter_host in runs of whole rows.  Every check that needs no GPU comes before kmx_create.
#include <kmx.h>
#include <algorithm>
#include <cstring>
#include <future>
#include <set>
#include <thread>
#include "kmx_io.hpp"
#include "kmx_run.hpp"

namespace fs = std::filesystem;
using namespace kmxio;

namespace {

struct FOpt {
  std::string in, key, out;
  uint32_t hard_min = 2, threads = 8, gpus = 1, count_bytes = 4;
  uint64_t batch_mb = 256;
  bool k = false, m = true, v = true, cpr_in = false, cpr_out = false, verbose = false;
};

const char* USAGE = "usage: kmx filter --in-matrix <run dir> --key <fof with one sample> --output <dir> [--hard-min INT] [--out-types k,m,v] [--cpr-in] [--cpr-out] "
                    "[-t INT (accepted, no effect)] [-v] [--gpus INT] [--filter-batch-mb INT] [--count-bytes 1|2|4]";

FOpt parse(int argc, char** argv)
{
  FOpt o;
  auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("missing value for ") + argv[i] + "\n" + USAGE); return argv[++i]; };
  auto num = [&](int& i) -> unsigned long { const std::string v = need(i); try { size_t n = 0; const unsigned long x = std::stoul(v, &n); if (n != v.size()) throw 1; return x; } catch (...) { die(std::string("bad number for ") + argv[i - 1] + ": " + v); } };
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--in-matrix") o.in = need(i);
    else if (a == "--key") o.key = need(i);
    else if (a == "--output") o.out = need(i);
    else if (a == "--hard-min") o.hard_min = num(i);
    else if (a == "--out-types") {
      o.k = o.m = o.v = false;
      std::stringstream ss(need(i)); std::string t; bool any = false;
      while (std::getline(ss, t, ',')) {
        if (t == "k") o.k = true; else if (t == "m") o.m = true; else if (t == "v") o.v = true;
        else die("--out-types: '" + t + "' is none of k, m, v");
        any = true;
      }
      if (!any) die("--out-types: nothing asked for (k, m, v)");
    }
    else if (a == "--cpr-in") o.cpr_in = true;
    else if (a == "--cpr-out") o.cpr_out = true;
    else if (a == "-t" || a == "--threads") o.threads = num(i);      // (taken as the reference takes it; the host work is a thread per shard plus its reader and writer)
    else if (a == "-v" || a == "--verbose") { o.verbose = true; if (i + 1 < argc && argv[i + 1][0] != '-') i++; }      // (the reference's takes a level)
    else if (a == "--gpus") o.gpus = num(i);
    else if (a == "--filter-batch-mb") o.batch_mb = num(i);
    else if (a == "--count-bytes") { o.count_bytes = num(i); if (o.count_bytes != 1 && o.count_bytes != 2 && o.count_bytes != 4) die("--count-bytes must be 1, 2 or 4"); }
    else die("unknown option " + a + "\n" + USAGE);
  }
  if (o.in.empty()) die(std::string("--in-matrix is required\n") + USAGE);
  if (o.key.empty()) die(std::string("--key is required\n") + USAGE);
  if (o.out.empty()) die(std::string("--output is required\n") + USAGE);
  if (o.batch_mb == 0) o.batch_mb = 1;
  if (o.gpus == 0) o.gpus = 1;
  if (o.gpus > 16) o.gpus = 16;
  return o;
}

struct Part { uint32_t id; bool pa; std::string path; };

void chk(kmx_ctx* c, int rc, const char* what) { if (rc != KMX_OK) die(std::string(what) + ": " + kmx_last_error(c)); }

}  // namespace

int kmx_filter_main(int argc, char** argv)
{
  const FOpt o = parse(argc, argv);
  // ---- the partitions that have a k-mer matrix (cmd.hpp:630-647; hash matrices are not looked for) ----
  std::vector<Part> parts;
  {
    const std::string md = o.in + "/matrices";
    std::error_code ec;
    for (auto it = fs::directory_iterator(md, ec); !ec && it != fs::directory_iterator(); it.increment(ec)) {
      std::string n = it->path().filename().string();
      if (n.rfind("matrix_", 0) != 0) continue;
      const bool lz = n.size() > 4 && n.substr(n.size() - 4) == ".lz4";
      if (lz != o.cpr_in) continue;
      if (lz) n.resize(n.size() - 4);
      const size_t dot = n.find('.');
      if (dot == std::string::npos) continue;
      const std::string ext = n.substr(dot), id = n.substr(7, dot - 7);
      if ((ext != ".pa" && ext != ".count") || id.empty() || id.find_first_not_of("0123456789") != std::string::npos) continue;
      parts.push_back({(uint32_t)std::stoul(id), ext == ".pa", it->path().string()});
    }
    std::sort(parts.begin(), parts.end(), [](const Part& a, const Part& b) { return a.id < b.id; });
  }
  if (parts.empty()) die("No files found for these parameters");
  const std::vector<Sample> samples = parse_fof(o.key, o.hard_min);
  if (samples.size() > 1) die("Filtering with many samples is not yet implemented. Fof must contain only one sample.");      // cmd.hpp:654-655
  const Sample& smp = samples[0];      // (a minimum in the fof line wins over --hard-min, cmd.hpp:672-673)
  if (fs::is_directory(o.out)) die("Directory already exists!");
  GatbConfig gc;
  if (!GatbConfig::load(o.in + "/config_gatb/gatb.config", gc)) die("Unable to read at " + o.in + "/config_gatb/gatb.config");
  uint16_t nb_parts = 0;
  const std::vector<uint16_t> table = read_repartition(o.in + "/repartition_gatb/repartition.minimRepart", &nb_parts);
  const uint32_t k = (uint32_t)gc.kmer_size, msize = (uint32_t)gc.minim_size, kw = (k + 31) / 32, P = nb_parts;
  if (k < 8 || k > 127 || msize < 4 || msize > 15 || table.size() != ((size_t)1 << (2 * msize))) die("the input run's gatb.config / repartition table do not fit together");
  for (const Part& p : parts) if (p.id >= P) die("matrix of partition " + std::to_string(p.id) + " but the run has " + std::to_string(P) + " partitions");

  // ---- the output run directory (cmd.hpp:651-658) ----
  const std::string root = fs::absolute(o.out).string();
  make_run_layout(root);
  fs::copy_file(o.key, root + "/kmtricks.fof");
  fs::copy(o.in + "/config_gatb", root + "/config_gatb", fs::copy_options::recursive | fs::copy_options::overwrite_existing);
  fs::copy(o.in + "/repartition_gatb", root + "/repartition_gatb", fs::copy_options::recursive | fs::copy_options::overwrite_existing);
  if (o.k) for (const Part& p : parts) fs::create_directories(root + "/counts/partition_" + std::to_string(p.id));

  // ---- the key sample: reads -> counts, left in HBM.  --gpus G as in `kmx pipeline`: G shards, a context and a store each, partition p
  //      belongs to shard p mod G (beyond the devices present the shards share them) ----
  if (kmx_version() != KMX_VERSION) die("libkmx.so is not the version this driver was built for");
  const uint32_t G = o.gpus, ndev = (uint32_t)std::max(1, kmx_device_count());
  std::vector<kmx_ctx*> ctxs(G, nullptr); std::vector<kmx_store*> stores(G, nullptr);
  for (uint32_t g = 0; g < G; g++) {
    if (kmx_create((int)(g % ndev), &ctxs[g]) != KMX_OK) die(std::string("kmx_create: ") + kmx_last_error(nullptr));
    if (kmx_store_create((int)(g % ndev), 0, &stores[g]) != KMX_OK) die("kmx_store_create failed");
  }
  std::vector<kmx_list> lists(P);
  {
    std::string bases, seq; std::vector<uint64_t> offs{0};
    for (const std::string& f : smp.files) { SeqReader rd(f); while (rd.next(seq)) { bases += seq; offs.push_back(bases.size()); } }
    // the split needs the run's whole table, so every partition's list is counted (list p goes to shard p mod G's store); those
    // of partitions without a matrix are never read
    std::vector<uint64_t> kmers(P);
    chk(ctxs[0], kmx_count_reads_dev(ctxs[0], bases.data(), offs.data(), offs.size() - 1, k, msize, table.data(), P, 0, 0, smp.hard_min, stores.data(), G, lists.data(),
                                     kmers.data(), nullptr, nullptr, nullptr, nullptr, nullptr), "kmx_count_reads_dev");
    if (o.verbose) fprintf(stderr, "[kmx filter] %s: %zu reads, %zu bases, hard-min %u\n", smp.id.c_str(), offs.size() - 1, bases.size(), smp.hard_min);
  }

  // ---- a host thread per shard, partition by partition: read (the next file while this one is filtered), filter in runs of rows
  //      (a run goes to the device from one of two page-locked buffers while the run before it is filtered and copied back), write
  //      (a run while the next is filtered) ----
  const uint32_t want_mv = (o.m ? KMX_FILTER_M : 0u) | (o.v ? KMX_FILTER_V : 0u);
  auto shard = [&](uint32_t g) {
  try {
  kmx_ctx* ctx = ctxs[g];
  std::vector<size_t> mine;
  for (size_t i = 0; i < parts.size(); i++) if (parts[i].id % G == g) mine.push_back(i);
  if (mine.empty()) return;
  auto load = [&](size_t i) { return std::async(std::launch::async, [&, i] { uint32_t fk = 0, n = 0; std::vector<uint8_t> b = read_matrix(parts[i].path, parts[i].pa, o.count_bytes, &fk, &n); return std::make_tuple(std::move(b), fk, n); }); };
  auto next_file = load(mine[0]);
  uint8_t* stage[2] = {nullptr, nullptr}; uint64_t stage_bytes = 0;
  for (size_t mi = 0; mi < mine.size(); mi++) {
    const Part& pt = parts[mine[mi]];
    auto got = next_file.get();
    if (mi + 1 < mine.size()) next_file = load(mine[mi + 1]);
    const std::vector<uint8_t>& body = std::get<0>(got);
    const uint32_t fk = std::get<1>(got), N = std::get<2>(got);
    if (fk != k) die("matrix " + pt.path + " was made with k = " + std::to_string(fk) + ", the run's gatb.config says " + std::to_string(k));
    const uint64_t irb = (uint64_t)kw * 8 + (pt.pa ? (N + 7) / 8 : (uint64_t)N * 4), orb = irb + (pt.pa ? 0 : 4);
    const uint64_t n_rows = body.size() / irb, run_rows = std::max<uint64_t>(1, std::min<uint64_t>((o.batch_mb << 20) / irb, 0xFFFFFF00ull));
    const kmx_list key = lists[pt.id];
    const std::string ps = std::to_string(pt.id);
    std::unique_ptr<Out> mo, vo;
    if (o.m) {
      mo.reset(new Out(root + "/matrices/matrix_" + ps + (pt.pa ? ".pa" : ".count") + (o.cpr_out ? ".lz4" : "")));
      if (pt.pa) matrix_pa_header(*mo, k, N, pt.id, o.cpr_out); else matrix_count_header(*mo, k, N + 1, pt.id, o.cpr_out);
    }
    if (o.v) vo.reset(new Out(root + "/matrices/" + ps + ".vec"));
    const uint64_t need = std::min<uint64_t>(run_rows, n_rows) * irb;
    if (need > stage_bytes) {
      for (uint8_t*& b : stage) { if (b) kmx_free_pinned(b); if (!(b = (uint8_t*)kmx_alloc_pinned(need))) die("kmx_alloc_pinned failed"); }
      stage_bytes = need;
    }
    uint8_t* marks = kmx_filter_marks_alloc(ctx, key.n);
    if (!marks) die(std::string("kmx_filter_marks_alloc: ") + kmx_last_error(ctx));
    // a run's results come to the host on this thread and are written on another while the next run is filtered
    std::future<void> writing;
    auto submit = [&](uint64_t r0, bool last) -> kmx_filter_result* {
      kmx_filter_task t; memset(&t, 0, sizeof t);
      t.key_words = kw; t.mode = pt.pa ? KMX_MODE_PA : KMX_MODE_COUNT; t.n_cols = N;
      t.want = want_mv | (last && o.k ? KMX_FILTER_K : 0u);
      if (!t.want) t.want = KMX_FILTER_V;      // (only k asked for: the runs before the last still leave their marks)
      t.n_rows = std::min(run_rows, n_rows - r0);
      // (run r's buffer held run r - 2, which has been waited for)
      uint8_t* buf = stage[(r0 / run_rows) & 1];
      if (t.n_rows) memcpy(buf, body.data() + r0 * irb, t.n_rows * irb);
      t.rows = t.n_rows ? buf : nullptr;
      t.key = key; t.marks = marks; t.key_on_device = 1;
      kmx_filter_result* r = nullptr;
      chk(ctx, kmx_filter_host(ctx, &t, &r), "kmx_filter_host");
      return r;
    };
    const uint64_t n_runs = std::max<uint64_t>(1, (n_rows + run_rows - 1) / run_rows);
    kmx_filter_result* cur = submit(0, n_runs == 1);
    for (uint64_t run = 0; run < n_runs; run++) {
      chk(ctx, kmx_filter_result_wait(cur), "kmx_filter");
      kmx_filter_result* nxt = run + 1 < n_runs ? submit((run + 1) * run_rows, run + 2 == n_runs) : nullptr;
      auto mb = std::make_shared<std::vector<uint8_t>>(o.m ? kmx_filter_result_body_bytes(cur) : 0);
      auto vb = std::make_shared<std::vector<uint32_t>>(o.v ? kmx_filter_result_vector_len(cur) : 0);
      // (a run before the last of a k-only job asks for v so that it leaves its marks: that vector stays on the device)
      if (o.m) chk(ctx, kmx_filter_result_copy_body(cur, mb->data(), mb->size()), "kmx_filter_result_copy_body");
      if (o.v) chk(ctx, kmx_filter_result_copy_vector(cur, vb->data(), vb->size()), "kmx_filter_result_copy_vector");
      if (run + 1 == n_runs && o.k) {
        const uint64_t na = kmx_filter_result_absent(cur), rb = kw * 8 + 4;
        std::vector<uint8_t> rec(na * rb);
        chk(ctx, kmx_filter_result_copy_absent(cur, rec.data(), rec.size()), "kmx_filter_result_copy_absent");
        std::vector<uint64_t> keys(na * kw); std::vector<uint32_t> counts(na);
        for (uint64_t i = 0; i < na; i++) { memcpy(&keys[i * kw], &rec[i * rb], kw * 8); memcpy(&counts[i], &rec[i * rb + kw * 8], 4); }
        write_kmer_file(root + "/counts/partition_" + ps + "/" + smp.id + ".kmer" + (o.cpr_out ? ".lz4" : ""), k, 0, pt.id, keys.data(), counts.data(), na, o.cpr_out);
      }
      if (o.verbose) fprintf(stderr, "[kmx filter] partition %u run %llu/%llu: %llu of %llu rows kept\n", pt.id, (unsigned long long)run + 1, (unsigned long long)n_runs,
                             (unsigned long long)kmx_filter_result_rows(cur), (unsigned long long)std::min(run_rows, n_rows - run * run_rows));
      kmx_filter_result_free(cur);
      cur = nxt;
      if (writing.valid()) writing.get();
      Out* mp = mo.get(); Out* vp = vo.get();
      const uint32_t cb = pt.pa ? 4 : o.count_bytes; const uint64_t kb = (uint64_t)kw * 8;
      writing = std::async(std::launch::async, [mb, vb, mp, vp, cb, kb, orb, N] {
        if (mp && cb == 4) mp->raw(mb->data(), mb->size());
        else if (mp) {      // counts go back to the width the matrix came with (saturated)
          const uint64_t rows = mb->size() / orb, rout = kb + (uint64_t)(N + 1) * cb, mx = cb == 1 ? 0xFFu : 0xFFFFu;
          std::vector<uint8_t> nar(rows * rout);
          for (uint64_t r = 0; r < rows; r++) {
            memcpy(&nar[r * rout], &(*mb)[r * orb], kb);
            for (uint32_t c = 0; c <= N; c++) { uint32_t x; memcpy(&x, &(*mb)[r * orb + kb + (uint64_t)c * 4], 4); x = std::min<uint32_t>(x, mx); memcpy(&nar[r * rout + kb + (uint64_t)c * cb], &x, cb); }
          }
          mp->raw(nar.data(), nar.size());
        }
        if (vp) { std::string txt; txt.reserve(vb->size() * 3); for (uint32_t x : *vb) { txt += std::to_string(x); txt += '\n'; } vp->raw(txt.data(), txt.size()); }
      });
    }
    if (writing.valid()) writing.get();
    if (mo) mo->close();
    if (vo) vo->close();
    kmx_filter_marks_free(ctx, marks);
  }
  for (uint8_t* b : stage) if (b) kmx_free_pinned(b);
  } catch (const std::exception& e) { die(e.what()); }
  };
  std::vector<std::thread> workers;
  for (uint32_t g = 1; g < G; g++) workers.emplace_back(shard, g);
  shard(0);
  for (std::thread& w : workers) w.join();
  for (uint32_t g = 0; g < G; g++) { kmx_store_destroy(stores[g]); kmx_destroy(ctxs[g]); }
  return 0;
}
