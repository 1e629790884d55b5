"""kmx_zquery_dev on device-resident indexes, at z = 0 and z = 3, on bench_query.py's two shapes: BASELINE configs[1]'s Bloom shape
(N = 100 samples, W = 3 125 056 rows a partition, P = 32) and the same windows at N = 2500; queries: 10^5 reads of 150 bp, and one 2-Mbp
contig.  k = 31, m = 10, a quarter of the matrices' bits set.  Per case: the kernels' time (median of the timed calls after warm-up,
HIP events through kmx_set_profiling), the algorithmic bytes, and -- timed in the same process on the same device-resident inputs --
the yardstick: kmx_query_dev, the plain query, whose code this path leaves as it was.  The ratio says what the position-major table
costs: the new path writes and reads back `pitch` bytes a k-mer on top of what the plain query moves.
Before a case is recorded its result is checked against tests/zquery_ref.py's numpy road on a subsample: the first reads of the batch,
or the contig's first bases sent as a query of their own (a single query's table has no part that could be checked alone), with the
rows fetched from the device index at the addresses numpy works out.  Needs the GPU (no fallback).
Usage: bench_zquery.py [--n 100,2500] [--z 0,3] [--reads 100000] [--contig 2000000] [--steps K] [--warmup W] [--out profiles/zquery_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import orc
import zquery_ref as zr

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="100,2500")
ap.add_argument("--z", default="0,3")
ap.add_argument("--reads", type=int, default=100000)
ap.add_argument("--contig", type=int, default=2000000)
ap.add_argument("--window", type=int, default=3125056)
ap.add_argument("--parts", type=int, default=32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sample-reads", type=int, default=64)
ap.add_argument("--sample-bases", type=int, default=20000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zquery_bench.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_zquery.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
K, M, W, P, RL = 31, 10, a.window, a.parts, 150


def main():
    ctx = lib.Context(0); ctx.set_profiling(True)
    lut, rep = orc.minimizer_lut(M), orc.repart_static(M, P)
    d_rep = torch.from_numpy(rep.view(np.int16)).to(dev)
    rng = np.random.default_rng(1)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    queries = {}
    for name, (cnt, ln, sub_cnt, sub_len) in {"reads": (a.reads, RL, min(a.sample_reads, a.reads), RL), "contig": (1, a.contig, 1, min(a.sample_bases, a.contig))}.items():
        blob = alpha[rng.integers(0, 4, cnt * ln)].tobytes()
        offs = (np.arange(cnt + 1, dtype=np.uint64) * np.uint64(ln))
        sub = [blob[i * ln:i * ln + sub_len].decode() for i in range(sub_cnt)]      # the subsample: queries of their own
        sub_blob, sub_offs = lib.Context.pack_reads(sub)
        queries[name] = dict(n_seqs=cnt, bases=len(blob), whole_queries=sub_len == ln, sub=sub, addr=zr.addresses_np(sub, K, M, rep, W, lut),
                             d_b=torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev), d_o=torch.from_numpy(offs.view(np.int64)).to(dev),
                             d_sb=torch.frombuffer(bytearray(sub_blob), dtype=torch.uint8).to(dev), d_so=torch.from_numpy(sub_offs.view(np.int64)).to(dev))
    out = []
    for N in [int(x) for x in a.n.split(",")]:
        nb = (N + 7) // 8
        body = W * nb
        index = torch.empty(P * body + 256, dtype=torch.uint8, device=dev)
        for o in range(0, len(index), 1 << 30):      # a quarter of the bits set
            e = min(o + (1 << 30), len(index))
            index[o:e] = torch.randint(0, 256, (e - o,), dtype=torch.uint8, device=dev) & torch.randint(0, 256, (e - o,), dtype=torch.uint8, device=dev)
        base = index.data_ptr() + 128
        rows_dev = [base + p * body for p in range(P)]
        for name, Q in queries.items():
            # the rows of the subsample's k-mers, fetched from the device index at numpy's addresses
            A = Q["addr"]
            sel = np.nonzero(A["ok"])[0]
            rowbytes = np.zeros((len(A["ok"]), nb), np.uint8)
            at = A["part"][sel] * body + A["row"][sel] * nb + 128
            for c0 in range(0, len(sel), 4096):
                idx = torch.from_numpy(at[c0:c0 + 4096, None] + np.arange(nb)[None, :]).to(dev)
                rowbytes[sel[c0:c0 + 4096]] = index[idx].cpu().numpy()
            torch.cuda.synchronize()
            args = (Q["d_b"].data_ptr(), Q["d_o"].data_ptr(), Q["n_seqs"], K, M, d_rep.data_ptr(), W, N, rows_dev)
            sub_args = (Q["d_sb"].data_ptr(), Q["d_so"].data_ptr(), len(Q["sub"]), K, M, d_rep.data_ptr(), W, N, rows_dev)
            ys = []
            for i in range(a.warmup + a.steps):      # the yardstick: the plain query on the same inputs
                r = ctx.query_dev(*args, keep=True)
                r.wait()
                if i >= a.warmup: ys.append(r.kernel_ms())
                if i == a.warmup + a.steps - 1: y_bytes = int(r.algo_bytes())
                r.free()
            y_ms = statistics.median(ys)
            for z in [int(x) for x in a.z.split(",")]:
                en, eh = zr.windows_np(A, rowbytes, K, z, N)
                got = ctx.zquery_dev(*sub_args, z)
                assert np.array_equal(got.n_kmers, en) and np.array_equal(got.hits, eh), f"N={N} {name} z={z}: the subsample differs from the numpy road"
                ms, res = [], None
                for i in range(a.warmup + a.steps):
                    r = ctx.zquery_dev(*args, z, keep=True)
                    r.wait()
                    if i >= a.warmup: ms.append(r.kernel_ms())
                    if i == a.warmup + a.steps - 1:
                        o = r.output()
                        res = dict(n_kpositions=int(o.n_kmers.sum(dtype=np.uint64)), algo_bytes=int(o.algo_bytes))
                        assert res["n_kpositions"] == Q["n_seqs"] * (Q["bases"] // Q["n_seqs"] - K - z + 1)      # (ACGT only)
                        if Q["whole_queries"]:      # the subsample's queries are the batch's first ones
                            assert np.array_equal(o.n_kmers[:len(en)], en) and np.array_equal(o.hits[:len(en)], eh), f"N={N} {name} z={z}: the batch's first queries differ"
                    r.free()
                k_ms = statistics.median(ms)
                res.update(case=f"N={N} {name} z={z}", n_cols=N, z=z, window=W, parts=P, k=K, m=M, queries=Q["n_seqs"], bases=Q["bases"],
                           index_bytes=P * body, kernel_ms=round(k_ms, 4), kernel_ms_min=round(min(ms), 4), kernel_ms_max=round(max(ms), 4),
                           query_ms=round(y_ms, 4), query_algo_bytes=y_bytes, zquery_over_query=round(k_ms / y_ms, 2),
                           algo_bytes_over_query=round(res["algo_bytes"] / y_bytes, 2), algo_gb_s=round(res["algo_bytes"] / k_ms / 1e6, 1),
                           steps=a.steps, warmup=a.warmup)
                print(json.dumps(res), flush=True)
                out.append(res)
        del index
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)
            f.write("\n")


main()
