"""kmx_cquery_dev on device-resident counting Bloom indexes: BASELINE configs[1]'s shape (N = 100 samples, W = 3 125 056 rows a
partition, P = 32) with fields of w = 2 and w = 4 bits, and the same windows at N = 2500; queries: 10^5 reads of 150 bp, and one 2-Mbp
contig.  k = 31, m = 10, random bodies.  Per case: the kernels' time (median of the timed calls after warm-up, HIP events through
kmx_set_profiling), the algorithmic bytes, and -- timed in the same process -- the yardstick: a kernel, compiled from the source below,
that loads the 128-byte lines covering each of the same rows, in the order the gather visits them, and does nothing else.  The
addresses are worked out here with numpy (canonical k-mer, XXH64, window minimum of the m-mer values), not taken from the library;
their number must equal the call's n_kmers and, where the first query is a read, its hits and sums are recomputed from them.  Needs
the GPU and hipcc (no fallback).
Usage: bench_cquery.py [--shapes 100:2,100:4,2500:2,2500:4] [--reads 100000] [--contig 2000000] [--steps K] [--warmup W]
                       [--out profiles/cquery_bench.json]"""
import argparse, ctypes, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import orc
import cquery_ref as cr

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="100:2,100:4,2500:2,2500:4")      # N:w
ap.add_argument("--reads", type=int, default=100000)
ap.add_argument("--contig", type=int, default=2000000)
ap.add_argument("--window", type=int, default=3125056)
ap.add_argument("--parts", type=int, default=32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cquery_bench.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_cquery.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
K, M, W, P, RL = 31, 10, a.window, a.parts, 150

YARDSTICK = r"""
#include <hip/hip_runtime.h>
// eight lanes a record: the 128-byte lines that cover the nb bytes at `addr`, 16 bytes a lane and line
__global__ __launch_bounds__(256) void k_lines(const unsigned long long* __restrict__ addr, unsigned long long n, unsigned nb, unsigned* __restrict__ sink)
{
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned acc = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n * 8; i += stride) {
    const unsigned long long a0 = addr[i >> 3], first = a0 & ~127ull, last = (a0 + nb - 1) & ~127ull;
    for (unsigned long long line = first; line <= last; line += 128) {
      const uint4 v = *reinterpret_cast<const uint4*>(line + 16 * (i & 7));
      acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
  }
  if (acc == 0x9E3779B9u) sink[0] = acc;      // (keeps the loads alive)
}
extern "C" float run_lines(const unsigned long long* addr, unsigned long long n, unsigned nb, unsigned* sink, int n_cu)
{
  hipEvent_t e0, e1; float ms = -1.f;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
  const unsigned long long blocks = (n * 8 + 255) / 256;
  const unsigned grid = (unsigned)(blocks < (unsigned long long)n_cu * 8 ? (blocks ? blocks : 1) : (unsigned long long)n_cu * 8);
  hipEventRecord(e0, 0);
  hipLaunchKernelGGL(k_lines, dim3(grid), dim3(256), 0, 0, addr, n, nb, sink);
  hipEventRecord(e1, 0);
  if (hipEventSynchronize(e1) == hipSuccess) hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return ms;
}
"""


def build_yardstick():
    d = tempfile.mkdtemp(prefix="kmx_cquery_bench_")
    src, so = os.path.join(d, "lines.hip"), os.path.join(d, "liblines.so")
    open(src, "w").write(YARDSTICK)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", so])
    so_lib = ctypes.CDLL(so)
    so_lib.run_lines.restype = ctypes.c_float
    so_lib.run_lines.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]
    return so_lib


def addresses(blob, starts, lens, lut, rep):
    """(partition, row, query) of every k-mer of ACGT-only sequences, in position order: the definition in numpy (bench_query.py's)"""
    codes = ((np.frombuffer(blob, np.uint8) >> 1) & 3).astype(np.uint64)
    L = len(codes)
    n = L - K + 1
    with np.errstate(over="ignore"):
        fwd, rev = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        for i in range(K):
            fwd = (fwd << np.uint64(2)) | codes[i:i + n]
            rev |= (codes[i:i + n] ^ np.uint64(2)) << np.uint64(2 * i)
        c = np.minimum(fwd, rev)
        del fwd, rev
        X1, X2, X3, X4, X5 = (np.uint64(x) for x in (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5))
        rotl = lambda x, r: (x << np.uint64(r)) | (x >> np.uint64(64 - r))
        h = (X5 + np.uint64(8)) ^ (rotl(c * X2, 31) * X1)
        h = rotl(h, 27) * X1 + X4
        h ^= h >> np.uint64(33); h *= X2; h ^= h >> np.uint64(29); h *= X3; h ^= h >> np.uint64(32)
        row = h % np.uint64(W)
        nm = L - M + 1
        mm = np.zeros(nm, np.uint64)
        for i in range(M):
            mm = (mm << np.uint64(2)) | codes[i:i + nm]
    val = lut[mm.astype(np.int64)]
    mini = val[:n].copy()
    for i in range(1, K - M + 1):
        np.minimum(mini, val[i:i + n], out=mini)
    part = rep[mini.astype(np.int64)].astype(np.int64)
    q = np.repeat(np.arange(len(lens)), lens)[:n]
    pos = np.arange(n) - np.repeat(starts, lens)[:n]
    ok = pos + K <= np.repeat(lens, lens)[:n]
    return part[ok], row[ok].astype(np.int64), q[ok]


def main():
    ctx = lib.Context(0); ctx.set_profiling(True)
    yard = build_yardstick()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lut, rep = orc.minimizer_lut(M), orc.repart_static(M, P)
    d_rep = torch.from_numpy(rep.view(np.int16)).to(dev)
    rng = np.random.default_rng(1)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    shapes = {"reads": (a.reads, RL), "contig": (1, a.contig)}
    queries = {}
    for name, (cnt, ln) in shapes.items():
        blob = alpha[rng.integers(0, 4, cnt * ln)].tobytes()
        lens = np.full(cnt, ln, np.int64)
        starts = np.arange(cnt, dtype=np.int64) * ln
        part, row, q = addresses(blob, starts, lens, lut, rep)
        order = np.argsort(part, kind="stable")      # the gather's order: by partition, position order inside
        offs = np.concatenate([starts, [cnt * ln]]).astype(np.uint64)
        queries[name] = dict(n_seqs=cnt, bases=len(blob), part=part[order], row=row[order], q=q[order],
                             d_b=torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev), d_o=torch.from_numpy(offs.view(np.int64)).to(dev))
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    out = []
    for N, w in [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]:
        nb = (N * w + 7) // 8
        body = W * nb
        index = torch.empty(P * body + 256, dtype=torch.uint8, device=dev)
        for o in range(0, len(index), 1 << 30):      # every class alike: random bytes
            e = min(o + (1 << 30), len(index))
            index[o:e] = torch.randint(0, 256, (e - o,), dtype=torch.uint8, device=dev)
        base = index.data_ptr() + 128
        rows_dev = [base + p * body for p in range(P)]
        for name, Q in queries.items():
            torch.cuda.synchronize()
            ms, res = [], None
            for i in range(a.warmup + a.steps):
                r = ctx.cquery_dev(Q["d_b"].data_ptr(), Q["d_o"].data_ptr(), Q["n_seqs"], K, M, d_rep.data_ptr(), W, N, rows_dev, w, min_class=1, keep=True)
                r.wait()
                if i >= a.warmup: ms.append(r.kernel_ms())
                if i == a.warmup + a.steps - 1:
                    o = r.output()
                    res = dict(n_kmers=int(o.n_kmers.sum(dtype=np.uint64)), algo_bytes=int(o.algo_bytes), hits0=o.hits[0].copy(), sums0=o.sums[0].copy())
                r.free()
            # the same row addresses, from numpy: as many as the call counted, and the first query's tables recomputed from them
            assert res["n_kmers"] == len(Q["row"]), (res["n_kmers"], len(Q["row"]))
            sel = Q["q"] == 0
            hits0, sums0 = res.pop("hits0"), res.pop("sums0")
            if sel.sum() <= 10000:      # (the contig's one query is too long to redo on the host: its addresses are the reads' function)
                a0 = Q["part"][sel] * body + Q["row"][sel] * nb
                idx = torch.from_numpy(a0[:, None] + np.arange(nb)[None, :]).to(dev) + 128
                v = cr.unpack_classes(index[idx].cpu().numpy(), N, w)
                fl = np.where(v == 0, np.uint64(0), np.uint64(1) << (np.maximum(np.minimum(v, 32), 1).astype(np.uint64) - np.uint64(1)))
                assert np.array_equal((v >= 1).sum(axis=0).astype(np.uint32), hits0), "the numpy addresses are not the library's"
                assert np.array_equal(fl.sum(axis=0, dtype=np.uint64), sums0), "the numpy addresses are not the library's"
                del idx
            addr = np.uint64(base) + (Q["part"] * body + Q["row"] * nb).astype(np.uint64)
            d_addr = torch.from_numpy(addr.view(np.int64)).to(dev)
            torch.cuda.synchronize()
            ys = []
            for i in range(a.warmup + a.steps):
                t = yard.run_lines(d_addr.data_ptr(), len(addr), nb, sink.data_ptr(), n_cu)
                if i >= a.warmup: ys.append(float(t))
            assert min(ys) > 0, "the yardstick kernel did not run"
            k_ms, y_ms = statistics.median(ms), statistics.median(ys)
            res.update(case=f"N={N} w={w} {name}", n_cols=N, bitw=w, row_bytes=nb, window=W, parts=P, k=K, m=M, queries=Q["n_seqs"], bases=Q["bases"],
                       index_bytes=P * body, kernel_ms=round(k_ms, 4), kernel_ms_min=round(min(ms), 4), kernel_ms_max=round(max(ms), 4),
                       yardstick_ms=round(y_ms, 4), kernel_over_yardstick=round(k_ms / y_ms, 2),
                       mkmers_per_s=round(res["n_kmers"] / k_ms / 1e3, 1), algo_gb_s=round(res["algo_bytes"] / k_ms / 1e6, 1),
                       steps=a.steps, warmup=a.warmup)
            print(json.dumps(res), flush=True)
            out.append(res)
            del d_addr
        del index
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)
            f.write("\n")


main()
