"""kmx_kquery_dev on device-resident k-mer matrices of BASELINE configs[2]'s shape (1000 columns, count rows of 8 + 4000 bytes) and of
a presence/absence index of the same columns (rows of 8 + 125 bytes): k = 31, m = 10, P = 32, queries of 150 bp, half of their k-mers
in the index.  Per case: the call's kernels' time (median of the timed calls after warm-up, HIP events through kmx_set_profiling: the
clears and all five kernels together -- the C ABI does not time them one by one), the algorithmic bytes as kmx_kquery_result_algo_bytes
counts them (bases + found x row bytes + the probes' keys + the tables written), and -- timed in the same process -- the yardstick: a
kernel, compiled from the source below, that loads the bytes of the same found rows, a wave a row, and does nothing else.  The found
rows are worked out here with numpy from the CPU checker's split and count (every occurrence, in partition order; inside a partition
in key order, where the gather goes in position order).  Needs the GPU and hipcc (no fallback).
Usage: bench_kquery.py [--n 1000] [--reads 20000] [--steps K] [--warmup W] [--out profiles/kquery_bench.json]"""
import argparse, ctypes, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import orc
import kquery_ref as kr

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000)
ap.add_argument("--reads", type=int, default=20000)
ap.add_argument("--parts", type=int, default=32)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_kquery.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
K, M, P, N, RL = 31, 10, a.parts, a.n, 150

YARDSTICK = r"""
#include <hip/hip_runtime.h>
// a wave a row: the row's bytes in dwords (rows of a PA matrix start at any byte: the loads are unaligned, as the gather's are)
struct __attribute__((packed, aligned(1))) Dword { unsigned v; };
__global__ __launch_bounds__(256) void k_rows(const unsigned long long* __restrict__ addr, unsigned long long n, unsigned row_bytes, unsigned* __restrict__ sink)
{
  const unsigned lane = threadIdx.x & 63u, nw = row_bytes / 4u;
  const unsigned long long waves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
  unsigned acc = 0;
  for (unsigned long long i = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += waves)
    for (unsigned w = lane; w < nw; w += 64u) acc ^= reinterpret_cast<const Dword*>(addr[i] + 4ull * w)->v;
  if (acc == 0x9E3779B9u) sink[0] = acc;      // (keeps the loads alive)
}
extern "C" float run_rows(const unsigned long long* addr, unsigned long long n, unsigned row_bytes, unsigned* sink, int n_cu)
{
  hipEvent_t e0, e1; float ms = -1.f;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
  const unsigned long long blocks = (n + 3) / 4;
  const unsigned grid = (unsigned)(blocks < (unsigned long long)n_cu * 8 ? (blocks ? blocks : 1) : (unsigned long long)n_cu * 8);
  hipEventRecord(e0, 0);
  hipLaunchKernelGGL(k_rows, dim3(grid), dim3(256), 0, 0, addr, n, row_bytes, sink);
  hipEventRecord(e1, 0);
  if (hipEventSynchronize(e1) == hipSuccess) hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return ms;
}
"""


def build_yardstick():
    d = tempfile.mkdtemp(prefix="kmx_kquery_bench_")
    src, so = os.path.join(d, "rows.hip"), os.path.join(d, "librows.so")
    open(src, "w").write(YARDSTICK)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", so])
    so_lib = ctypes.CDLL(so)
    so_lib.run_rows.restype = ctypes.c_float
    so_lib.run_rows.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]
    return so_lib


def main():
    yard = build_yardstick()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lut, rep = orc.minimizer_lut(M), orc.repart_static(M, P)
    reads = kr.random_reads(11, a.reads, RL)
    blob, offs = lib.Context.pack_reads(reads)
    d_b = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    d_o = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_r = torch.from_numpy(rep.view(np.int16)).to(dev)
    # the queries' distinct canonical k-mers per partition with their occurrences; every second one becomes a row
    per_part = []
    for recs, nk, _ in orc.superk_partition(reads, K, M, lut, rep, P):
        keys, cnt = orc.count_kmer(recs, K, 1) if nk else (np.zeros((0, 1), np.uint64), np.zeros(0, np.uint32))
        per_part.append((keys[:, 0].copy(), cnt))
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    ctx = lib.Context(0); ctx.set_profiling(True)
    out = []
    for mode, name in ((lib.MODE_COUNT, "count"), (lib.MODE_PA, "pa")):
        stride = 8 + (4 * N if mode == lib.MODE_COUNT else (N + 7) // 8)
        bodies, addr, found = [], [], 0
        for keys, cnt in per_part:
            kept = np.ascontiguousarray(keys[::2])
            body = torch.randint(1, 256, (len(kept), stride), dtype=torch.uint8, device=dev)
            if len(kept):
                body[:, :8] = torch.from_numpy(kept.view(np.uint8).reshape(len(kept), 8).copy()).to(dev)
            bodies.append(body)
            rows = np.repeat(np.arange(len(kept), dtype=np.uint64), cnt[::2].astype(np.int64))      # every occurrence of a kept key
            addr.append(np.uint64(body.data_ptr()) + rows * np.uint64(stride))
            found += len(rows)
        addr = np.concatenate(addr)
        d_addr = torch.from_numpy(addr.view(np.int64)).to(dev)
        torch.cuda.synchronize()
        args = (d_b.data_ptr(), d_o.data_ptr(), len(offs) - 1, K, M, d_r.data_ptr(), N, 1, mode, [b.data_ptr() for b in bodies], [len(b) for b in bodies])
        ms, algo, res = [], 0, None
        for i in range(a.warmup + a.steps):
            res = ctx.kquery_dev(*args, sums=mode == lib.MODE_COUNT)
            if i >= a.warmup:
                ms.append(res.kernel_ms)
            algo = res.algo_bytes
        n_valid = int(res.n_kmers.sum(dtype=np.uint64))
        want = len(blob) + found * stride + 8 * n_valid + (12 if mode == lib.MODE_COUNT else 4) * len(reads) * N
        assert algo == want, (algo, want)      # the library found the rows this script did
        ys = [yard.run_rows(d_addr.data_ptr(), len(addr), stride, sink.data_ptr(), n_cu) for _ in range(a.warmup + a.steps)][a.warmup:]
        assert min(ys) > 0, "the yardstick kernel did not run"
        k_ms, y_ms = statistics.median(ms), statistics.median(ys)
        out.append(dict(mode=name, n_cols=N, parts=P, k=K, queries=len(reads), bases=len(blob), valid_kmers=n_valid, found=found, row_bytes=stride,
                        rows=int(sum(len(b) for b in bodies)), algo_bytes=int(algo), kernel_ms=round(k_ms, 4), algo_gbps=round(algo / k_ms / 1e6, 1),
                        yardstick_ms=round(y_ms, 4), yardstick_gbps=round(found * stride / y_ms / 1e6, 1), kernel_over_yardstick=round(k_ms / y_ms, 2),
                        steps=a.steps, warmup=a.warmup))
        print(json.dumps(out[-1]), flush=True)
        del bodies, d_addr
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
