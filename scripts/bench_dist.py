"""kmx_dist_dev on device-resident bodies the size of one partition of the headline workload (3.15 M rows / 32 = 98 437 rows): N = 100
and N = 1000 samples, PA and COUNT rows, COUNT with and without mins; a quarter of the columns present.  Per case: the time of the
call and of each kernel (median of the timed calls after warm-up, HIP events through kmx_set_profiling; the clearing of the tables is
inside the first part), the algorithmic bytes, the pair-word operations per second counted as ceil(rows / 64) * N (N + 1) / 2, and --
timed in the same process -- the memory yardstick: a kernel, compiled from the source below, that loads the same body once and does
nothing else.  The tables of the first rows of every body are checked against tests/dist_ref.py first.  Needs the GPU and hipcc (no
fallback).
Usage: bench_dist.py [--n 100,1000] [--rows 98437] [--steps 20] [--warmup 3] [--check-rows 3000] [--out profiles/dist_bench.json]"""
import argparse, ctypes, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import dist_ref as dr

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="100,1000")
ap.add_argument("--rows", type=int, default=3_150_000 // 32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=3000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_dist.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()

YARDSTICK = r"""
#include <hip/hip_runtime.h>
// the body once, 16 bytes a lane (the buffer starts at a multiple of 16 and is padded to one)
__global__ __launch_bounds__(256) void k_load(const uint4* __restrict__ p, unsigned long long n16, unsigned* __restrict__ sink)
{
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned acc = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
    const uint4 v = p[i];
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x9E3779B9u) sink[0] = acc;      // (keeps the loads alive)
}
extern "C" float run_load(const void* p, unsigned long long n16, unsigned* sink, int n_cu)
{
  hipEvent_t e0, e1; float ms = -1.f;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
  const unsigned long long blocks = (n16 + 255) / 256;
  const unsigned grid = (unsigned)(blocks < (unsigned long long)n_cu * 8 ? (blocks ? blocks : 1) : (unsigned long long)n_cu * 8);
  hipEventRecord(e0, 0);
  hipLaunchKernelGGL(k_load, dim3(grid), dim3(256), 0, 0, (const uint4*)p, n16, sink);
  hipEventRecord(e1, 0);
  if (hipEventSynchronize(e1) == hipSuccess) hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return ms;
}
"""


def build_yardstick():
    d = tempfile.mkdtemp(prefix="kmx_dist_bench_")
    src, so = os.path.join(d, "load.hip"), os.path.join(d, "libload.so")
    open(src, "w").write(YARDSTICK)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", so])
    so_lib = ctypes.CDLL(so)
    so_lib.run_load.restype = ctypes.c_float
    so_lib.run_load.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
    return so_lib


def device_body(rows, N, mode, seed):
    """random keys (one word), a quarter of the columns present; made on the device -> uint8 tensor, padded to 16 bytes"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rb = dr.row_bytes(1, N, mode)
    t = torch.zeros((rows * rb + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    v = t[:rows * rb].view(rows, rb)
    v[:, :8] = torch.randint(0, 256, (rows, 8), dtype=torch.uint8, device=dev, generator=g)
    if mode == dr.MODE_COUNT:
        c = torch.randint(1, 50, (rows, N), dtype=torch.int32, device=dev, generator=g)
        c = c * (torch.rand((rows, N), device=dev, generator=g) < 0.25)
        v[:, 8:] = c.to(torch.int32).view(torch.uint8).view(rows, 4 * N)
    else:
        nb = (N + 7) // 8
        v[:, 8:] = (torch.randint(0, 256, (rows, nb), dtype=torch.uint8, device=dev, generator=g) &
                    torch.randint(0, 256, (rows, nb), dtype=torch.uint8, device=dev, generator=g))
    torch.cuda.synchronize()
    return t


def main():
    yard = build_yardstick()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    out, rows = [], a.rows
    for N in [int(x) for x in a.n.split(",")]:
        for mode, name in ((dr.MODE_PA, "pa"), (dr.MODE_COUNT, "count")):
            rb = dr.row_bytes(1, N, mode)
            body = device_body(rows, N, mode, 1000 * N + mode)
            for mins in ((False, True) if mode == dr.MODE_COUNT else (False,)):
                # a subsample against the restatement first
                cr = min(a.check_rows, rows)
                host = body[:cr * rb].cpu().numpy()
                exp = dr.dist_expected_np(host, N, 1, mode, mins=mins, blas=True)
                got = ctx.dist_dev(body.data_ptr(), cr, N, 1, mode, mins=mins)
                assert np.array_equal(got.inter, exp[0]) and (not mins or np.array_equal(got.mins, exp[1])), f"N={N} {name}: the tables of the first {cr} rows differ from dist_ref"
                total, parts, algo = [], [], 0
                for step in range(a.warmup + a.steps):
                    r = ctx.dist_dev(body.data_ptr(), rows, N, 1, mode, mins=mins, keep=True)
                    r.wait()
                    if step >= a.warmup:
                        total.append(r.kernel_ms()); parts.append(r.kernel_parts_ms()); algo = r.algo_bytes()
                    r.free()
                assert min(total) > 0, "profiling gave no time"
                ys = [yard.run_load(body.data_ptr(), body.numel() // 16, sink.data_ptr(), n_cu) for _ in range(a.warmup + a.steps)][a.warmup:]
                assert min(ys) > 0, "the yardstick kernel did not run"
                med = statistics.median
                k_ms, y_ms = med(total), med(ys)
                slab_ms, pairs_ms, mins_ms = (med([p[i] for p in parts]) for i in range(3))
                pair_words = (rows + 63) // 64 * N * (N + 1) // 2
                rec = dict(n_cols=N, mode=name, mins=mins, rows=rows, row_bytes=rb, body_bytes=rows * rb, algo_bytes=algo, steps=a.steps, warmup=a.warmup,
                           kernel_ms=round(k_ms, 4), kernel_ms_min=round(min(total), 4), kernel_ms_max=round(max(total), 4),
                           clear_and_slab_ms=round(slab_ms, 4), pairs_ms=round(pairs_ms, 4), mins_ms=round(mins_ms, 4) if mins else None,
                           pair_word_ops=pair_words, pair_word_ops_per_s=round(pair_words / (pairs_ms * 1e-3), 1),
                           algo_gb_per_s=round(algo / (k_ms * 1e-3) / 1e9, 2),
                           yardstick_ms=round(y_ms, 4), yardstick_gb_per_s=round(body.numel() / (y_ms * 1e-3) / 1e9, 2),
                           kernel_over_yardstick=round(k_ms / y_ms, 2), checked_rows=cr)
                out.append(rec)
                print(json.dumps(rec), flush=True)
            del body
            torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
