"""kmx_spectra_dev on a device-resident partition: 1000 count columns and 98 000 rows (the headline configuration's shape; k = 31, one key
word) and 100 columns with ten times the rows, with bodies of four shapes side by side -- `zero` (every cell 0: every increment of a
histogram falls on one bin), `same` (one random row repeated: one bin a column, one cell a pair), `skewed` (97 % zeros, the shape of a
real matrix) and `uniform` (counts of 0 ... 299 alike: the most bins and cells touched).  Per case HIST (every column, cap 255) and JOINT
(one pair: the gather road on the wide matrix; column 0 against 16 others at a joint cap of 63: six groups of pairs), each timed alone:
the time of the call's kernels (median of the timed calls after warm-up, HIP events through kmx_set_profiling), the algorithmic bytes,
and -- timed the same way in the same process -- the yardstick bench_query.py uses: a kernel, compiled from the source below, that only
loads the bytes the road must read (the body in 16-byte pieces for HIST and for a streamed JOINT, once a group; the gathered counts of a
row, a thread a row, for the gather road) and does nothing else.  Recorded: yardstick time / kernel time.  A subsample of every body is
checked against tests/spectra_ref.py first.  Needs the GPU and hipcc (no fallback).
Usage: bench_spectra.py [--rows 98000] [--steps 20] [--warmup 3] [--check-rows 2000] [--out profiles/spectra_bench.json]"""
import argparse, ctypes, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import spectra_ref as sr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=98_000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=2000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_spectra.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
med = statistics.median
COUNT, PA = sr.MODE_COUNT, sr.MODE_PA

YARDSTICK = r"""
#include <hip/hip_runtime.h>
// n bytes from p (16-byte aligned), 16 bytes a lane, `passes` times over
__global__ __launch_bounds__(256) void k_read(const uint4* __restrict__ p, unsigned long long n16, unsigned passes, unsigned* __restrict__ sink)
{
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned acc = 0;
  for (unsigned t = 0; t < passes; t++)
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
      const uint4 v = p[i];
      acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
  if (acc == 0x9E3779B9u) sink[0] = acc;      // (keeps the loads alive)
}
// a thread a row: the u dwords (or bytes) of the row at off[0 ... u)
__global__ __launch_bounds__(256) void k_gather(const unsigned char* __restrict__ p, unsigned long long rows, unsigned long long row_bytes, const unsigned* __restrict__ off,
                                                unsigned u, unsigned wide, unsigned* __restrict__ sink)
{
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned acc = 0;
  for (unsigned long long r = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride)
    for (unsigned k = 0; k < u; k++) {
      const unsigned char* q = p + r * row_bytes + off[k];
      acc ^= wide ? *reinterpret_cast<const unsigned*>(q) : (unsigned)*q;
    }
  if (acc == 0x9E3779B9u) sink[0] = acc;
}
static float timed(hipEvent_t e0, hipEvent_t e1) { float ms = -1.f; if (hipEventSynchronize(e1) == hipSuccess) hipEventElapsedTime(&ms, e0, e1); return ms; }
extern "C" float run_read(const void* p, unsigned long long bytes, unsigned passes, unsigned* sink, int n_cu)
{
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
  hipEventRecord(e0, 0);
  hipLaunchKernelGGL(k_read, dim3((unsigned)n_cu * 8), dim3(256), 0, 0, (const uint4*)p, bytes / 16, passes, sink);
  hipEventRecord(e1, 0);
  const float ms = timed(e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return ms;
}
extern "C" float run_gather(const void* p, unsigned long long rows, unsigned long long row_bytes, const unsigned* off, unsigned u, unsigned wide, unsigned* sink, int n_cu)
{
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.f;
  hipEventRecord(e0, 0);
  hipLaunchKernelGGL(k_gather, dim3((unsigned)n_cu * 8), dim3(256), 0, 0, (const unsigned char*)p, rows, row_bytes, off, u, wide, sink);
  hipEventRecord(e1, 0);
  const float ms = timed(e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return ms;
}
"""


def build_yardstick():
    d = tempfile.mkdtemp(prefix="kmx_spectra_bench_")
    src, so = os.path.join(d, "loads.hip"), os.path.join(d, "libloads.so")
    open(src, "w").write(YARDSTICK)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", so])
    so_lib = ctypes.CDLL(so)
    so_lib.run_read.restype = ctypes.c_float
    so_lib.run_read.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]
    so_lib.run_gather.restype = ctypes.c_float
    so_lib.run_gather.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]
    return so_lib


def device_body(rows, N, kw, mode, shape, seed):
    """made on the device -> uint8 tensor (16-byte aligned)"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rb = sr.row_bytes(kw, N, mode)
    t = torch.zeros(rows * rb, dtype=torch.uint8, device=dev)
    v = t.view(rows, rb)
    v[:, :8 * kw] = torch.randint(0, 256, (rows, 8 * kw), dtype=torch.uint8, device=dev, generator=g)
    if shape == "zero":
        c = torch.zeros((rows, N), dtype=torch.int32, device=dev)
    elif shape == "same":
        c = (torch.randint(0, 300, (1, N), dtype=torch.int32, device=dev, generator=g) * (torch.rand((1, N), device=dev, generator=g) < 0.5)).expand(rows, N)
    elif shape == "skewed":
        c = torch.randint(1, 50, (rows, N), dtype=torch.int32, device=dev, generator=g) * (torch.rand((rows, N), device=dev, generator=g) < 0.03)
    else:
        c = torch.randint(0, 300, (rows, N), dtype=torch.int32, device=dev, generator=g)
    if mode == COUNT:
        v[:, 8 * kw:] = c.contiguous().to(torch.int32).view(torch.uint8).view(rows, 4 * N)
    else:
        pad = (-N) % 8
        bits = torch.cat([c != 0, torch.ones((rows, pad), dtype=torch.bool, device=dev)], dim=1).view(rows, -1, 8).to(torch.uint8)
        w = (2 ** torch.arange(8, device=dev)).to(torch.uint8)
        v[:, 8 * kw:] = (bits * w).sum(dim=2).to(torch.uint8)
    torch.cuda.synchronize()
    return t


def timed(call):
    total, algo = [], 0
    for step in range(a.warmup + a.steps):
        r = call()
        r.wait()
        if step >= a.warmup:
            total.append(r.kernel_ms()); algo = r.algo_bytes()
        r.free()
    assert min(total) > 0, "profiling gave no time"
    return med(total), min(total), max(total), algo


def main():
    yard = build_yardstick()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    out, kw = [], 1

    def yard_read(body, passes):
        ts = [yard.run_read(body.data_ptr(), body.numel(), passes, sink.data_ptr(), n_cu) for _ in range(a.warmup + a.steps)][a.warmup:]
        return med(ts)

    def yard_gather(body, rows, rb, offs, wide):
        o = torch.tensor(offs, dtype=torch.int32, device=dev)
        ts = [yard.run_gather(body.data_ptr(), rows, rb, o.data_ptr(), len(offs), wide, sink.data_ptr(), n_cu) for _ in range(a.warmup + a.steps)][a.warmup:]
        return med(ts)

    for N, rows in ((1000, a.rows), (100, 10 * a.rows)):
        for mode, mname in ((COUNT, "count"), (PA, "pa")):
            rb = sr.row_bytes(kw, N, mode)
            joints = (("one_pair", np.array([[0, N - 1]], np.uint32), 63), ("against_16", np.array([[0, 1 + 5 * j] for j in range(16)], np.uint32), 63))
            for shape in ("zero", "same", "skewed", "uniform"):
                body = device_body(rows, N, kw, mode, shape, 31 + mode + N)
                cr = min(a.check_rows, rows)
                head = body[:cr * rb].cpu().numpy()
                got = ctx.spectra_dev(body.data_ptr(), cr, N, kw, mode, cap=255, pairs=joints[1][1], joint_cap=63)
                eh, ej = sr.spectra_expected_np(head, N, kw, mode, None, 255, joints[1][1], 63)
                assert got.hist.tobytes() == eh.tobytes() and got.joint.tobytes() == ej.tobytes(), f"{mname} {N} {shape}: the first {cr} rows"
                y_body = yard_read(body, 1)
                h_ms, h_min, h_max, h_algo = timed(lambda: ctx.spectra_dev(body.data_ptr(), rows, N, kw, mode, cap=255, keep=True))
                rec = dict(kernel="spectra", part="hist", mode=mname, shape=shape, n_cols=N, rows=rows, row_bytes=rb, body_bytes=rows * rb, cap=255, steps=a.steps, warmup=a.warmup,
                           checked_rows=cr, kernel_ms=round(h_ms, 4), kernel_ms_min=round(h_min, 4), kernel_ms_max=round(h_max, 4), algo_bytes=h_algo,
                           algo_gb_per_s=round(h_algo / (h_ms * 1e-3) / 1e9, 1), load_only_ms=round(y_body, 4), load_only_over_kernel=round(y_body / h_ms, 3))
                out.append(rec); print(json.dumps(rec), flush=True)
                for jname, pairs, jc in joints:
                    pl = sr.joint_plan(pairs, jc, rb)
                    if pl["stream"]:
                        y = yard_read(body, pl["n_groups"])
                    else:      # (one group: its distinct columns)
                        cols = sorted({int(c) for c in pairs.reshape(-1)})
                        y = yard_gather(body, rows, rb, [8 * kw + (4 * c if mode == COUNT else c >> 3) for c in cols], int(mode == COUNT))
                    j_ms, j_min, j_max, j_algo = timed(lambda: ctx.spectra_dev(body.data_ptr(), rows, N, kw, mode, hist=False, pairs=pairs, joint_cap=jc, keep=True))
                    rec = dict(kernel="spectra", part="joint", pairs=jname, n_pairs=len(pairs), joint_cap=jc, groups=pl["n_groups"], road="stream" if pl["stream"] else "gather",
                               mode=mname, shape=shape, n_cols=N, rows=rows, row_bytes=rb, body_bytes=rows * rb, steps=a.steps, warmup=a.warmup,
                               kernel_ms=round(j_ms, 4), kernel_ms_min=round(j_min, 4), kernel_ms_max=round(j_max, 4), algo_bytes=j_algo,
                               algo_gb_per_s=round(j_algo / (j_ms * 1e-3) / 1e9, 1), load_only_ms=round(y, 4), load_only_over_kernel=round(y / j_ms, 3))
                    out.append(rec); print(json.dumps(rec), flush=True)
                del body
                torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
