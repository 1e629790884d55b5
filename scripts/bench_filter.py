"""kmx_filter_dev on a device-resident partition: the headline shape (about 100 000 rows of 1000 u32 columns, k = 31) against key
lists that keep about 1 %, 50 % and 100 % of the rows, and the k = 63 presence/absence shape of BASELINE configs[4] (500 samples, keys of
two words).  Per case: the kernels' time (median of the timed calls after warm-up, HIP events through kmx_set_profiling), the
algorithmic bytes (keys and key list read, kept rows in and out, vector and absent records out), their rate against the 8 TB/s of
the project's rooflines, and -- measured in the same process -- the time of a plain device-to-device copy of the same number of
bytes, the yardstick that does not depend on the code under test.  Needs the GPU (no fallback).
Usage: bench_filter.py [--rows N] [--steps K] [--warmup W] [--out profiles/filter_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_filter.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
ctx = lib.Context(0); ctx.set_profiling(True)
HBM = 8e12


def case(name, kw, n_cols, mode, keep, seed):
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << 62, (int(a.rows * 2.2), kw), dtype=np.uint64), axis=0)
    keys = keys[np.lexsort([keys[:, j] for j in range(kw)])]
    is_row = np.zeros(len(keys), bool); is_row[rng.permutation(len(keys))[:a.rows]] = True
    rk = keys[is_row]
    shared = rng.random(len(rk)) < keep if keep < 1 else np.ones(len(rk), bool)
    others = keys[~is_row][:max(a.rows - int(shared.sum()), 0)]      # the key list is as long as the matrix
    kk = np.concatenate([rk[shared], others]); kk = kk[np.lexsort([kk[:, j] for j in range(kw)])]
    pb = 4 * n_cols if mode == lib.MODE_COUNT else (n_cols + 7) // 8
    rows = torch.randint(0, 256, (len(rk), 8 * kw + pb), dtype=torch.uint8, device=dev)
    rows[:, :8 * kw] = torch.from_numpy(rk.view(np.uint8).reshape(len(rk), 8 * kw)).to(dev)
    rec = torch.from_numpy(lib.pack_records(kk, rng.integers(1, 255, len(kk), dtype=np.uint32), kw).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    ms, res = [], None
    for i in range(a.warmup + a.steps):
        r = ctx.filter_dev(rows.data_ptr(), len(rk), n_cols, kw, mode, (rec.data_ptr(), len(kk)), "kmv", keep=True)
        r.wait()
        if i >= a.warmup: ms.append(r.kernel_ms())
        res = dict(rows=len(rk), kept=r.rows(), row_bytes_out=r.row_bytes(), key_records=len(kk), algo_bytes=r.algo_bytes())
        r.free()
    # the yardstick: a device-to-device copy that reads and writes algo_bytes in all (half of them each way)
    half = max(res["algo_bytes"] // 2, 1)
    src = torch.empty(half, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    cp = []
    for i in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        if i >= a.warmup: cp.append(e0.elapsed_time(e1))
    k_ms, c_ms = statistics.median(ms), statistics.median(cp)
    res.update(case=name, key_words=kw, n_cols=n_cols, mode="count" if mode == lib.MODE_COUNT else "pa", kernel_ms=round(k_ms, 4),
               kernel_ms_min=round(min(ms), 4), kernel_ms_max=round(max(ms), 4), algo_tb_s=round(res["algo_bytes"] / k_ms / 1e9, 3),
               share_of_8tb_s=round(res["algo_bytes"] / (k_ms * 1e-3) / HBM, 4), d2d_copy_same_bytes_ms=round(c_ms, 4),
               kernel_over_copy=round(k_ms / c_ms, 2), steps=a.steps, warmup=a.warmup)
    print(json.dumps(res), flush=True)
    return res


out = [case("count N=1000 k=31, 1 % kept", 1, 1000, lib.MODE_COUNT, 0.01, 1),
       case("count N=1000 k=31, 50 % kept", 1, 1000, lib.MODE_COUNT, 0.5, 2),
       case("count N=1000 k=31, 100 % kept", 1, 1000, lib.MODE_COUNT, 1.0, 3),
       case("pa N=500 k=63, 50 % kept", 2, 500, lib.MODE_PA, 0.5, 4)]
if a.out:
    json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), open(a.out, "w"), indent=1)
