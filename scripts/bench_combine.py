"""kmx_combine_dev on device-resident blocks: two count blocks of 1000 columns (k = 31, half of each block's keys shared) -- the wide
case --, the same columns in 8 blocks of 250, the k = 63 presence/absence shape (two blocks of 500 columns, keys of two words) and
32 one-column count blocks.  Per case: the kernels' time (median of the timed calls after warm-up, min - max; HIP events through
kmx_set_profiling), the algorithmic bytes (every input row read once plus every output row written once), their rate against the
8 TB/s of the project's rooflines, and -- measured in the same process -- the time of a plain device-to-device copy that reads and
writes the same number of bytes in all, the yardstick that does not depend on the code under test.  --e2e DIR adds the driver end
to end: `kmx combine --gpus 1` against the same binary without --gpus over two synthetic runs of 32 partitions written under DIR
(a RAM file system), wall clocks of both.  Needs the GPU (no fallback).
Usage: bench_combine.py [--rows N] [--steps K] [--warmup W] [--e2e DIR] [--out profiles/combine_bench.json]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--e2e", default=None)
ap.add_argument("--e2e-rows", type=int, default=4000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_combine.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
ctx = lib.Context(0); ctx.set_profiling(True)
HBM = 8e12


def block_keys(rng, n_blocks, rows, kw, share):
    """sorted keys of n_blocks blocks of `rows` rows: a share of every block's keys is common to all blocks"""
    n_sh = int(rows * share)
    keys = np.unique(rng.integers(0, 1 << 62, (int((n_sh + n_blocks * (rows - n_sh)) * 1.1) + 8, kw), dtype=np.uint64), axis=0)
    keys = keys[rng.permutation(len(keys))]
    out = []
    for i in range(n_blocks):
        k = np.concatenate([keys[:n_sh], keys[n_sh + i * (rows - n_sh):n_sh + (i + 1) * (rows - n_sh)]])
        out.append(k[np.lexsort([k[:, j] for j in range(kw)])])
    return out


def case(name, kw, n_blocks, n_cols, mode, rows, seed, share=0.5):
    rng = np.random.default_rng(seed)
    pb = 4 * n_cols if mode == lib.MODE_COUNT else (n_cols + 7) // 8
    blocks, keep = [], []
    for k in block_keys(rng, n_blocks, rows, kw, share):
        t = torch.randint(0, 256, (len(k), 8 * kw + pb), dtype=torch.uint8, device=dev)
        t[:, :8 * kw] = torch.from_numpy(k.view(np.uint8).reshape(len(k), 8 * kw)).to(dev)
        keep.append(t); blocks.append((t.data_ptr(), len(k), n_cols, 4))
    torch.cuda.synchronize()
    ms, res = [], None
    for i in range(a.warmup + a.steps):
        r = ctx.combine_dev(blocks, kw, mode, keep=True)
        r.wait()
        if i >= a.warmup: ms.append(r.kernel_ms())
        res = dict(blocks=n_blocks, rows_per_block=rows, rows_out=r.rows(), row_bytes_out=r.row_bytes(), algo_bytes=r.algo_bytes())
        r.free()
    # the yardstick: a device-to-device copy that reads and writes algo_bytes in all (half of them each way)
    half = max(res["algo_bytes"] // 2, 1)
    src = torch.empty(half, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    cp = []
    for i in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        if i >= a.warmup: cp.append(e0.elapsed_time(e1))
    del src, dst
    k_ms, c_ms = statistics.median(ms), statistics.median(cp)
    res.update(case=name, key_words=kw, n_cols_per_block=n_cols, mode="count" if mode == lib.MODE_COUNT else "pa", shared=share,
               kernel_ms=round(k_ms, 4), kernel_ms_min=round(min(ms), 4), kernel_ms_max=round(max(ms), 4),
               algo_tb_s=round(res["algo_bytes"] / k_ms / 1e9, 3), share_of_8tb_s=round(res["algo_bytes"] / (k_ms * 1e-3) / HBM, 4),
               d2d_copy_same_bytes_ms=round(c_ms, 4), kernel_over_copy=round(k_ms / c_ms, 2), steps=a.steps, warmup=a.warmup)
    print(json.dumps(res), flush=True)
    return res


def end_to_end(root):
    """two synthetic count runs of 32 partitions (500 and 300 columns) under root; wall clocks of the host path and of --gpus 1"""
    import combine_runs as runs, shutil
    root = os.path.join(root, "kmx_combine_bench"); shutil.rmtree(root, ignore_errors=True); os.makedirs(root)
    P, cols = 32, [500, 300]
    rng = np.random.default_rng(5)
    per_run = [[], []]
    for p in range(P):
        ks = block_keys(rng, 2, a.e2e_rows, 1, 0.5)
        for r in range(2):
            per_run[r].append((ks[r], rng.integers(0, 256, (len(ks[r]), 4 * cols[r]), dtype=np.uint8), cols[r], 4))
    for r in range(2):
        runs.write_run(f"{root}/run{r}", "count", 31, per_run[r], [f"R{r}S{i}" for i in range(cols[r])])
    open(f"{root}/runs.fof", "w").write(f"{root}/run0\n{root}/run1\n")
    in_bytes = sum(len(b[0]) * (8 + 4 * b[2]) for r in per_run for b in r)
    res = dict(partitions=P, rows_per_block=a.e2e_rows, cols=cols, input_bytes=in_bytes)
    for name, flags in (("host", []), ("gpus1", ["--gpus", "1"]), ("host_again", []), ("gpus1_again", ["--gpus", "1"])):
        out = f"{root}/out_{name}"
        t0 = time.perf_counter()
        r = subprocess.run([runs.KMX, "combine", "--fof", f"{root}/runs.fof", "--output", out] + flags, capture_output=True, text=True, timeout=900)
        res[f"wall_s_{name}"] = round(time.perf_counter() - t0, 3)
        if r.returncode != 0:
            sys.exit(f"kmx combine {flags} failed: {r.stderr}")
    if runs.tree(f"{root}/out_host") != runs.tree(f"{root}/out_gpus1"):
        sys.exit("kmx combine --gpus 1 does not write what the host path writes")
    res["outputs_equal"] = True
    res["output_bytes"] = sum(os.path.getsize(f"{root}/out_host/matrices/matrix_{p}.count") for p in range(P))
    shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(res), flush=True)
    return res


out = [case("count 2 x N=1000 k=31 (wide)", 1, 2, 1000, lib.MODE_COUNT, a.rows, 1),
       case("count 8 x N=250 k=31", 1, 8, 250, lib.MODE_COUNT, a.rows, 2),
       case("pa 2 x N=500 k=63", 2, 2, 500, lib.MODE_PA, a.rows, 3),
       case("count 32 x N=1 k=31", 1, 32, 1, lib.MODE_COUNT, a.rows, 4)]
doc = dict(device=torch.cuda.get_device_name(0), cases=out)
if a.e2e:
    doc["end_to_end"] = end_to_end(a.e2e)
if a.out:
    json.dump(doc, open(a.out, "w"), indent=1)
