"""kmx_colsums_dev and kmx_diff_dev on device-resident bodies: count rows of N = 1000 samples with k = 31 (one key word) and
presence/absence rows of N = 500 with k = 63 (two key words), 100 000 rows, half of the samples controls and half cases, with about
0.1 % of the rows kept and with every row kept.  Per case: the time of the call's kernels (median of the timed calls after warm-up, HIP
events through kmx_set_profiling), the algorithmic bytes, and -- timed in the same process -- the yardstick: a device-to-device copy
that moves the same number of bytes (a copy of algo_bytes / 2: as many read and as many written).  The records of the first rows of
every body are checked against tests/diff_ref.py first.  Needs the GPU (no fallback).
Usage: bench_diff.py [--rows 100000] [--steps 20] [--warmup 3] [--check-rows 2000] [--out profiles/diff_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import dist_ref as dr
import diff_ref as fr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=2000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_diff.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
med = statistics.median


def device_body(rows, N, kw, mode, seed):
    """random keys, a quarter of the columns present; made on the device -> uint8 tensor"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rb = dr.row_bytes(kw, N, mode)
    t = torch.zeros(rows * rb, dtype=torch.uint8, device=dev)
    v = t.view(rows, rb)
    v[:, :8 * kw] = torch.randint(0, 256, (rows, 8 * kw), dtype=torch.uint8, device=dev, generator=g)
    if mode == fr.MODE_COUNT:
        c = torch.randint(1, 50, (rows, N), dtype=torch.int32, device=dev, generator=g)
        c = c * (torch.rand((rows, N), device=dev, generator=g) < 0.25)
        v[:, 8 * kw:] = c.to(torch.int32).view(torch.uint8).view(rows, 4 * N)
    else:
        nb = (N + 7) // 8
        v[:, 8 * kw:] = (torch.randint(0, 256, (rows, nb), dtype=torch.uint8, device=dev, generator=g) &
                         torch.randint(0, 256, (rows, nb), dtype=torch.uint8, device=dev, generator=g))
    torch.cuda.synchronize()
    return t


def copy_ms(nbytes):
    """a device-to-device copy of nbytes, the median of the timed calls after warm-up"""
    src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    ms = []
    for step in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); e1.synchronize()
        if step >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    return med(ms)


def timed(call):
    total, algo, kept = [], 0, 0
    for step in range(a.warmup + a.steps):
        r = call()
        r.wait()
        if step >= a.warmup:
            total.append(r.kernel_ms()); algo = r.algo_bytes(); kept = r.rows() if hasattr(r, "rows") else 0
        r.free()
    assert min(total) > 0, "profiling gave no time"
    return med(total), min(total), max(total), algo, kept


def main():
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    out, rows = [], a.rows
    for name, mode, N, k in (("count", fr.MODE_COUNT, 1000, 31), ("pa", fr.MODE_PA, 500, 63)):
        kw = (k + 31) // 32
        rb = dr.row_bytes(kw, N, mode)
        body = device_body(rows, N, kw, mode, 1000 * N + mode)
        group = np.array([0] * (N // 2) + [1] * (N - N // 2), np.uint8)
        sums = ctx.colsums_dev(body.data_ptr(), rows, N, kw, mode)
        T0, T1 = fr.totals_of(sums, group)
        # a subsample against the restatement first
        cr = min(a.check_rows, rows)
        host = body[:cr * rb].cpu().numpy()
        assert np.array_equal(ctx.colsums_dev(body.data_ptr(), cr, N, kw, mode), fr.colsums_np(host, N, kw, mode)), f"{name}: the column sums of the first {cr} rows differ"
        exp = fr.diff_expected_mixed(host, N, kw, mode, group, T0, T1)
        got = ctx.diff_dev(body.data_ptr(), cr, N, kw, mode, group, T0, T1, 0.0)
        assert got.recs["row"].tolist() == list(range(cr)) and got.body == host.tobytes(), f"{name}: the rows kept at threshold 0"
        for q, x in zip(got.recs, exp):
            assert (int(q["sum_ctrl"]), int(q["sum_case"]), int(q["rec_ctrl"]), int(q["rec_case"]), int(q["over"])) == (x["c0"], x["c1"], x["r0"], x["r1"], x["over"])
            assert abs(x["stat"] - float(q["stat"])) <= x["tol"], f"{name}: the statistic of row {int(q['row'])}"
        # the threshold that keeps about 0.1 % of the rows: from the device's own statistics of every row
        allr = ctx.diff_dev(body.data_ptr(), rows, N, kw, mode, group, T0, T1, 0.0)
        st = np.sort(allr.recs["stat"])[::-1]
        kk = max(1, rows // 1000)
        thr_small = float(0.5 * (st[kk - 1] + st[kk])) if kk < rows else 0.0
        del allr
        k_ms, k_min, k_max, algo, _ = timed(lambda: ctx.colsums_dev(body.data_ptr(), rows, N, kw, mode, keep=True))
        y_ms = copy_ms(algo // 2)
        rec = dict(kernel="colsums", mode=name, n_cols=N, kmer_size=k, rows=rows, row_bytes=rb, body_bytes=rows * rb, algo_bytes=algo, steps=a.steps, warmup=a.warmup,
                   kernel_ms=round(k_ms, 4), kernel_ms_min=round(k_min, 4), kernel_ms_max=round(k_max, 4), algo_gb_per_s=round(algo / (k_ms * 1e-3) / 1e9, 2),
                   copy_bytes=algo // 2, copy_ms=round(y_ms, 4), kernels_over_copy=round(k_ms / y_ms, 2), checked_rows=cr)
        out.append(rec); print(json.dumps(rec), flush=True)
        for label, thr in (("0.1 %", thr_small), ("100 %", 0.0)):
            k_ms, k_min, k_max, algo, kept = timed(lambda: ctx.diff_dev(body.data_ptr(), rows, N, kw, mode, group, T0, T1, thr, keep=True))
            y_ms = copy_ms(algo // 2)
            rec = dict(kernel="diff", mode=name, n_cols=N, kmer_size=k, rows=rows, row_bytes=rb, body_bytes=rows * rb, kept=label, kept_rows=int(kept), threshold=thr,
                       algo_bytes=algo, steps=a.steps, warmup=a.warmup, kernel_ms=round(k_ms, 4), kernel_ms_min=round(k_min, 4), kernel_ms_max=round(k_max, 4),
                       algo_gb_per_s=round(algo / (k_ms * 1e-3) / 1e9, 2), copy_bytes=algo // 2, copy_ms=round(y_ms, 4), kernels_over_copy=round(k_ms / y_ms, 2),
                       checked_rows=cr)
            out.append(rec); print(json.dumps(rec), flush=True)
        del body
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
