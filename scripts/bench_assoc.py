"""kmx_assoc_dev on device-resident bodies: count rows of N = 1000 samples with k = 31 (one key word) and presence/absence rows of
N = 500 with k = 63 (two key words), 100 000 rows, every sample listed, V = 1 (no covariate, not even the intercept) and V = 11 (the
phenotype and ten basis vectors), with about 0.1 % of the rows kept and with every row kept.  Per case: the time of the call's kernels
(median of the timed calls after warm-up, HIP events through kmx_set_profiling), the algorithmic bytes, and -- timed in the same
process -- two yardsticks: kmx_diff_dev on the same body keeping as many rows, and a device-to-device copy that moves the call's
algorithmic bytes (a copy of algo_bytes / 2: as many read and as many written).  The records of the first rows of every body are checked
against tests/assoc_ref.py first, bit for bit.  Needs the GPU (no fallback).
Usage: bench_assoc.py [--rows 100000] [--steps 20] [--warmup 3] [--check-rows 2000] [--out profiles/assoc_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import dist_ref as dr
import diff_ref as fr
import assoc_ref as ar

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=2000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_assoc.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
med = statistics.median


def device_body(rows, N, kw, mode, seed):
    """random keys, a quarter of the columns present; made on the device -> uint8 tensor"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rb = dr.row_bytes(kw, N, mode)
    t = torch.zeros(rows * rb, dtype=torch.uint8, device=dev)
    v = t.view(rows, rb)
    v[:, :8 * kw] = torch.randint(0, 256, (rows, 8 * kw), dtype=torch.uint8, device=dev, generator=g)
    if mode == ar.MODE_COUNT:
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
            total.append(r.kernel_ms()); algo = r.algo_bytes(); kept = r.rows()
        r.free()
    assert min(total) > 0, "profiling gave no time"
    return med(total), min(total), max(total), algo, kept


def cut_for(stats, rows, share):
    """the threshold that keeps about `share` of the rows, from the device's own statistics of every row"""
    st = np.sort(stats)[::-1]
    kk = max(1, int(rows * share))
    return float(0.5 * (st[kk - 1] + st[kk])) if kk < rows else 0.0


def main():
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    out, rows = [], a.rows
    for name, mode, N, k in (("count", ar.MODE_COUNT, 1000, 31), ("pa", ar.MODE_PA, 500, 63)):
        kw = (k + 31) // 32
        rb = dr.row_bytes(kw, N, mode)
        body = device_body(rows, N, kw, mode, 1000 * N + mode)
        cr = min(a.check_rows, rows)
        host = body[:cr * rb].cpu().numpy()
        # the yardstick kmx_diff_dev: half of the samples controls, half cases
        group = np.array([0] * (N // 2) + [1] * (N - N // 2), np.uint8)
        T0, T1 = fr.totals_of(ctx.colsums_dev(body.data_ptr(), rows, N, kw, mode), group)
        dall = ctx.diff_dev(body.data_ptr(), rows, N, kw, mode, group, T0, T1, 0.0)
        diff_thr = {"0.1 %": cut_for(dall.recs["stat"], rows, 0.001), "100 %": 0.0}
        del dall
        diff_ms = {}
        for label, thr in diff_thr.items():
            d_ms, _, _, d_algo, d_kept = timed(lambda: ctx.diff_dev(body.data_ptr(), rows, N, kw, mode, group, T0, T1, thr, keep=True))
            diff_ms[label] = (d_ms, d_algo, d_kept)
        for V in (1, 11):
            vecs = ar.make_vecs("random", N, V, 17 + V)
            par = dict(vecs=vecs, frac_bits=30, gain=2.5, vmin=2.0 ** -10)
            # a subsample against the restatement first
            exp = ar.assoc_expected_np(host, N, kw, mode, vecs, 30, 2.5, 2.0 ** -10, 0.0)
            got = ctx.assoc_dev(body.data_ptr(), cr, N, kw, mode, threshold=0.0, **par)
            assert got.body == exp[1] and got.recs.tobytes() == exp[0].tobytes(), f"{name} V={V}: the first {cr} rows differ from the restatement"
            allr = ctx.assoc_dev(body.data_ptr(), rows, N, kw, mode, threshold=0.0, **par)
            thr_small = cut_for(allr.recs["stat"], rows, 0.001)
            del allr
            for label, thr in (("0.1 %", thr_small), ("100 %", 0.0)):
                k_ms, k_min, k_max, algo, kept = timed(lambda: ctx.assoc_dev(body.data_ptr(), rows, N, kw, mode, threshold=thr, keep=True, **par))
                y_ms = copy_ms(algo // 2)
                d_ms, d_algo, d_kept = diff_ms[label]
                rec = dict(kernel="assoc", mode=name, n_cols=N, kmer_size=k, n_vec=V, rows=rows, row_bytes=rb, body_bytes=rows * rb, kept=label, kept_rows=int(kept),
                           threshold=thr, algo_bytes=algo, steps=a.steps, warmup=a.warmup, kernel_ms=round(k_ms, 4), kernel_ms_min=round(k_min, 4),
                           kernel_ms_max=round(k_max, 4), algo_gb_per_s=round(algo / (k_ms * 1e-3) / 1e9, 2), copy_bytes=algo // 2, copy_ms=round(y_ms, 4),
                           kernels_over_copy=round(k_ms / y_ms, 2), diff_kernel_ms=round(d_ms, 4), diff_kept_rows=int(d_kept), diff_algo_bytes=d_algo,
                           kernels_over_diff=round(k_ms / d_ms, 2), checked_rows=cr)
                out.append(rec); print(json.dumps(rec), flush=True)
        del body
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
