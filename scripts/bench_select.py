"""kmx_select_dev on device-resident bodies of 100 000 rows: count rows of N = 1000 samples with k = 31 (one key word) -- every column
as it stands, M = 200 scattered columns, and the same 200 as presence/absence bits, each with about 0.1 %, about half and all of the
rows kept -- and presence/absence rows of N = 500 with k = 63 (two key words), M = 100 permuted columns.  Per case: the time of the
call's kernels (median of the timed calls after warm-up, HIP events through kmx_set_profiling), the algorithmic bytes, and -- timed the
same way in the same process -- two yardsticks: a device-to-device copy that moves the same number of bytes (a copy of algo_bytes / 2),
and, for the identity cases, kmx_diff_dev at threshold 0 with the same min_rec on the same body (the closest road there was before
select).  The first rows of every case are checked against tests/select_ref.py first.  Needs the GPU (no fallback).
Usage: bench_select.py [--rows 100000] [--steps 20] [--warmup 3] [--check-rows 2000] [--out profiles/select_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import select_ref as sr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=2000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_select.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
med = statistics.median
COUNT, PA = sr.MODE_COUNT, sr.MODE_PA


def device_body(rows, N, kw, mode, seed):
    """random keys, a quarter of the columns present; made on the device -> uint8 tensor"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rb = sr.row_bytes(kw, N, mode)
    t = torch.zeros(rows * rb, dtype=torch.uint8, device=dev)
    v = t.view(rows, rb)
    v[:, :8 * kw] = torch.randint(0, 256, (rows, 8 * kw), dtype=torch.uint8, device=dev, generator=g)
    if mode == COUNT:
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


def main():
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    out, rows = [], a.rows
    rng = np.random.default_rng(5)
    shapes = (("count", COUNT, 1000, 31, (("identity", None, COUNT), ("200 scattered", np.sort(rng.permutation(1000)[:200]).astype(np.uint32), COUNT),
                                          ("200 scattered to pa", None, PA))),
              ("pa", PA, 500, 63, (("100 permuted", rng.permutation(500)[:100].astype(np.uint32), PA),)))
    for name, mode, N, k, lists in shapes:
        kw = (k + 31) // 32
        rb = sr.row_bytes(kw, N, mode)
        body = device_body(rows, N, kw, mode, 1000 * N + mode)
        scattered = lists[1][1] if len(lists) > 1 else None
        for label, cols, out_mode in lists:
            if label.endswith("to pa"):
                cols = scattered
            M = N if cols is None else len(cols)
            # the recurrence of every row over these columns, from the device itself: the bounds that keep 0.1 % and half of the rows
            allr = ctx.select_dev(body.data_ptr(), rows, N, kw, mode, cols=cols, out_mode=out_mode)
            rec_sorted = np.sort(allr.recs["rec"])[::-1]
            del allr
            bounds = (("0.1 %", int(rec_sorted[max(1, rows // 1000) - 1])), ("50 %", int(rec_sorted[rows // 2])), ("100 %", 0)) if mode == COUNT else (("100 %", 0),)
            # a subsample against the restatement first
            cr = min(a.check_rows, rows)
            host = body[:cr * rb].cpu().numpy()
            for _, lo in bounds:
                got = ctx.select_dev(body.data_ptr(), cr, N, kw, mode, cols=cols, out_mode=out_mode, min_rec=lo)
                exp = sr.select_expected_np(host, N, kw, mode, cols, out_mode=out_mode, min_rec=lo)
                assert got.body == exp[0] and got.recs.tobytes() == exp[1].tobytes(), f"{name} {label}: the first {cr} rows at min_rec {lo}"
            for share, lo in bounds:
                k_ms, k_min, k_max, algo, kept = timed(lambda: ctx.select_dev(body.data_ptr(), rows, N, kw, mode, cols=cols, out_mode=out_mode, min_rec=lo, keep=True))
                y_ms = copy_ms(algo // 2)
                rec = dict(kernel="select", mode=name, out_mode=["count", "pa"][out_mode], columns=label, n_cols=N, n_out=M, kmer_size=k, rows=rows, row_bytes=rb,
                           body_bytes=rows * rb, kept=share, min_rec=lo, kept_rows=int(kept), algo_bytes=algo, steps=a.steps, warmup=a.warmup,
                           kernel_ms=round(k_ms, 4), kernel_ms_min=round(k_min, 4), kernel_ms_max=round(k_max, 4), algo_gb_per_s=round(algo / (k_ms * 1e-3) / 1e9, 2),
                           copy_bytes=algo // 2, copy_ms=round(y_ms, 4), kernels_over_copy=round(k_ms / y_ms, 2), checked_rows=cr)
                if label == "identity":      # the road there was before: diff at threshold 0 keeps the rows that pass min_rec (every column a control or a case)
                    group = np.array([0] * (N // 2) + [1] * (N - N // 2), np.uint8)
                    d_ms, d_min, d_max, _, d_kept = timed(lambda: ctx.diff_dev(body.data_ptr(), rows, N, kw, mode, group, 1000, 1000, 0.0, lo, keep=True))
                    assert d_kept == kept, (d_kept, kept)
                    rec.update(diff_ms=round(d_ms, 4), diff_ms_min=round(d_min, 4), diff_ms_max=round(d_max, 4), select_over_diff=round(k_ms / d_ms, 3))
                out.append(rec); print(json.dumps(rec), flush=True)
        del body
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
