"""kmx_pan_dev on device-resident bodies of the headline configuration's shape: 1000 count columns and about 98 000 rows a partition
(k = 31, one key word), and a presence/absence body of the same columns -- with the rows of a real matrix's shape (most rows private or
core) and with every recurrence as often as any other (the most flushes of k_pan_shared).  Per case: the time of the call's kernels by
part (score + fold, order, shared; median of the timed calls after warm-up, HIP events through kmx_set_profiling), the algorithmic
bytes and their rate against the 8 TB/s of the project's rooflines, and -- timed the same way in the same process -- the yardstick:
kmx_colsums_dev on the same body, which reads the body once and adds per column.  Recorded: score : colsums, and
(score + order + shared) : 2 x colsums.  A subsample of every body is checked against tests/pan_ref.py first.  Needs the GPU.
Usage: bench_pan.py [--rows 98000] [--steps 20] [--warmup 3] [--check-rows 2000] [--out profiles/pan_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import pan_ref as pr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=98_000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=2000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_pan.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
med = statistics.median
COUNT, PA = pr.MODE_COUNT, pr.MODE_PA
HBM_PEAK = 8e12


def device_body(rows, N, kw, mode, shape, seed):
    """made on the device -> uint8 tensor.  skewed: 60 % of the rows in one sample, 30 % in all, the rest in a random half"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rb = pr.row_bytes(kw, N, mode)
    t = torch.zeros(rows * rb, dtype=torch.uint8, device=dev)
    v = t.view(rows, rb)
    v[:, :8 * kw] = torch.randint(0, 256, (rows, 8 * kw), dtype=torch.uint8, device=dev, generator=g)
    u = torch.rand((rows, 1), device=dev, generator=g)
    x = torch.rand((rows, N), device=dev, generator=g)
    if shape == "skewed":
        one = torch.randint(0, N, (rows, 1), device=dev, generator=g)
        held = torch.where(u < 0.6, torch.arange(N, device=dev)[None, :] == one, torch.where(u < 0.9, torch.ones_like(x, dtype=torch.bool), x < 0.5))
    else:
        held = x < u      # the row's fill is uniform in [0, 1): every recurrence about as often
    if mode == COUNT:
        c = torch.randint(1, 50, (rows, N), dtype=torch.int32, device=dev, generator=g) * held
        v[:, 8 * kw:] = c.to(torch.int32).view(torch.uint8).view(rows, 4 * N)
    else:
        pad = (-N) % 8
        bits = torch.cat([held, torch.ones((rows, pad), dtype=torch.bool, device=dev)], dim=1).view(rows, -1, 8).to(torch.uint8)
        w = (2 ** torch.arange(8, device=dev)).to(torch.uint8)
        v[:, 8 * kw:] = (bits * w).sum(dim=2).to(torch.uint8)
    torch.cuda.synchronize()
    return t


def timed(call, parts):
    total, ps, algo = [], [], 0
    for step in range(a.warmup + a.steps):
        r = call()
        r.wait()
        if step >= a.warmup:
            total.append(r.kernel_ms()); algo = r.algo_bytes()
            if parts:
                ps.append(r.kernel_parts_ms())
        r.free()
    assert min(total) > 0, "profiling gave no time"
    return med(total), min(total), max(total), algo, [med(p[i] for p in ps) for i in range(3)] if parts else None


def main():
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    out, rows, N, kw = [], a.rows, 1000, 1
    for mode, mname in ((COUNT, "count"), (PA, "pa")):
        for shape in ("skewed", "uniform"):
            rb = pr.row_bytes(kw, N, mode)
            body = device_body(rows, N, kw, mode, shape, 31 + mode)
            cr = min(a.check_rows, rows)
            got = ctx.pan_dev(body.data_ptr(), cr, N, kw, mode, shared=True)
            exp = pr.pan_expected_np(body[:cr * rb].cpu().numpy(), N, kw, mode)
            assert got.spectrum.tobytes() == exp[0].tobytes() and got.shared.tobytes() == exp[1].tobytes(), f"{mname} {shape}: the first {cr} rows"
            c_ms, c_min, c_max, c_algo, _ = timed(lambda: ctx.colsums_dev(body.data_ptr(), rows, N, kw, mode, keep=True), False)
            s_ms, s_min, s_max, s_algo, _ = timed(lambda: ctx.pan_dev(body.data_ptr(), rows, N, kw, mode, keep=True), False)
            f_ms, f_min, f_max, f_algo, parts = timed(lambda: ctx.pan_dev(body.data_ptr(), rows, N, kw, mode, shared=True, keep=True), True)
            rec = dict(kernel="pan", mode=mname, shape=shape, n_cols=N, rows=rows, row_bytes=rb, body_bytes=rows * rb, steps=a.steps, warmup=a.warmup, checked_rows=cr,
                       colsums_ms=round(c_ms, 4), colsums_ms_min=round(c_min, 4), colsums_ms_max=round(c_max, 4), colsums_algo_bytes=c_algo,
                       spectrum_ms=round(s_ms, 4), spectrum_ms_min=round(s_min, 4), spectrum_ms_max=round(s_max, 4), spectrum_algo_bytes=s_algo,
                       spectrum_hbm_fraction=round(s_algo / (s_ms * 1e-3) / HBM_PEAK, 4),
                       shared_total_ms=round(f_ms, 4), shared_total_ms_min=round(f_min, 4), shared_total_ms_max=round(f_max, 4), shared_algo_bytes=f_algo,
                       shared_hbm_fraction=round(f_algo / (f_ms * 1e-3) / HBM_PEAK, 4),
                       score_ms=round(parts[0], 4), order_ms=round(parts[1], 4), shared_ms=round(parts[2], 4),
                       score_over_colsums=round(s_ms / c_ms, 3), all_over_two_colsums=round(f_ms / (2 * c_ms), 3))
            out.append(rec); print(json.dumps(rec), flush=True)
            del body
            torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
