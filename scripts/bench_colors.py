"""kmx_colors_dev on device-resident bodies of the headline configuration's shape: 1000 count columns and about 100 000 rows a partition
(k = 31, one key word), and a presence/absence body of the same columns, in three class structures: skewed (60 % of the rows in one
class, 30 % in a second, every other row a class of its own), about 1000 classes of equal size, and every row distinct.  Per case: the
time of the call's kernels and of its three parts (pack; clearing + claim; the numbering kernels -- median of the timed calls after
warm-up, HIP events through kmx_set_profiling), the algorithmic bytes and their rate, and -- timed the same way in the same process --
the yardstick: kmx_colsums_dev on the same body, which reads the body once.  A subsample of every body is checked against
tests/colors_ref.py first.  Needs the GPU.
Usage: bench_colors.py [--rows 100000] [--steps 20] [--warmup 3] [--check-rows 2000] [--out profiles/colors_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import colors_ref as cr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=2000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_colors.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
med = statistics.median
COUNT, PA = cr.MODE_COUNT, cr.MODE_PA
HBM_PEAK = 8e12


def device_body(rows, N, kw, mode, structure, seed):
    """made on the device -> uint8 tensor"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rb = cr.row_bytes(kw, N, mode)
    t = torch.zeros(rows * rb, dtype=torch.uint8, device=dev)
    v = t.view(rows, rb)
    v[:, :8 * kw] = torch.randint(0, 256, (rows, 8 * kw), dtype=torch.uint8, device=dev, generator=g)
    x = torch.rand((rows, N), device=dev, generator=g) < 0.5      # every row distinct (2^-1000 says otherwise)
    if structure == "skewed":
        u = torch.rand((rows, 1), device=dev, generator=g)
        one = torch.zeros((1, N), dtype=torch.bool, device=dev); one[0, 17] = True      # private to one sample
        held = torch.where(u < 0.6, one, torch.where(u < 0.9, torch.ones_like(x), x))
    elif structure == "1000-classes":
        pool = torch.rand((1000, N), device=dev, generator=g) < 0.5
        held = pool[torch.arange(rows, device=dev) % 1000]
    else:
        held = x
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
        for structure in ("skewed", "1000-classes", "distinct"):
            rb = cr.row_bytes(kw, N, mode)
            body = device_body(rows, N, kw, mode, structure, 31 + mode)
            n = min(a.check_rows, rows)
            got = ctx.colors_dev(body.data_ptr(), n, N, kw, mode)
            exp = cr.colors_expected_np(body[:n * rb].cpu().numpy(), N, kw, mode)
            assert got.n_classes == exp[0] and got.ids.tobytes() == exp[1].tobytes() and got.patterns.tobytes() == exp[4].tobytes(), f"{mname} {structure}: the first {n} rows"
            whole = ctx.colors_dev(body.data_ptr(), rows, N, kw, mode)
            c_ms, c_min, c_max, c_algo, _ = timed(lambda: ctx.colsums_dev(body.data_ptr(), rows, N, kw, mode, keep=True), False)
            t_ms, t_min, t_max, t_algo, parts = timed(lambda: ctx.colors_dev(body.data_ptr(), rows, N, kw, mode, keep=True), True)
            rec = dict(kernel="colors", mode=mname, structure=structure, n_cols=N, rows=rows, classes=int(whole.n_classes), row_bytes=rb, body_bytes=rows * rb, steps=a.steps,
                       warmup=a.warmup, checked_rows=n,
                       colsums_ms=round(c_ms, 4), colsums_ms_min=round(c_min, 4), colsums_ms_max=round(c_max, 4), colsums_algo_bytes=c_algo,
                       colors_ms=round(t_ms, 4), colors_ms_min=round(t_min, 4), colors_ms_max=round(t_max, 4), colors_algo_bytes=t_algo,
                       colors_algo_gb_s=round(t_algo / (t_ms * 1e-3) / 1e9, 1), colors_hbm_fraction=round(t_algo / (t_ms * 1e-3) / HBM_PEAK, 4),
                       pack_ms=round(parts[0], 4), claim_ms=round(parts[1], 4), number_ms=round(parts[2], 4),
                       colors_over_colsums=round(t_ms / c_ms, 3), pack_over_colsums=round(parts[0] / c_ms, 3))
            out.append(rec); print(json.dumps(rec), flush=True)
            del body
            torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
