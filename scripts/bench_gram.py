"""kmx_gram_dev on device-resident bodies: 100 000 rows of 1000 count columns at k = 31 (one key word), and of 500 presence/absence
columns at k = 63 (two key words) -- with the rows of a real matrix's shape (most rows private or core) and with every recurrence as
often as any other (the most classes, so the most padding of the order and the most changes of weight in k_gram_pairs).  The weights are
the driver's own (eigenstrat, F = 8).  Per case: the time of the call's kernels by part (score + fold, order, slab, pairs; median of the
timed calls after warm-up, HIP events through kmx_set_profiling), the algorithmic bytes and their rate, and -- timed the same way in the
same process -- two yardsticks: kmx_dist_dev on the same body (the unweighted table, slab + pairs: what the ordering and the multiply
cost on top of it) and a device-to-device copy of the call's algorithmic bytes.  Recorded: gram : dist and gram : copy.  No speed target
is set: the numbers are the record.  A subsample of every body is checked against tests/gram_ref.py first.  Needs the GPU.
Usage: bench_gram.py [--rows 100000] [--steps 20] [--warmup 3] [--check-rows 2000] [--out profiles/gram_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import gram_ref as gr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=2000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_gram.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
med = statistics.median
COUNT, PA = gr.MODE_COUNT, gr.MODE_PA


def device_body(rows, N, kw, mode, shape, seed):
    """made on the device -> uint8 tensor.  skewed: 60 % of the rows in one sample, 30 % in all, the rest in a random half"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    rb = gr.row_bytes(kw, N, mode)
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


def timed(call, n_parts):
    total, ps, algo = [], [], 0
    for step in range(a.warmup + a.steps):
        r = call()
        r.wait()
        if step >= a.warmup:
            total.append(r.kernel_ms()); algo = r.algo_bytes()
            ps.append(r.kernel_parts_ms())
        r.free()
    assert min(total) > 0, "profiling gave no time"
    return med(total), min(total), max(total), algo, [med(p[i] for p in ps) for i in range(n_parts)]


def timed_copy(n_bytes):
    """a device-to-device copy that moves n_bytes in all (half read, half written), by HIP events"""
    src = torch.empty(n_bytes // 2, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    ms = []
    for step in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        if step >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    return med(ms)


def main():
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    out, rows = [], a.rows
    for mode, mname, N, kw, k in ((COUNT, "count", 1000, 1, 31), (PA, "pa", 500, 2, 63)):
        for shape in ("skewed", "uniform"):
            rb = gr.row_bytes(kw, N, mode)
            body = device_body(rows, N, kw, mode, shape, 41 + mode)
            w = gr.make_weights("eigenstrat", N)
            cr = min(a.check_rows, rows)
            got = ctx.gram_dev(body.data_ptr(), cr, N, kw, mode, w)
            exp = gr.gram_expected_np(body[:cr * rb].cpu().numpy(), N, kw, mode, w)
            assert got.table.tobytes() == exp.tobytes(), f"{mname} {shape}: the first {cr} rows"
            d_ms, d_min, d_max, d_algo, dparts = timed(lambda: ctx.dist_dev(body.data_ptr(), rows, N, kw, mode, keep=True), 2)
            g_ms, g_min, g_max, g_algo, parts = timed(lambda: ctx.gram_dev(body.data_ptr(), rows, N, kw, mode, w, keep=True), 4)
            c_ms = timed_copy(g_algo)
            rec = dict(kernel="gram", mode=mname, shape=shape, k=k, n_cols=N, rows=rows, row_bytes=rb, body_bytes=rows * rb, steps=a.steps, warmup=a.warmup, checked_rows=cr,
                       gram_ms=round(g_ms, 4), gram_ms_min=round(g_min, 4), gram_ms_max=round(g_max, 4), gram_algo_bytes=g_algo,
                       gram_gb_per_s=round(g_algo / (g_ms * 1e-3) / 1e9, 1),
                       score_ms=round(parts[0], 4), order_ms=round(parts[1], 4), slab_ms=round(parts[2], 4), pairs_ms=round(parts[3], 4),
                       dist_ms=round(d_ms, 4), dist_ms_min=round(d_min, 4), dist_ms_max=round(d_max, 4), dist_algo_bytes=d_algo,
                       dist_slab_ms=round(dparts[0], 4), dist_pairs_ms=round(dparts[1], 4),
                       copy_ms=round(c_ms, 4), gram_over_dist=round(g_ms / d_ms, 3), gram_over_copy=round(g_ms / c_ms, 3))
            out.append(rec); print(json.dumps(rec), flush=True)
            del body
            torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
