"""Seeded random cases of kmx_colsums_* and kmx_diff_* against tests/diff_ref.py: mode, N in 2 ... 2000, rows in 0 ... 5000, key words,
fill, groups drawn at random, the body cut into one to four colsums calls that add into one device table, host or device-resident rows
at any byte offset, thresholds 0, p = 0.05 and the middle between two neighbouring statistics at a random share, min_rec.  Column sums,
the integers of every record and the kept body exactly; the statistic within the derived tolerance of mpmath; the keep set exactly
outside the tolerance band (rows inside it are counted, not judged).  Needs the GPU (no fallback).
Usage: stress_diff.py [--cases 60] [--seed 1] [--seconds 240] [--out profiles/diff_stress.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import dist_ref as dr
import diff_ref as fr

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_diff.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()


def main():
    ctx = lib.Context(0)
    rng = np.random.default_rng(a.seed)
    t0, done, failed, worst = time.time(), [], [], 0.0
    for case in range(a.cases):
        if time.time() - t0 > a.seconds:
            break
        mode = int(rng.choice([fr.MODE_COUNT, fr.MODE_PA]))
        N = int(rng.choice([rng.integers(2, 132), rng.integers(2, 2001)]))
        rows = int(rng.choice([rng.integers(0, 300), rng.integers(0, 5001)]))
        rows = int(min(rows, 4_000_000 // N))
        kw = int(rng.integers(1, 5))
        fill = float(rng.choice([0.02, 0.3, 0.5, 1.0]))
        group = fr.random_groups(int(rng.integers(1 << 30)), N) if N > 2 else np.array([0, 1], np.uint8)
        body = fr.make_body(int(rng.integers(1 << 30)), rows, N, kw, mode, fill, pad_ones=True, maxed=0.05, group=group, effect=0.05)
        rb = dr.row_bytes(kw, N, mode)
        resident, shift = bool(rng.integers(0, 2)), int(rng.integers(0, 8))

        def on_device(part):
            buf = torch.zeros(len(part) + 8, dtype=torch.uint8, device=dev)
            buf[shift:shift + len(part)] = torch.from_numpy(np.array(part)).to(dev)
            torch.cuda.synchronize()
            return buf

        # the column sums, over cuts, into one table
        n_calls = int(rng.integers(1, 5))
        cuts = [0] + sorted(int(x) for x in rng.integers(0, rows + 1, n_calls - 1)) + [rows]
        table = torch.zeros(N, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for c in range(n_calls):
            part = body[cuts[c] * rb:cuts[c + 1] * rb]
            if resident:
                buf = on_device(part)
                ctx.colsums_dev(buf.data_ptr() + shift, cuts[c + 1] - cuts[c], N, kw, mode, sums_dev=table.data_ptr())
            else:
                ctx.colsums(part, cuts[c + 1] - cuts[c], N, kw, mode, sums_dev=table.data_ptr())
        torch.cuda.synchronize()
        sums = fr.colsums_np(body, N, kw, mode)
        ok = np.array_equal(table.cpu().numpy().view(np.uint64), sums)
        T0, T1 = fr.totals_of(sums, group)
        T0, T1 = T0 or int(rng.integers(1, 1 << 40)), T1 or int(rng.integers(1, 1 << 40))
        exp = fr.diff_expected_mixed(body, N, kw, mode, group, T0, T1)
        stats = sorted((float(x["stat"]) for x in exp), reverse=True)
        k = int(rng.integers(1, max(2, rows)))
        thrs = [0.0, fr.threshold(fr.P05)] + ([0.5 * (stats[k - 1] + stats[k])] if k < rows else [])
        min_rec = int(rng.choice([0, 1, 2, N // 4]))
        src = np.asarray(body).reshape(-1, rb) if rows else np.zeros((0, rb), np.uint8)
        in_band = 0
        buf = on_device(body) if resident else None
        for thr in thrs:
            if resident:
                out = ctx.diff_dev(buf.data_ptr() + shift, rows, N, kw, mode, group, T0, T1, thr, min_rec)
            else:
                out = ctx.diff(body, rows, N, kw, mode, group, T0, T1, thr, min_rec)
            kept, band = fr.keep_expected(exp, thr, min_rec)
            in_band += sum(band)
            got = set(out.recs["row"].tolist())
            ok = ok and all((i in got) == kept[i] for i in range(rows) if not band[i]) and got <= set(range(rows))
            ok = ok and bool((np.diff(out.recs["row"].astype(np.int64)) > 0).all()) and out.body == src[out.recs["row"]].tobytes()
            for q in out.recs:
                x = exp[int(q["row"])]
                ok = ok and (int(q["sum_ctrl"]), int(q["sum_case"]), int(q["rec_ctrl"]), int(q["rec_case"]), int(q["over"])) == (x["c0"], x["c1"], x["r0"], x["r1"], x["over"])
                err = abs(x["stat"] - float(q["stat"]))
                ok = ok and err <= x["tol"]
                if x["tol"]:
                    worst = max(worst, float(err / x["tol"]) * 16)
        rec = dict(case=case, mode=["count", "pa"][mode], n_cols=N, rows=rows, key_words=kw, fill=fill, cuts=cuts, resident=resident,
                   shift=shift if resident else None, thresholds=thrs, min_rec=min_rec, rows_in_band=in_band, ok=bool(ok))
        done.append(rec)
        if not ok:
            failed.append(rec)
        print(json.dumps(rec), flush=True)
    ctx.close()
    summary = dict(device=torch.cuda.get_device_name(0), seed=a.seed, cases=len(done), failed=len(failed), seconds=round(time.time() - t0, 1),
                   worst_stat_error_units=round(worst, 3), tolerance_units=16, runs=done)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
    print(json.dumps(dict(cases=len(done), failed=len(failed), worst_stat_error_units=round(worst, 3))))
    sys.exit(1 if failed else 0)


main()
