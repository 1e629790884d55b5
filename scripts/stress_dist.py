"""Seeded random cases of kmx_dist_* against the numpy road of tests/dist_ref.py: mode (count with and without mins, pa, bf), N in
1 ... 3000, rows in 0 ... 20 000, fill, key words, the body cut into one to four calls that add into one device table, host or
device-resident rows at any byte offset.  Exact equality of the tables.  Needs the GPU (no fallback).
Usage: stress_dist.py [--cases 40] [--seed 1] [--seconds 240] [--out profiles/dist_stress.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import dist_ref as dr

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_dist.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()
WORK = 2e10      # rows * N^2 of a case: what the reference can afford


def main():
    ctx = lib.Context(0)
    rng = np.random.default_rng(a.seed)
    t0, done, failed = time.time(), [], []
    for case in range(a.cases):
        if time.time() - t0 > a.seconds:
            break
        mode = int(rng.choice([dr.MODE_COUNT, dr.MODE_PA, dr.MODE_BF]))
        mins = mode == dr.MODE_COUNT and bool(rng.integers(0, 2))
        N = int(rng.choice([rng.integers(1, 131), rng.integers(1, 3001)]))
        rows = int(rng.choice([rng.integers(0, 300), rng.integers(0, 20001)]))
        rows = int(min(rows, (WORK / 8 if mins else WORK) // (N * N)))
        kw = 0 if mode == dr.MODE_BF else int(rng.integers(1, 5))
        fill = float(rng.choice([0.0, 0.02, 0.3, 0.5, 1.0]))
        body = dr.make_body(int(rng.integers(1 << 30)), rows, N, kw, mode, fill, pad_ones=True, maxed=0.05)
        rb = dr.row_bytes(kw, N, mode)
        exp = dr.dist_expected_np(body, N, kw, mode, mins=mins, blas=True)
        n_calls = int(rng.integers(1, 5))
        cuts = [0] + sorted(int(x) for x in rng.integers(0, rows + 1, n_calls - 1)) + [rows]
        resident, shift = bool(rng.integers(0, 2)), int(rng.integers(0, 8))
        t_inter = torch.zeros(N * N, dtype=torch.int64, device=dev)
        t_mins = torch.zeros(N * N, dtype=torch.int64, device=dev) if mins else None
        torch.cuda.synchronize()
        for c in range(n_calls):
            part = body[cuts[c] * rb:cuts[c + 1] * rb]
            kwargs = dict(inter_dev=t_inter.data_ptr(), mins_dev=t_mins.data_ptr() if mins else None)
            if resident:
                buf = torch.zeros(len(part) + 8, dtype=torch.uint8, device=dev)
                buf[shift:shift + len(part)] = torch.from_numpy(part.copy()).to(dev)
                torch.cuda.synchronize()
                ctx.dist_dev(buf.data_ptr() + shift, cuts[c + 1] - cuts[c], N, kw, mode, **kwargs)
            else:
                ctx.dist(part, cuts[c + 1] - cuts[c], N, kw, mode, **kwargs)
        torch.cuda.synchronize()
        got_i = t_inter.cpu().numpy().view(np.uint64).reshape(N, N)
        ok = np.array_equal(got_i, exp[0]) and (not mins or np.array_equal(t_mins.cpu().numpy().view(np.uint64).reshape(N, N), exp[1]))
        rec = dict(case=case, mode=["count", "pa", "bf"][mode], mins=mins, n_cols=N, rows=rows, key_words=kw, fill=fill, cuts=cuts, resident=resident,
                   shift=shift if resident else None, ok=bool(ok))
        done.append(rec)
        if not ok:
            failed.append(rec)
        print(json.dumps(rec), flush=True)
    ctx.close()
    summary = dict(device=torch.cuda.get_device_name(0), seed=a.seed, cases=len(done), failed=len(failed), seconds=round(time.time() - t0, 1), runs=done)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
    print(json.dumps(dict(cases=len(done), failed=len(failed))))
    sys.exit(1 if failed else 0)


main()
