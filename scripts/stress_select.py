"""Seeded random cases of kmx_select_* against tests/select_ref.py: the pair of modes, N in 1 ... 2000, rows in 0 ... 5000, key words,
fill, the column list (left out, the identity, reversed, a permutation cut at a random M), min_abund, the recurrence range, ZERO_BELOW,
host or device-resident rows at any byte offset.  The kept body and every record are compared exactly.  Needs the GPU (no fallback).
Usage: stress_select.py [--cases 60] [--seed 1] [--seconds 240] [--out profiles/select_stress.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import select_ref as sr

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_select.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()


def main():
    ctx = lib.Context(0)
    rng = np.random.default_rng(a.seed)
    t0, done, failed = time.time(), [], []
    for case in range(a.cases):
        if time.time() - t0 > a.seconds:
            break
        mode, out_mode = sr.MODE_PAIRS[int(rng.integers(0, 3))]
        N = int(rng.choice([rng.integers(1, 132), rng.integers(1, 2001)]))
        rows = int(rng.choice([rng.integers(0, 300), rng.integers(0, 5001)]))
        rows = int(min(rows, 4_000_000 // N))
        kw = int(rng.integers(1, 5))
        fill = float(rng.choice([0.0, 0.02, 0.3, 0.5, 1.0]))
        kind = str(rng.choice(["none", "identity", "reversed", "perm", "perm", "one"]))
        M = int(rng.integers(1, N + 1))
        cols = sr.make_cols(kind, N, M, int(rng.integers(1 << 30)))
        M = N if cols is None else len(cols)
        amin = int(rng.choice([1, 2, 3, sr.U32])) if mode == sr.MODE_COUNT else 1
        lo, hi = [(0, None), (1, None), (M, M), (1, M - 1), (2, 1), (int(rng.integers(0, M + 1)), int(rng.integers(0, M + 2)))][int(rng.integers(0, 6))]
        zb = bool(rng.integers(0, 2)) and out_mode == sr.MODE_COUNT
        body = sr.make_body(int(rng.integers(1 << 30)), rows, N, kw, mode, fill=fill, pad_ones=True, maxed=0.05, lo=1, hi=5)
        args = dict(out_mode=out_mode, min_abund=amin, min_rec=lo, max_rec=hi, zero_below=zb)
        exp_body, exp_recs = sr.select_expected_np(body, N, kw, mode, cols, **args)
        resident, shift = bool(rng.integers(0, 2)), int(rng.integers(0, 8))
        if resident:
            buf = torch.zeros(len(body) + 8, dtype=torch.uint8, device=dev)
            buf[shift:shift + len(body)] = torch.from_numpy(np.array(body)).to(dev)
            torch.cuda.synchronize()
            out = ctx.select_dev(buf.data_ptr() + shift, rows, N, kw, mode, cols=cols, **args)
        else:
            out = ctx.select(body, rows, N, kw, mode, cols=cols, **args)
        ok = out.body == exp_body and out.recs.tobytes() == exp_recs.tobytes()
        rec = dict(case=case, mode=["count", "pa"][mode], out_mode=["count", "pa"][out_mode], n_cols=N, n_out=M, cols=kind, rows=rows, key_words=kw, fill=fill,
                   min_abund=amin, min_rec=lo, max_rec=hi, zero_below=zb, resident=resident, shift=shift if resident else None, kept=len(exp_recs), ok=bool(ok))
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
    print(json.dumps(dict(cases=len(done), failed=len(failed), equal=len(done) - len(failed))))
    sys.exit(1 if failed else 0)


main()
