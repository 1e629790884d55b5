"""Seeded random cases of kmx_assoc_* against tests/assoc_ref.py: the mode, N in 1 ... 1200, rows in 0 ... 5000, key words, the recurrence
shape (skewed, uniform, one class, all-zero rows, a fill), the list (left out, a permuted subset, one column, every second column), V in
1 ... 32, the vectors (random, all +2^30, all -2^30, alternating, zero), min_abund, the threshold (0, +inf, the median statistic), the
recurrence window, vmin, host or device-resident rows at any byte offset, the launch knobs set or not.  Kept rows, rec and s0 exactly,
stat and beta bit for bit, the kept body byte for byte.  Needs the GPU (no fallback).
Usage: stress_assoc.py [--cases 60] [--seed 1] [--seconds 240] [--out profiles/assoc_stress.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import assoc_ref as ar

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_assoc.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()


def main():
    ctx = lib.Context(0)
    rng = np.random.default_rng(a.seed)
    t0, done, failed = time.time(), [], []
    for case in range(a.cases):
        if time.time() - t0 > a.seconds:
            break
        mode = int(rng.integers(0, 2))
        N = int(rng.choice([rng.integers(1, 132), rng.integers(1, 1201)]))
        rows = int(rng.choice([rng.integers(0, 300), rng.integers(0, 5001)]))
        rows = int(min(rows, 2_000_000 // N))
        kw = int(rng.integers(1, 5))
        shape = [0.02, 0.3, 1.0, "skewed", "uniform", "same", "zero"][int(rng.integers(0, 7))]
        kind = str(rng.choice(ar.KINDS))
        cols = ar.make_cols(kind, N, int(rng.integers(1 << 30)))
        M = N if cols is None else len(cols)
        V = int(rng.integers(1, 33))
        vkind = str(rng.choice(ar.VKINDS))
        vecs = ar.make_vecs(vkind, M, V, int(rng.integers(1 << 30)))
        amin = int(rng.choice([1, 2, 3, ar.U32])) if mode == ar.MODE_COUNT else 1
        vmin = [2.0 ** -10, 0.0, float(M + 1)][int(rng.integers(0, 3))]
        lo, hi = [(0, ar.U32), (1, max(1, M - 1)), (M // 2 + 1, M // 2), (0, M // 2)][int(rng.integers(0, 4))]
        body = ar.shaped_body(int(rng.integers(1 << 30)), rows, N, kw, mode, shape)
        allr = ar.assoc_rows_np(body, N, kw, mode, vecs, 30, 3.7, vmin, cols, amin)
        tk = str(rng.choice(["zero", "inf", "median"]))
        thr = 0.0 if tk == "zero" or rows == 0 else ar.INF if tk == "inf" else float(np.sort(allr["stat"])[rows // 2])
        exp = ar.assoc_expected_np(body, N, kw, mode, vecs, 30, 3.7, vmin, thr, cols, amin, lo, hi)
        resident, shift = bool(rng.integers(0, 2)), int(rng.integers(0, 8))
        knobs = [dict(), dict(KMX_ASSOC_CUS="1"), dict(KMX_ASSOC_GRID=str(int(rng.integers(1, 9)))), dict(KMX_ASSOC_CUS="2", KMX_ASSOC_GRID="5")][int(rng.integers(0, 4))]
        args = dict(vecs=vecs, frac_bits=30, gain=3.7, vmin=vmin, threshold=thr, cols=cols, min_abund=amin, min_rec=lo, max_rec=hi)
        os.environ.update(knobs)
        if resident:
            buf = torch.zeros(len(body) + 8, dtype=torch.uint8, device=dev)
            buf[shift:shift + len(body)] = torch.from_numpy(np.array(body)).to(dev)
            torch.cuda.synchronize()
            out = ctx.assoc_dev(buf.data_ptr() + shift, rows, N, kw, mode, **args)
        else:
            out = ctx.assoc(body, rows, N, kw, mode, **args)
        for k in knobs:
            del os.environ[k]
        ok = out.body == exp[1] and out.recs.tobytes() == exp[0].tobytes() and out.algo_bytes == ar.algo_bytes(rows, N, kw, mode, V, len(exp[0]))
        rec = dict(case=case, mode=["count", "pa"][mode], n_cols=N, n_use=M, cols=kind, rows=rows, key_words=kw, shape=shape, n_vec=V, vecs=vkind, min_abund=amin,
                   vmin=vmin, threshold=tk, window=[lo, hi], resident=resident, shift=shift if resident else None, knobs=knobs, kept=len(exp[0]), ok=bool(ok))
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
