"""Seeded random cases of kmx_gram_* against tests/gram_ref.py: the mode, N in 1 ... 1200, rows in 0 ... 5000, key words, the recurrence
shape (skewed, uniform, one class, all-zero rows, a fill), the list (left out, reversed, a scattered subset, one column), the weights
(all 1, all 2^32 - 1, zero for some classes, the driver's own, dist's), min_abund, host or device-resident rows at any byte offset, one
call or two calls over a cut into the caller's table, the launch knobs set or not.  The table is compared bit for bit.  Needs the GPU
(no fallback).
Usage: stress_gram.py [--cases 60] [--seed 1] [--seconds 240] [--out profiles/gram_stress.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import gram_ref as gr

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_gram.py needs the GPU")
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
        kind = str(rng.choice(gr.KINDS))
        cols = gr.make_cols(kind, N, int(rng.integers(1 << 30)))
        M = N if cols is None else len(cols)
        wkind = str(rng.choice(gr.WEIGHTS))
        w = gr.make_weights(wkind, M, int(rng.integers(1 << 30)))
        amin = int(rng.choice([1, 2, 3, gr.U32])) if mode == gr.MODE_COUNT else 1
        body = gr.shaped_body(int(rng.integers(1 << 30)), rows, N, kw, mode, shape)
        exp = gr.gram_expected_np(body, N, kw, mode, w, cols, amin)
        resident, shift, two = bool(rng.integers(0, 2)), int(rng.integers(0, 8)), bool(rng.integers(0, 2)) and rows > 1
        knobs = [dict(), dict(KMX_GRAM_CUS="1"), dict(KMX_GRAM_GRID=str(int(rng.integers(1, 9)))), dict(KMX_GRAM_CUS="2", KMX_GRAM_GRID="5")][int(rng.integers(0, 4))]
        rb = gr.row_bytes(kw, N, mode)
        cuts = [0, int(rng.integers(1, rows)), rows] if two else [0, rows]
        d_t = torch.zeros((N, N), dtype=torch.int64, device=dev)
        buf = torch.zeros(len(body) + 8, dtype=torch.uint8, device=dev)
        buf[shift:shift + len(body)] = torch.from_numpy(np.array(body)).to(dev)
        torch.cuda.synchronize()
        os.environ.update(knobs)
        for r0, r1 in zip(cuts, cuts[1:]):
            args = dict(cols=cols, min_abund=amin, table_dev=d_t.data_ptr())
            if resident:
                ctx.gram_dev(buf.data_ptr() + shift + r0 * rb, r1 - r0, N, kw, mode, w, **args)
            else:
                ctx.gram(body[r0 * rb:r1 * rb], r1 - r0, N, kw, mode, w, **args)
        for k in knobs:
            del os.environ[k]
        torch.cuda.synchronize()
        ok = d_t.cpu().numpy().view(np.uint64).tobytes() == exp.tobytes()
        rec = dict(case=case, mode=["count", "pa"][mode], n_cols=N, n_use=M, cols=kind, rows=rows, key_words=kw, shape=shape, weights=wkind, min_abund=amin,
                   resident=resident, shift=shift if resident else None, calls=len(cuts) - 1, knobs=knobs,
                   classes=int((gr.class_sizes(body, N, kw, mode, cols, amin) > 0).sum()), ok=bool(ok))
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
