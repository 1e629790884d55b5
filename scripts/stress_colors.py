"""Seeded random cases of kmx_colors_* against tests/colors_ref.py: the mode, N in 1 ... 2000, rows in 0 ... 5000, key words, the class
structure (one class, every row a class, skewed, two classes row by row, the last listed column alone, random), the list (left out,
reversed, a scattered subset, one column), min_abund, host or device-resident rows at any byte offset, and the signature cut to a few
bits (KMX_COLORS_HASH_BITS, on bodies of at most 700 rows).  ids, first rows, sizes and patterns are compared bit for bit and the
identities of the header are checked.  Needs the GPU (no fallback).
Usage: stress_colors.py [--cases 60] [--seed 1] [--seconds 240] [--out profiles/colors_stress.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import colors_ref as cr

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_colors.py needs the GPU")
dev = torch.device("cuda", 0); torch.cuda.init()


def main():
    ctx = lib.Context(0)
    rng = np.random.default_rng(a.seed)
    t0, done, failed = time.time(), [], []
    os.environ.pop("KMX_COLORS_HASH_BITS", None)
    for case in range(a.cases):
        if time.time() - t0 > a.seconds:
            break
        mode = int(rng.integers(0, 2))
        N = int(rng.choice([rng.integers(1, 132), rng.integers(1, 2001)]))
        rows = int(rng.choice([rng.integers(0, 300), rng.integers(0, 5001)]))
        rows = int(min(rows, 4_000_000 // N))
        kw = int(rng.integers(1, 5))
        structure = str(rng.choice(cr.STRUCTURES))
        kind = str(rng.choice(cr.KINDS))
        cols = cr.make_cols(kind, N, int(rng.integers(1 << 30)))
        M = N if cols is None else len(cols)
        amin = int(rng.choice([1, 2, 3, cr.U32])) if mode == cr.MODE_COUNT else 1
        body = cr.structured_body(int(rng.integers(1 << 30)), rows, N, kw, mode, structure, cols)
        exp = cr.colors_expected_np(body, N, kw, mode, cols, amin)
        resident, shift = bool(rng.integers(0, 2)), int(rng.integers(0, 8))
        bits = int(rng.choice([0, 1, 3, 8])) if rows <= 700 and exp[0] <= 300 and rng.integers(0, 2) else None
        if bits is not None:
            os.environ["KMX_COLORS_HASH_BITS"] = str(bits)
        if resident:
            buf = torch.zeros(len(body) + 8, dtype=torch.uint8, device=dev)
            buf[shift:shift + len(body)] = torch.from_numpy(np.array(body)).to(dev)
            torch.cuda.synchronize()
            out = ctx.colors_dev(buf.data_ptr() + shift, rows, N, kw, mode, cols=cols, min_abund=amin)
        else:
            out = ctx.colors(body, rows, N, kw, mode, cols=cols, min_abund=amin)
        os.environ.pop("KMX_COLORS_HASH_BITS", None)
        ok = (out.n_classes == exp[0] and out.ids.tobytes() == exp[1].tobytes() and out.first.tobytes() == exp[2].tobytes() and out.sizes.tobytes() == exp[3].tobytes()
              and out.patterns.tobytes() == exp[4].tobytes())
        if ok:
            cr.check_identities(out.n_classes, out.ids, out.first, out.sizes, out.patterns, rows, M, spectrum0=cr.pan_expected_np(body, N, kw, mode, cols, amin)[0][0])
        rec = dict(case=case, mode=["count", "pa"][mode], n_cols=N, n_use=M, cols=kind, rows=rows, key_words=kw, structure=structure, min_abund=amin, resident=resident,
                   shift=shift if resident else None, hash_bits=bits, classes=int(exp[0]), ok=bool(ok))
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
