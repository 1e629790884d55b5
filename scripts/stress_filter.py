"""Randomised parity of kmx_filter_host against tests/filter_ref.py (the definition of `kmx filter` restated with a dictionary and a
set) over everything the filter takes: keys of one to four words over the whole width (tests/synth.py's shapes), count and PA rows,
1 to 5000 columns, matrices from empty to 60 000 rows, key lists far denser and far sparser than the rows, any share of the rows
kept, counts of 2^32 - 1, every subset of the outputs, the partition whole or in runs of rows with the marks carried over.
Usage: stress_filter.py [--cases N] [--seed S] (or N S as positional arguments); exit status 1 at the first difference."""
import os, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import filter_ref as fr
from synth import SHAPES
from kmtricks_amd import lib

args, pos = {"--cases": 40, "--seed": 1}, []
it = iter(sys.argv[1:])
for a in it:
    if a in args: args[a] = int(next(it))
    else: pos.append(int(a))
n_cases = pos[0] if pos else args["--cases"]
seed = pos[1] if len(pos) > 1 else args["--seed"]
rng = random.Random(seed)
ctx = lib.Context(0)
for case in range(n_cases):
    mode = rng.choice([fr.MODE_COUNT, fr.MODE_PA]); kw = rng.choice([1, 1, 2, 3, 4])
    n_cols = rng.choice([1, 2, 7, 8, 9, 31, 64, 100, 255, 1000, 5000])
    n_rows = rng.choice([0, 1, 2, 255, 256, 257, 3000, 60000]) if n_cols <= 100 else rng.choice([0, 1, 257, 1500])
    keep = rng.choice([0.0, 0.01, 0.3, 0.5, 0.99, 1.0]); ratio = rng.choice([0.0, 0.1, 1.0, 1.0, 3.0, 12.0])
    shape = rng.choice(SHAPES); want = rng.choice(["k", "m", "v", "km", "kv", "mv", "kmv", "kmv"])
    run = rng.choice([0, 0, 1, 100, 1000])
    print(f"case {case}: mode={mode} kw={kw} N={n_cols} rows={n_rows} keep={keep} ratio={ratio} keys={shape} want={want} run={run} ...", flush=True)
    row_keys, payload, key_keys, key_counts = fr.synth_case(rng.randrange(1 << 30), n_rows, n_cols, kw, mode, keep, ratio, shape, extreme=rng.random() < 0.3)
    em, ev, eak, eac = fr.filter_expected(row_keys, payload, key_keys, key_counts, mode)
    if run and len(row_keys) > run and len(row_keys) / run <= 300:
        marks = np.zeros(len(key_counts), np.uint8)
        starts = list(range(0, len(row_keys), run)); bodies, vecs = [], []
        for s in starts:
            out = ctx.filter(fr.matrix_body(row_keys[s:s + run], payload[s:s + run]), n_cols, kw, mode, (key_keys, key_counts),
                             want if s == starts[-1] else (want.replace("k", "") or "v"), marks=marks)
            bodies.append(out.body)
            if "v" in want: vecs.append(out.vector)
        body, vec = b"".join(bodies), np.concatenate(vecs) if vecs else np.zeros(0, np.uint32)
    else:
        out = ctx.filter(fr.matrix_body(row_keys, payload), n_cols, kw, mode, (key_keys, key_counts), want)
        body, vec = out.body, out.vector
    ok_m = body == (em if "m" in want else b"")
    ok_v = np.array_equal(vec, ev if "v" in want else np.zeros(0, np.uint32))
    ok_k = np.array_equal(out.absent_keys, eak if "k" in want else eak[:0]) and np.array_equal(out.absent_counts, eac if "k" in want else eac[:0])
    if not (ok_m and ok_v and ok_k):
        print("MISMATCH m", ok_m, "v", ok_v, "k", ok_k); sys.exit(1)
print("all", n_cases, "cases equal the restatement")
