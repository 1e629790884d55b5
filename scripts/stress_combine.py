"""Randomised parity of kmx_combine_host against tests/combine_ref.py (the definition of `kmx combine` restated with a dictionary)
over everything a combine takes: 1 to 64 blocks, keys of one to four words over the whole width (tests/synth.py's shapes), count
blocks of 1-, 2- and 4-byte counts and PA blocks, 1 to 5000 columns a block, blocks from empty to 30 000 rows and ten times apart
in length, any share of shared keys, counts at the maximum of their width, with and without KMX_COMBINE_DROP_LAST.
Usage: stress_combine.py [--cases N] [--seed S] (or N S as positional arguments); exit status 1 at the first difference."""
import os, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import combine_ref as cr
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
    mode = rng.choice([cr.MODE_COUNT, cr.MODE_PA]); kw = rng.choice([1, 1, 2, 3, 4])
    B = rng.choice([1, 2, 2, 3, 5, 8, 33, 64])
    wide = B <= 3 and rng.random() < 0.4
    cols = [rng.choice([1, 7, 8, 9, 200, 1000, 5000] if wide else [1, 1, 2, 7, 8, 9, 31, 64]) for _ in range(B)]
    base = rng.choice([0, 1, 2, 255, 256, 257, 3000]) if wide or B > 8 else rng.choice([0, 1, 257, 3000, 30000])
    rows = [rng.choice([base, base, base // 10, min(base * 10, 30000), 0]) for _ in range(B)]
    cbs = [rng.choice([1, 2, 4, 4]) for _ in range(B)]
    share = rng.choice([0.0, 0.01, 0.3, 0.5, 0.99, 1.0]); shape = rng.choice(SHAPES); drop = rng.random() < 0.5
    print(f"case {case}: mode={mode} kw={kw} B={B} cols={cols} rows={rows} bytes={cbs} share={share} keys={shape} drop_last={drop} ...", flush=True)
    blocks = cr.synth_case(rng.randrange(1 << 30), rows, cols, kw, mode, share, shape, cbs, extreme=rng.random() < 0.3)
    exp, n = cr.combine_expected(blocks, kw, mode, drop)
    out = ctx.combine([(cr.block_body(b[0], b[1]), b[2], b[3]) for b in blocks], kw, mode, drop)
    if out.rows != n or out.body != exp:
        print("MISMATCH rows", out.rows, "expected", n, "bytes equal:", out.body == exp); sys.exit(1)
print("all", n_cases, "cases equal the restatement")
