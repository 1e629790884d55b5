#!/usr/bin/env python3
"""A seeded random sweep of kmx_cquery_host against tests/cquery_ref.py: k, m, N, W, P, the field width, min_class, the kind of body,
the number and the lengths of the queries, Ns and lower case sprinkled in, partitions left out of the call.  Exact equality of n_kmers,
hits and sums.  A call that fails (a GPU fault included) ends the script: nothing is tried again.

  python scripts/stress_cquery.py [--seed S] [--cases C] [--out profiles/cquery_stress.json]"""
import argparse, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cquery_stress.json"))
    a = ap.parse_args()
    from kmtricks_amd import lib
    import query_ref as qr
    import cquery_ref as cr
    rng = np.random.default_rng(a.seed)
    ctx = lib.Context(0)
    t0, failed, kmers = time.time(), [], 0
    for c in range(a.cases):
        k = int(rng.choice([8, 12, 21, 31, 32, 33, 48, 63, 64, 65, 96, 97, 127]))
        m = int(rng.integers(4, min(k, 12))) if k > 10 else int(rng.integers(4, k))
        N = int(rng.choice([1, 3, 8, 9, 31, 64, 65, 100, 257, 512, 513, 1000, 2049]))
        W = int(rng.choice([1, 7, 256, 4099, 65521]))
        P = int(rng.choice([1, 2, 5, 32, 256]))
        w = int(rng.integers(1, 9))
        while W * P * ((N * w + 7) // 8) > (1 << 28):      # (the index stays below 256 MB)
            P = max(1, P // 2)
        mc = int(rng.choice([1, min(2, (1 << w) - 1), (1 << w) - 1]))
        dist = ("uniform", "uniform", "uniform", "zero", "ones", 1, (1 << w) - 1)[int(rng.integers(7))]
        mats, rep = cr.synth_index_bfc(int(rng.integers(1 << 30)), N, W, P, k, m, w, pad_ones=True, dist=dist)
        if rng.random() < 0.3:
            mats = [mt if rng.random() < 0.5 else None for mt in mats]
        seqs = []
        for _ in range(int(rng.integers(1, 40))):
            n = int(rng.choice([0, k - 1, k, k + 1, 63 + k, 64 + k, 150, 1000, 5000]))
            s = qr.random_reads(int(rng.integers(1 << 30)), 1, n, "ACGT" if rng.random() < 0.7 else "ACGTNacgt")[0] if n else ""
            seqs.append(s)
        en, eh, es = cr.cquery_expected_np(seqs, k, m, rep, W, N, mats, w, mc)
        out = ctx.cquery(seqs, k, m, rep, W, N, mats, w, min_class=mc)      # (an error here ends the sweep)
        kmers += int(en.sum())
        if not (np.array_equal(out.n_kmers, en) and np.array_equal(out.hits, eh) and np.array_equal(out.sums, es)):
            failed.append(dict(case=c, k=k, m=m, N=N, W=W, P=P, w=w, min_class=mc, dist=str(dist)))
            print(f"case {c}: k={k} m={m} N={N} W={W} P={P} w={w} min_class={mc} dist={dist} DIFFERS", flush=True)
    ctx.close()
    res = dict(seed=a.seed, cases=a.cases, failed=failed, kmers=kmers, seconds=round(time.time() - t0, 1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
