#!/usr/bin/env python3
"""A seeded random sweep of kmx_zquery_host against tests/zquery_ref.py (the numpy road): k, z, m, N, W, P, the fill of the matrices,
the number and the lengths of the queries, Ns and lower case sprinkled in, partitions left out of every call, and the partitions dealt
into one to three calls of a series.  Exact equality of n_kmers and hits.

  python scripts/stress_zquery.py [--seed S] [--cases C] [--out profiles/zquery_stress.json]"""
import argparse, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zquery_stress.json"))
    a = ap.parse_args()
    from kmtricks_amd import lib
    import query_ref as qr
    import zquery_ref as zr
    rng = np.random.default_rng(a.seed)
    ctx = lib.Context(0)
    t0, failed, windows, calls = time.time(), [], 0, 0
    for c in range(a.cases):
        k = int(rng.choice([8, 12, 21, 31, 32, 33, 48, 63, 64, 65, 96, 97, 127]))
        z = int(rng.integers(0, min(8, k - 1) + 1))
        m = int(rng.integers(4, min(k, 12))) if k > 10 else int(rng.integers(4, k))
        N = int(rng.choice([1, 3, 8, 31, 32, 33, 64, 100, 257, 1000, 2049]))
        W = int(rng.choice([1, 7, 256, 4099, 65521]))
        P = int(rng.choice([1, 2, 5, 32, 256]))
        if P == 256:
            W = min(W, 4099)      # (256 matrices of 65521 rows take longer to draw than to query)
        K = k + z
        mats, rep = qr.synth_index(int(rng.integers(1 << 30)), N, W, P, k, m, float(rng.choice([0.3, 0.8, 0.95])), pad_ones=True)
        if rng.random() < 0.3:
            mats = [mt if rng.random() < 0.5 else None for mt in mats]
        seqs = []
        for _ in range(int(rng.integers(1, 40))):
            n = int(rng.choice([0, k - 1, K - 1, K, K + 1, 63 + K, 64 + K, 150, 1000, 5000]))
            s = qr.random_reads(int(rng.integers(1 << 30)), 1, n, "ACGT" if rng.random() < 0.7 else "ACGTNacgt" + "ACGT" * 6)[0] if n else ""
            seqs.append(s)
        en, eh = zr.zquery_expected_np(seqs, k, z, m, rep, W, N, mats)
        n_calls = int(rng.integers(1, 4))
        deal = rng.integers(0, n_calls, P)
        first = out = None
        try:
            for g in range(n_calls):
                mm = [mt if deal[p] == g else None for p, mt in enumerate(mats)]
                r = ctx.zquery(seqs, k, m, rep, W, N, mm, z, bits_dev=first.bits_dev() if first else None, last=g == n_calls - 1, keep=first is None)
                calls += 1
                if first is None:
                    first = r
                if g == n_calls - 1:
                    out = first.output() if n_calls == 1 else r
        finally:
            if first is not None:
                first.free()
        windows += int(en.sum())
        if not (np.array_equal(out.n_kmers, en) and np.array_equal(out.hits, eh)):
            failed.append(dict(case=c, k=k, z=z, m=m, N=N, W=W, P=P, calls=n_calls))
            print(f"case {c}: k={k} z={z} m={m} N={N} W={W} P={P} calls={n_calls} DIFFERS", flush=True)
    ctx.close()
    res = dict(seed=a.seed, cases=a.cases, failed=failed, calls=calls, windows=windows, seconds=round(time.time() - t0, 1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
