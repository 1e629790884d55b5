#!/usr/bin/env python3
"""A seeded random sweep of kmx_kquery_host against tests/kquery_ref.py: k, m, N, P, the mode, the share of the queries' own k-mers in
the index and of near misses among them, zero and saturated counts, the number and the lengths of the queries, Ns and lower case
sprinkled in, partitions left out of the call.  Exact equality of n_kmers, hits and (count rows) sums.

  python scripts/stress_kquery.py [--seed S] [--cases C] [--out profiles/kquery_stress.json]"""
import argparse, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kquery_stress.json"))
    a = ap.parse_args()
    from kmtricks_amd import lib
    import kquery_ref as kr
    rng = np.random.default_rng(a.seed)
    ctx = lib.Context(0)
    t0, failed, kmers = time.time(), [], 0
    for c in range(a.cases):
        k = int(rng.choice([8, 12, 21, 31, 32, 33, 48, 63, 64, 65, 96, 97, 127]))
        m = int(rng.integers(4, min(k, 12))) if k > 10 else int(rng.integers(4, k))
        mode = int(rng.choice([kr.MODE_COUNT, kr.MODE_PA]))
        N = int(rng.choice([1, 3, 8, 31, 32, 33, 64, 100, 257, 1000, 2049]))
        P = int(rng.choice([1, 2, 5, 32, 256]))
        seqs = []
        for _ in range(int(rng.integers(1, 40))):
            n = int(rng.choice([0, k - 1, k, k + 1, 63 + k, 64 + k, 150, 1000, 5000]))
            s = kr.random_reads(int(rng.integers(1 << 30)), 1, n, "ACGT" if rng.random() < 0.7 else "ACGTNacgt")[0] if n else ""
            seqs.append("A" * 40 + s if n > 100 and rng.random() < 0.3 else s)
        plain = [s.upper().replace("N", "A") for s in seqs]      # (the index's keys: the reads' k-mers and a few strangers' across the Ns)
        mats, rep = kr.synth_kindex(int(rng.integers(1 << 30)), N, P, k, m, mode, plain, float(rng.choice([0.0, 0.3, 0.9, 1.0])),
                                    near=float(rng.choice([0.0, 0.2, 0.5])), pad_ones=True, zeros=float(rng.choice([0.0, 0.3])), maxed=float(rng.choice([0.0, 0.1])))
        if rng.random() < 0.3:
            mats = [mt if rng.random() < 0.5 else None for mt in mats]
        en, eh, es = kr.kquery_expected_bulk(seqs, k, m, rep, N, mode, mats)
        out = ctx.kquery(seqs, k, m, rep, N, (k + 31) // 32, mode, mats, sums=mode == kr.MODE_COUNT)
        kmers += int(en.sum())
        if not (np.array_equal(out.n_kmers, en) and np.array_equal(out.hits, eh) and (mode == kr.MODE_PA or np.array_equal(out.sums, es))):
            failed.append(dict(case=c, k=k, m=m, N=N, P=P, mode=mode))
            print(f"case {c}: k={k} m={m} N={N} P={P} mode={mode} DIFFERS", flush=True)
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
