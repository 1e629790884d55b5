"""Seeded random sets and reads through kmx_kset_* / kmx_match_* against road A of tests/match_ref.py: k in 8 ... 127; reads of random
lengths (empty ones, ones shorter than k, N and lower case) that carry pieces of the set's source on either strand; sets with duplicates,
with keys no read holds, empty sets; host or device-resident inputs; ids and occurrences on or off; the hash cut to a few bits
(KMX_MATCH_HASH_BITS, on sets of at most 400 keys) and the launch knobs.  The keys' ids, every record, id and occurrence count are compared
bit for bit.  Needs the GPU (no fallback).
Usage: stress_match.py [--cases 40] [--seed 1] [--seconds 240] [--out profiles/match_stress.json]"""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import match_ref as mr

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_match.py needs the GPU")
torch.cuda.init()
KNOBS = ("KMX_MATCH_HASH_BITS", "KMX_MATCH_CUS", "KMX_MATCH_GRID")


def make_case(rng):
    k = rng.choice(mr.K_SWEEP + (rng.randrange(8, 128),))
    src = [mr.rand_seq(rng, rng.randrange(k, 1500)) for _ in range(rng.randrange(1, 5))]
    reads = []
    for _ in range(rng.randrange(0, 120)):
        kind = rng.randrange(6)
        s = mr.rand_seq(rng, rng.randrange(0, 300))
        if kind >= 2:
            p = rng.choice(src)
            b = rng.randrange(len(p))
            p = p[b:b + rng.randrange(1, 3 * k)]
            p = mr.rc_str(p) if kind == 3 else p.lower() if kind == 4 else p
            s = s[:len(s) // 2] + p + ("N" if kind == 5 else "") + s[len(s) // 2:]
        reads.append("" if kind == 0 and rng.random() < 0.3 else s)
    keys = mr.kmers_of(src, k)
    keys = rng.sample(keys, rng.randrange(0, len(keys) + 1)) if rng.random() < 0.8 else []
    keys += [rng.choice(keys) for _ in range(rng.randrange(0, 40))] if keys else []
    keys += mr.kmers_of([mr.rand_seq(rng, k + rng.randrange(0, 20))], k) if rng.random() < 0.5 else []
    rng.shuffle(keys)
    return k, keys, reads


def main():
    ctx = lib.Context(0)
    rng = random.Random(a.seed)
    t0, done, diffs, log = time.time(), 0, [], []
    for case in range(a.cases):
        if time.time() - t0 > a.seconds:
            break
        k, keys, reads = make_case(rng)
        for kn in KNOBS:
            os.environ.pop(kn, None)
        knobs = {}
        if len(keys) <= 400 and rng.random() < 0.4:
            knobs["KMX_MATCH_HASH_BITS"] = str(rng.choice([0, 1, 3, 6]))
        if rng.random() < 0.3:
            knobs[rng.choice(KNOBS[1:])] = str(rng.choice([1, 2, 7]))
        os.environ.update(knobs)
        want_ids, want_occ, on_dev = rng.random() < 0.7, rng.random() < 0.7, rng.random() < 0.5
        exp = mr.match_strings(keys, k, reads)
        words = mr.keys_to_words(keys, k)
        hold = []
        if on_dev and keys:
            dk = torch.from_numpy(words.view(np.int64).copy().reshape(-1)).to("cuda:0"); hold.append(dk)
            torch.cuda.synchronize()
            s = ctx.kset_dev(dk.data_ptr(), len(keys), k)
        else:
            s = ctx.kset(words, k)
        bad = []
        try:
            if s.ids().tolist() != exp.key_ids or s.n_distinct != exp.n_distinct:
                bad.append("key ids")
            if on_dev:
                blob, offs = ctx.pack_reads(reads)
                db = torch.from_numpy(np.frombuffer(blob if blob else b"N", np.uint8).copy()).to("cuda:0")
                do = torch.from_numpy(offs.view(np.int64).copy()).to("cuda:0")
                torch.cuda.synchronize()
                out = ctx.match_dev(s, db.data_ptr(), do.data_ptr(), len(reads), ids=want_ids, occ=want_occ)
            else:
                out = ctx.match(s, reads, ids=want_ids, occ=want_occ)
            if [tuple(int(x) for x in r) for r in out.recs.tolist()] != exp.recs:
                bad.append("recs")
            if (out.total_kmers, out.total_hits) != (exp.total_kmers, exp.total_hits):
                bad.append("totals")
            if want_ids and out.ids.tolist() != exp.ids:
                bad.append("ids")
            if want_occ and out.occ.tolist() != exp.occ:
                bad.append("occ")
        finally:
            s.free()
        entry = dict(case=case, k=k, keys=len(keys), distinct=exp.n_distinct, reads=len(reads), bases=sum(map(len, reads)), kmers=exp.total_kmers,
                     hits=exp.total_hits, dev=on_dev, ids=want_ids, occ=want_occ, knobs=knobs, differs=bad)
        log.append(entry)
        done += 1
        if bad:
            diffs.append(entry)
            print("DIFFERENCE", entry)
    for kn in KNOBS:
        os.environ.pop(kn, None)
    ctx.close()
    res = dict(script="stress_match.py", seed=a.seed, cases_run=done, cases_asked=a.cases, differences=len(diffs), seconds=round(time.time() - t0, 1),
               device=torch.cuda.get_device_name(0), cases=log)
    print(json.dumps({k: v for k, v in res.items() if k != "cases"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(1 if diffs else 0)


main()
