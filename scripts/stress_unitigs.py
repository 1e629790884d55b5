"""Seeded random k-mer sets through kmx_unitigs_* against road A of tests/unitig_ref.py: k in 8 ... 127, dense random keys at small k,
the k-mers of random sequences with planted repeats and inverted repeats, circles, mixtures of all three; shuffled or sorted; host or
device-resident keys; the hash cut to a few bits (KMX_UNITIG_HASH_BITS, on sets of at most 400 keys) and the launch knobs.  Every output
is compared bit for bit.  Needs the GPU (no fallback).
Usage: stress_unitigs.py [--cases 40] [--seed 1] [--seconds 240] [--out profiles/unitigs_stress.json]"""
import argparse, json, os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import unitig_ref as ur

ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=40)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--seconds", type=float, default=240.0, help="no new case is started after this many seconds")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stress_unitigs.py needs the GPU")
torch.cuda.init()
KNOBS = ("KMX_UNITIG_HASH_BITS", "KMX_UNITIG_CUS", "KMX_UNITIG_GRID")


def make_keys(rng, k, kind):
    keys = set()
    if kind in ("dense", "mix") and k <= 12:
        keys |= {ur.canon_int(rng.getrandbits(2 * k), k) for _ in range(rng.randrange(1, 3000))}
    if kind in ("seq", "mix"):
        for _ in range(rng.randrange(1, 4)):
            s = ur.rand_seq(rng, rng.randrange(k, 600))
            rep = ur.rand_seq(rng, k + rng.randrange(0, 9))
            at = rng.randrange(len(s))
            s = s[:at] + rep + s[at:] + rng.choice([rep, ur.rc_str(rep), ""]) + ur.rand_seq(rng, rng.randrange(0, 50))
            keys |= set(ur.kmers_of(s, k))
    if kind in ("circle", "mix"):
        for _ in range(rng.randrange(1, 4)):
            keys |= set(ur.kmers_of(ur.rand_seq(rng, rng.randrange(2, 300)), k, circular=True))
    return ur.ordered(sorted(keys), rng, rng.random() < 0.7)


def main():
    ctx = lib.Context(0)
    rng = random.Random(a.seed)
    t0, done, failed = time.time(), [], []
    for case in range(a.cases):
        if time.time() - t0 > a.seconds:
            break
        k = rng.choice([rng.randrange(8, 13), rng.randrange(8, 128), rng.choice([31, 32, 33, 63, 64, 65, 96, 97, 127])])
        kind = rng.choice(["dense", "seq", "circle", "mix"]) if k <= 12 else rng.choice(["seq", "circle", "mix"])
        keys = make_keys(rng, k, kind)
        exp = ur.unitigs_links(keys, k)
        words = ur.keys_to_words(keys, k)
        env = {}
        if len(keys) <= 400 and rng.random() < 0.5:
            env["KMX_UNITIG_HASH_BITS"] = str(rng.choice([0, 1, 3, 8]))
        if rng.random() < 0.3:
            env[rng.choice(KNOBS[1:])] = str(rng.choice([1, 2, 3]))
        for kn in KNOBS:
            os.environ.pop(kn, None)
        os.environ.update(env)
        resident = rng.random() < 0.5
        if resident and len(keys):
            d = torch.from_numpy(words.view(np.int64).copy()).to("cuda:0")
            torch.cuda.synchronize()
            out = ctx.unitigs_dev(d.data_ptr(), len(keys), k)
        else:
            out = ctx.unitigs(words, k)
        for kn in KNOBS:
            os.environ.pop(kn, None)
        ok = (out.n_unitigs == exp.U and out.unitig.tolist() == exp.unitig and out.pos.tolist() == exp.pos and out.ori.tolist() == exp.ori and
              out.start.tolist() == exp.start and out.len.tolist() == exp.len and out.circ.tolist() == exp.circ and out.seq_off.tolist() == exp.seq_off(k) and
              [s.decode() for s in out.seqs] == exp.seqs)
        rec = dict(case=case, k=k, kind=kind, n=len(keys), unitigs=exp.U, cycles=sum(exp.circ), resident=resident, env=env, ok=ok)
        (done if ok else failed).append(rec)
        print(json.dumps(rec), flush=True)
    ctx.close()
    summary = dict(seed=a.seed, cases=len(done) + len(failed), differences=len(failed), seconds=round(time.time() - t0, 1), failed=failed,
                   device=torch.cuda.get_device_name(0), k_values=sorted({r["k"] for r in done}), cycles=sum(r["cycles"] for r in done))
    print(json.dumps(summary))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(1 if failed else 0)


main()
