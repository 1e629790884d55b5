"""kmx_unitigs_dev on the distinct canonical k-mers of a random 5-Mbp sequence into which repeats are planted (1 % of its length: copies
and reverse-complemented copies of 500-base pieces), at k = 31 (one key word) and k = 63 (two), shuffled and device resident.  Per case:
the time of the call's kernels and of its four parts (table; links; rank; finish -- median of the timed calls after warm-up, HIP events
through kmx_set_profiling), the algorithmic bytes, the unitigs found, and -- timed with HIP events in the same process -- the yardstick
for the link pass: a gather (torch's index_select over the key array, a key an element of 8 or 16 bytes) that performs the same number
of random 8 * key_words-byte loads, 8 a k-mer, and nothing else.  No threshold is set; the script records what the device gives.  Needs the GPU.
Usage: bench_unitigs.py [--bases 5000000] [--steps 10] [--warmup 2] [--out profiles/unitigs_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib
import unitig_ref as ur

ap = argparse.ArgumentParser()
ap.add_argument("--bases", type=int, default=5_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_unitigs.py needs the GPU")
torch.cuda.init()
med = statistics.median


def sequence(rng, n):
    """digits (A0 C1 T2 G3) of a random sequence, 1 % of it planted repeats"""
    d = rng.integers(0, 4, n, dtype=np.uint8)
    for _ in range(n // 100 // 500):
        src, dst = rng.integers(0, n - 500, 2)
        piece = d[src:src + 500].copy()
        d[dst:dst + 500] = piece if rng.random() < 0.5 else (piece[::-1] ^ 2)
    return d


def canonical_kmers(d, k):
    """the distinct canonical k-mers of the digit string d -> uint64[n, key_words], low word first, shuffled"""
    kw, m = ur.key_words_of(k), len(d) - k + 1
    f, r = np.zeros((m, kw), np.uint64), np.zeros((m, kw), np.uint64)
    for j in range(k):      # base j of the k-mer at i is d[i + j]: digit k - 1 - j forward, digit j (complemented) of the reverse complement
        x = d[j:j + m].astype(np.uint64)
        fi, ri = k - 1 - j, j
        f[:, fi >> 5] |= x << np.uint64(2 * (fi & 31))
        r[:, ri >> 5] |= (x ^ np.uint64(2)) << np.uint64(2 * (ri & 31))
    less = np.zeros(m, bool); decided = np.zeros(m, bool)
    for w in range(kw - 1, -1, -1):
        ne = (f[:, w] != r[:, w]) & ~decided
        less |= ne & (r[:, w] < f[:, w])
        decided |= ne
    c = np.where(less[:, None], r, f)
    c = np.unique(c, axis=0)
    return c


def main():
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    rng = np.random.default_rng(5)
    d = sequence(rng, a.bases)
    out = []
    for k in (31, 63):
        kw = ur.key_words_of(k)
        keys = canonical_kmers(d, k)
        keys = keys[rng.permutation(len(keys))]
        n = len(keys)
        small = [int(sum(int(w) << (64 * i) for i, w in enumerate(row))) for row in keys[:3000]]      # a subsample against road A first
        got, exp = ctx.unitigs(ur.keys_to_words(small, k), k), ur.unitigs_links(small, k)
        assert got.n_unitigs == exp.U and got.unitig.tolist() == exp.unitig and [s.decode() for s in got.seqs] == exp.seqs, f"k = {k}: the first 3000 keys"
        dk = torch.from_numpy(keys.view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        total, parts, algo, U = [], [], 0, 0
        for step in range(a.warmup + a.steps):
            r = ctx.unitigs_dev(dk.data_ptr(), n, k, keep=True)
            r.wait()
            if step >= a.warmup:
                total.append(r.kernel_ms()); parts.append(r.kernel_parts_ms()); algo = r.algo_bytes(); U = r.n_unitigs()
            r.free()
        # the yardstick: 8 n random loads of 8 * kw bytes
        idx = torch.randint(0, n, (8 * n,), device="cuda:0")
        flat = dk.view(-1) if kw == 1 else dk.view(torch.complex128).view(-1)      # one element a key: 8 or 16 bytes a load
        gather = []
        for step in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); g = flat.index_select(0, idx); e1.record(); torch.cuda.synchronize()
            if step >= a.warmup:
                gather.append(e0.elapsed_time(e1))
            del g
        p = [med(x[i] for x in parts) for i in range(4)]
        rec = dict(kernel="unitigs", k=k, key_words=kw, bases=a.bases, kmers=n, unitigs=int(U), steps=a.steps, warmup=a.warmup,
                   unitigs_ms=round(med(total), 4), unitigs_ms_min=round(min(total), 4), unitigs_ms_max=round(max(total), 4), algo_bytes=algo,
                   algo_gb_s=round(algo / (med(total) * 1e-3) / 1e9, 1), table_ms=round(p[0], 4), links_ms=round(p[1], 4), rank_ms=round(p[2], 4), finish_ms=round(p[3], 4),
                   gather_loads=8 * n, gather_bytes_each=8 * kw, gather_ms=round(med(gather), 4), links_over_gather=round(p[1] / med(gather), 3))
        out.append(rec); print(json.dumps(rec), flush=True)
        del flat, dk, idx
        torch.cuda.empty_cache()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), cases=out), f, indent=1)


main()
