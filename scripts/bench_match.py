"""kmx_match_dev on device-resident 150-base reads against sets of 10^5, 10^6 (the size of a `kmx diff` output: they fit the L2 / Infinity
Cache) and 10^8 k-mers (a whole run: they do not), at k = 31 and k = 63, at a hit rate of about 100 % (the reads are windows of the
sequence whose k-mers are the set, half of them reverse-complemented) and of about 0 % (random reads).  Per case: the time of the call's
kernels and of its two parts (probe; cover -- median of the timed calls after warm-up, HIP events through kmx_set_profiling), the
algorithmic bytes, and -- timed with HIP events in the same process -- two yardsticks: a gather (torch's index_select over a table of
as many u64 as the set's table has slots) that performs the same number of random 8-byte loads, one a valid k-mer, and nothing else; and a
sum over the bases, which merely reads them.  The set is handed over with its duplicates (a sequence's k-mers as they come).  No threshold
is set; the script records what the device gives.  Needs the GPU.
Usage: bench_match.py [--reads 400000] [--sizes 100000,1000000,100000000] [--steps 10] [--warmup 2] [--out profiles/match_bench.json]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from kmtricks_amd import lib

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=400_000)
ap.add_argument("--sizes", default="100000,1000000,100000000")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_match.py needs the GPU")
torch.cuda.init()
med = statistics.median
DEV, L = "cuda:0", 150
MIN = -(1 << 63)


def canonical_kmers(d, k):
    """the canonical k-mer at every position of the digit string d (A0 C1 T2 G3, a device tensor) -> int64[m, key_words], low word first"""
    kw, m = (k + 31) // 32, d.numel() - k + 1
    f, r = torch.zeros((m, kw), dtype=torch.int64, device=DEV), torch.zeros((m, kw), dtype=torch.int64, device=DEV)
    for j in range(k):      # base j of the k-mer at i is d[i + j]: digit k - 1 - j forward, digit j (complemented) of the reverse complement
        x = d[j:j + m].to(torch.int64)
        fi, ri = k - 1 - j, j
        f[:, fi >> 5] |= x << (2 * (fi & 31))
        r[:, ri >> 5] |= (x ^ 2) << (2 * (ri & 31))
    less = torch.zeros(m, dtype=torch.bool, device=DEV); decided = torch.zeros(m, dtype=torch.bool, device=DEV)
    for w in range(kw - 1, -1, -1):      # (unsigned order: the sign bit flipped)
        ne = (f[:, w] != r[:, w]) & ~decided
        less |= ne & ((r[:, w] ^ MIN) < (f[:, w] ^ MIN))
        decided |= ne
    return torch.where(less[:, None], r, f).contiguous()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return med(out)


def main():
    ctx = lib.Context(0)
    ctx.set_profiling(True)
    g = torch.Generator(device=DEV); g.manual_seed(11)
    acgt = torch.tensor([ord(c) for c in "ACTG"], dtype=torch.uint8, device=DEV)      # digit -> letter
    offs = (torch.arange(a.reads + 1, dtype=torch.int64, device=DEV) * L).contiguous()
    n_bases = a.reads * L
    rows = []
    for n_set in [int(x) for x in a.sizes.split(",")]:
        for k in (31, 63):
            src = torch.randint(0, 4, (n_set + k - 1,), dtype=torch.uint8, device=DEV, generator=g)
            keys = canonical_kmers(src, k)      # n_set keys, duplicates as they come
            torch.cuda.synchronize()
            s = ctx.kset_dev(keys.data_ptr(), n_set, k)
            s.wait()
            build_ms, n_distinct = s.kernel_ms, s.n_distinct
            del keys
            slots = 2
            while slots < 2 * n_set:
                slots <<= 1
            table = torch.zeros(slots, dtype=torch.int64, device=DEV)
            for hit in (1, 0):
                if hit:      # windows of the source, every other one reverse-complemented
                    at = torch.randint(0, n_set + k - 1 - L, (a.reads,), device=DEV, generator=g)
                    d = src[(at[:, None] + torch.arange(L, device=DEV)[None, :])]
                    d[1::2] = d[1::2].flip(1) ^ 2
                else:
                    d = torch.randint(0, 4, (a.reads, L), dtype=torch.uint8, device=DEV, generator=g)
                bases = acgt[d.reshape(-1).to(torch.int64)].contiguous()
                torch.cuda.synchronize()
                ms, probe, cover, out = [], [], [], None
                for step in range(a.warmup + a.steps):
                    r = ctx.match_dev(s, bases.data_ptr(), offs.data_ptr(), a.reads, keep=True)
                    r.wait()
                    if step >= a.warmup:
                        p, c = r.kernel_parts_ms()
                        ms.append(r.kernel_ms()); probe.append(p); cover.append(c)
                    if step == a.warmup + a.steps - 1:
                        out = dict(kmers=r._call("total_kmers"), hits=r._call("total_hits"), algo_bytes=r.algo_bytes())
                    r.free()
                idx = torch.randint(0, slots, (out["kmers"],), dtype=torch.int64, device=DEV, generator=g)
                gather = timed(lambda: table.index_select(0, idx), a.steps, a.warmup)
                read = timed(lambda: bases.view(torch.int64).sum(), a.steps, a.warmup)
                del idx
                row = dict(n_set=n_set, n_distinct=n_distinct, k=k, table_mb=round(8 * slots / 2 ** 20, 1), build_ms=round(build_ms, 3), hit_rate=round(out["hits"] / max(out["kmers"], 1), 4),
                           reads=a.reads, bases=n_bases, kernel_ms=round(med(ms), 4), probe_ms=round(med(probe), 4), cover_ms=round(med(cover), 4),
                           gather_ms=round(gather, 4), read_bases_ms=round(read, 4), probe_over_gather=round(med(probe) / gather, 2),
                           ns_per_lookup=round(1e6 * med(probe) / max(out["kmers"], 1), 4), glookups_s=round(out["kmers"] / med(probe) / 1e6, 2),
                           algo_gb_s=round(out["algo_bytes"] / med(ms) / 1e6, 1), **out)
                rows.append(row)
                print(json.dumps(row), flush=True)
            s.free()
            del table, src
    ctx.close()
    res = dict(script="bench_match.py", device=torch.cuda.get_device_name(0), read_length=L, steps=a.steps, warmup=a.warmup, cases=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


main()
