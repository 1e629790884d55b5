"""A second restatement of the Bloom writers (hash:bf:bin, hash:bfc:bin, hash:bft:bin) and the list layouts the Bloom merge kernels are
tested on (tests only).

`bloom_expected` is to the Bloom modes what `dict_merge` (test_merge_independent.py) is to COUNT / PA: written per HASH with Python
integers from include/kmx.h and the hand-worked vectors' comments -- a dictionary hash -> entries over all samples, no cursors, no
streams, no bit loops; a bfc row is ONE integer, written big-endian; a bft row is ONE integer per sample, written little-endian.  It
shares nothing with oracle/kmx_oracle.c (pack_insert_msb, orc_to_n_b, orc_transpose_bits), which it judges in test_bloom_ref_cpu.py."""
import numpy as np

MODE_BF, MODE_BFC, MODE_BFT = 2, 3, 4
EXTREME = [254, 255, 256, (1 << 15) - 1, 1 << 15, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]


def bloom_expected(lists, soft, rec_min, share_min, mode, lower, upper, bitw=2):
    """lists[i] = {hash: count}, every hash in [lower, upper].  -> (body bytes, rows, stats[6][N])"""
    N, W = len(lists), upper - lower + 1
    table = {}
    for i, l in enumerate(lists):
        for h, c in l.items():
            assert lower <= h <= upper and c > 0
            table.setdefault(h, []).append((i, c))
    stats = [[0] * N for _ in range(6)]          # NON_SOLID, RESCUED, UNIQUE_WO, UNIQUE_W, TOTAL_WO, TOTAL_W
    kept = {}                                    # hash -> [(sample, count)]: the non-zero cells of the rows that are kept
    for h, ent in table.items():
        solid = [(i, c) for i, c in ent if c >= soft[i]]
        weak = [(i, c) for i, c in ent if c < soft[i]]
        saved = weak if (share_min > 0 and len(solid) >= share_min) else []
        for i, c in solid:
            stats[2][i] += 1; stats[3][i] += 1; stats[4][i] += c; stats[5][i] += c
        for i, c in weak:
            stats[0][i] += 1
        for i, c in saved:
            stats[1][i] += 1; stats[3][i] += 1; stats[5][i] += c
        if len(solid) >= rec_min:                # (recurrence-min 0 keeps a hash nobody holds solid: its row is the zero vector)
            kept[h] = solid + saved
    if mode == MODE_BFT:
        n8, w8 = (N + 7) // 8 * 8, (W + 7) // 8 * 8
        col = [0] * n8                           # sample s: bit r = hash lower + r
        for h, cells in kept.items():
            for i, _ in cells:
                col[i] |= 1 << (h - lower)
        return b"".join(v.to_bytes(w8 // 8, "little") for v in col), n8, stats
    rb = (N + 7) // 8 if mode == MODE_BF else (N * bitw + 7) // 8
    body = bytearray(W * rb)
    for h, cells in kept.items():
        row = 0
        if mode == MODE_BF:                      # bit i & 7 of byte i >> 3: bit i of the row as a little-endian integer
            for i, _ in cells:
                row |= 1 << i
            body[(h - lower) * rb:(h - lower + 1) * rb] = row.to_bytes(rb, "little")
        else:                                    # field i: bits [i * w, (i + 1) * w) counted from the MSB of byte 0: a big-endian integer
            for i, c in cells:
                row |= min(c.bit_length(), (1 << bitw) - 1) << (8 * rb - (i + 1) * bitw)
            body[(h - lower) * rb:(h - lower + 1) * rb] = row.to_bytes(rb, "big")
    return bytes(body), W, stats


def layout(kind, seed, N, lower, W, per, step, extreme=False):
    """N lists {hash: count} in [lower, lower + W), counts 1 ... 6 (around per-list soft-mins of 1 ... 3):
      uniform    `per` records spread over the whole window
      clustered  each list's `per` records inside one band of per * 4 / 3 rows at a random place
      ends       even lists entirely in the first per * 9 / 8 rows, odd lists entirely in the last
      edges      about 90 % of {m - 1, m, m + 1 : m a multiple of `step`} plus the window's last row
    extreme: a tenth of the counts come from EXTREME"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N):
        if kind == "uniform":
            rows = rng.choice(W, size=min(per, W), replace=False)
        elif kind == "clustered":
            band = min(W, per * 4 // 3)
            rows = int(rng.integers(0, W - band + 1)) + rng.choice(band, size=min(per, band), replace=False)
        elif kind == "ends":
            band = min(W, per * 9 // 8)
            rows = (W - band if i & 1 else 0) + rng.choice(band, size=min(per, band), replace=False)
        elif kind == "edges":
            m = np.arange(0, W + step, step, dtype=np.int64)
            rows = np.unique(np.concatenate([m - 1, m, m + 1]))
            rows = rows[(rows >= 0) & (rows < W)]
            rows = np.union1d(rows[rng.random(len(rows)) < 0.9], [W - 1])
        else:
            raise ValueError(kind)
        cs = rng.integers(1, 7, len(rows)).astype(np.uint64)
        if extreme:
            m = rng.random(len(cs)) < 0.1
            cs[m] = np.array(EXTREME, np.uint64)[rng.integers(0, len(EXTREME), int(m.sum()))]
        out.append({lower + int(r): int(c) for r, c in zip(rows, cs)})
    return out


def cohort(seed, N, lower, W, dens, extreme=False):
    """N lists {hash: count}: about `dens` x W records each, four fifths of them out of a pool the lists share (rows most samples hold:
    recurrences and rescues), the others private"""
    rng = np.random.default_rng(seed)
    pool = rng.choice(W, size=max(1, min(W, int(W * dens))), replace=False)
    out = []
    for i in range(N):
        rows = np.union1d(pool[rng.random(len(pool)) < 0.8], rng.integers(0, W, max(1, int(W * dens / 5))))
        cs = rng.integers(1, 7, len(rows)).astype(np.uint64)
        if extreme:
            m = rng.random(len(cs)) < 0.1
            cs[m] = np.array(EXTREME, np.uint64)[rng.integers(0, len(EXTREME), int(m.sum()))]
        out.append({lower + int(r): int(c) for r, c in zip(rows, cs)})
    return out


def soft_mins(N):
    """1 + i % 3, and from two lists on one list (the middle one) at 2^32 - 1: its records are non-solid (but a count of 2^32 - 1), its
    rescued counts alone make its TOTAL_W"""
    soft = [1 + i % 3 for i in range(N)]
    if N >= 2:
        soft[N // 2] = 0xFFFFFFFF
    return soft


def arrays(lists):
    """{hash: count} dictionaries -> the ascending (keys uint64[n], counts uint32[n]) arrays the C ABIs take"""
    out = []
    for l in lists:
        ks = sorted(l)
        out.append((np.array(ks, np.uint64), np.array([l[h] for h in ks], np.uint32)))
    return out
