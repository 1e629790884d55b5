"""Seeded synthetic partitions (sorted per-sample count lists) for the parity tests."""
import numpy as np


def synth_lists(seed, n_lists, pool, p_present, n_private, kw=1, key_bits=62, count_max=50, ragged=False):
    """`pool` shared keys, each present in a sample with probability p_present, plus n_private
    keys private to each sample.  -> list of (keys uint64[n, kw], counts uint32[n]) ascending."""
    rng = np.random.default_rng(seed)
    total = pool + n_lists * n_private

    def draw(n):
        lo = rng.integers(0, 1 << min(key_bits, 62), n, dtype=np.uint64)
        if kw == 1:
            return lo.reshape(n, 1)
        if kw == 2:
            hi = rng.integers(0, 1 << max(1, min(key_bits - 64, 62)), n, dtype=np.uint64)
            return np.stack([lo, hi], axis=1)
        # three and four words (k = 64 ... 127): the upper words take one of eight values spread over all 64 bits (the top bit
        # included), so that many keys agree in some of their words and every word decides some comparisons
        ws = [lo if rng.random() < 0.9 else (lo & np.uint64(7))]
        for _ in range(kw - 1):
            ws.append(rng.integers(0, 8, n, dtype=np.uint64) * np.uint64(0x2492492492492492))
        top_bits = max(1, min(key_bits - 64 * (kw - 1), 62))
        ws[-1] = ws[-1] >> np.uint64(64 - top_bits) if top_bits < 62 else ws[-1]
        return np.stack(ws, axis=1)

    allk = np.unique(draw(int(total * 1.1) + 8), axis=0)
    rng.shuffle(allk, axis=0)
    return _assemble(rng, allk[:total], n_lists, pool, p_present, n_private, kw, count_max, ragged)


def _assemble(rng, allk, n_lists, pool, p_present, n_private, kw, count_max, ragged=False):
    """the lists out of distinct keys allk[n, kw]: the first `pool` shared, n_private private to each list"""
    shared, priv = allk[:pool], allk[pool:]
    out = []
    for i in range(n_lists):
        pp = p_present if not ragged else p_present * rng.random()
        mask = rng.random(pool) < pp
        ks = np.concatenate([shared[mask], priv[i * n_private:(i + 1) * n_private]], axis=0)
        if ragged and i % 7 == 3:
            ks = ks[:0]
        # ascending, most significant word first
        order = np.lexsort([ks[:, j] for j in range(kw)])
        ks = np.ascontiguousarray(ks[order])
        cs = rng.integers(1, count_max, len(ks), dtype=np.uint32)
        out.append((ks, cs))
    return out


# ---------------------------------------------------------------------------------------------------------------- full-width keys
U64 = (1 << 64) - 1
SHAPES = ("uniform", "straddle", "near-max", "low-word-only", "zero")
TOP_WORD = 0xC3A5C85C97CB3127          # the most significant word of every low-word-only key (bit 63 set)


def max_canonical(kw):
    """the largest canonical k-mer of k = 32 * kw (k = 128 for kw = 4: a bound the API accepts, no k reaches it): G^(16 kw) C^(16 kw),
    G = 3 and C = 1 (A0 C1 T2 G3), the first nucleotide in the top digit -- its reverse complement C^(16 kw) G^(16 kw) is smaller"""
    return kmer_value("G" * (16 * kw) + "C" * (16 * kw))


def key_words(v, kw):
    """a key as its words, low word first"""
    return [(v >> (64 * w)) & U64 for w in range(kw)]


def key_value(words):
    return sum(int(x) << (64 * w) for w, x in enumerate(words))


def _draw_wide(rng, n, kw, shape):
    """n keys (uint64[n, kw], low word first, not yet distinct) of one full-width shape"""
    def u64(m, hi=U64):
        return rng.integers(0, hi, m, dtype=np.uint64, endpoint=True)

    if shape == "uniform":                 # every word uniform over its 64 bits, the most significant one included
        return np.stack([u64(n) for _ in range(kw)], axis=1)
    if shape == "straddle":                # the most significant word within delta of 2^63, where a signed compare reverses the order
        delta = max(4 * n, 64) if kw == 1 else 3
        top = (np.uint64(1 << 63) - np.uint64(delta)) + u64(n, 2 * delta)
        return np.stack([u64(n) for _ in range(kw - 1)] + [top], axis=1)
    if shape == "near-max":                # at and just below the largest canonical value of k = 32 * kw
        ws = [np.full(n, x, np.uint64) for x in key_words(max_canonical(kw), kw)]      # (no word of it is below 4 n + 8: no borrow)
        ws[0] -= rng.integers(0, 4 * n + 8, n).astype(np.uint64)
        if kw > 1:
            ws[1] -= rng.integers(0, 3, n).astype(np.uint64)
        return np.stack(ws, axis=1)
    if shape == "low-word-only":           # every upper word alike (the middle ones of four values); low words in pairs that differ
        base = u64(n // 2 + 1, (1 << 63) - 1)      # in bit 63 alone
        ws = [np.concatenate([base, base | np.uint64(1 << 63)])[:n]]
        mids = np.array([0x0123456789ABCDEF, 0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0xFEDCBA9876543210], np.uint64)
        ws += [mids[rng.integers(0, 4, n)] for _ in range(kw - 2)]
        ws += [np.full(n, TOP_WORD, np.uint64)] if kw > 1 else []
        return np.stack(ws, axis=1)
    if shape == "zero":                    # the smallest keys: 0, 1 and a few above, every upper word 0
        return np.stack([u64(n, 8 * n + 16)] + [np.zeros(n, np.uint64)] * (kw - 1), axis=1)
    raise ValueError(shape)


def _special_keys(kw, shape):
    """keys a shape always holds (in the shared pool): the largest canonical value itself, key 0 and key 1"""
    if shape == "near-max":
        mx = max_canonical(kw)
        return [key_words(mx, kw), key_words(mx - 1, kw)]
    if shape == "zero":
        return [key_words(0, kw), key_words(1, kw)]
    if shape == "low-word-only":
        return [key_words((TOP_WORD << (64 * (kw - 1))) if kw > 1 else 0, kw)]
    return []


def synth_wide_lists(seed, n_lists, pool, p_present, n_private, kw=1, shape="uniform", count_max=50, ragged=False):
    """synth_lists over the whole key width: the keys of one of SHAPES (`uniform`, `straddle`, `near-max`, `low-word-only`, `zero`),
    lists strictly ascending, most significant word first.  The special keys of the shape (the largest canonical value, keys 0 and 1)
    lead the shared pool."""
    rng = np.random.default_rng(seed)
    total = pool + n_lists * n_private
    special = np.array(_special_keys(kw, shape), np.uint64).reshape(-1, kw)
    drawn = np.unique(_draw_wide(rng, int(total * 1.2) + 8, kw, shape), axis=0)
    drawn = drawn[~(drawn[:, None, :] == special[None, :, :]).all(axis=2).any(axis=1)] if len(special) else drawn
    rng.shuffle(drawn, axis=0)
    allk = np.concatenate([special, drawn], axis=0)[:total]
    return _assemble(rng, allk, n_lists, pool, p_present, n_private, kw, count_max, ragged)


def synth_hash_lists(seed, n_lists, lower, window, density, count_max=20):
    """hash-mode lists: each sample holds ~density*window distinct hashes of [lower, lower+window)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_lists):
        n = int(window * density * (0.5 + rng.random()))
        hs = np.unique(rng.integers(lower, lower + window, n, dtype=np.uint64))
        cs = rng.integers(1, count_max, len(hs), dtype=np.uint32)
        out.append((hs.reshape(-1, 1), cs))
    return out


_NT = {"A": 0, "C": 1, "T": 2, "G": 3}


def kmer_value(s):
    """a k-mer's value as the reference encodes it: A0 C1 T2 G3, the first nucleotide in the top digit (kmer.hpp:938)"""
    v = 0
    for c in s:
        v = v * 4 + _NT[c]
    return v


def canonical_value(s):
    rc = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return min(kmer_value(s), kmer_value(rc))


def superk_record(seq, k):
    """the super-k-mer record of the len(seq) - k + 1 consecutive k-mers of `seq` (gatb Model.hpp:1388-1433 as sorting_count.hpp:153-275
    reads it): [u8 n][ceil((k + n - 1) / 4) bytes of S, little endian], S = the first k-mer's value + the following nucleotides at
    digits k, k + 1, ..."""
    n = len(seq) - k + 1
    assert 1 <= n <= 255
    S = kmer_value(seq[:k])
    for j, c in enumerate(seq[k:]):
        S |= _NT[c] << (2 * (k + j))
    return bytes([n]) + S.to_bytes((k + n - 1 + 3) // 4, "little")


def synth_superk_stream(seed, k, n_records, max_kmers, genome=4000):
    """records cut at random places of a random genome (so that k-mers repeat), 1 .. max_kmers k-mers each -> (bytes, {canonical value: count})"""
    rng = np.random.default_rng(seed)
    g = "".join("ACGT"[i] for i in rng.integers(0, 4, genome + k + max_kmers))
    out, counts = [], {}
    for _ in range(n_records):
        n = int(rng.integers(1, max_kmers + 1)); at = int(rng.integers(0, genome))
        seq = g[at:at + k + n - 1]
        if rng.random() < 0.5:
            seq = seq[::-1].translate(str.maketrans("ACGT", "TGCA"))
        out.append(superk_record(seq, k))
        for j in range(n):
            v = canonical_value(seq[j:j + k])
            counts[v] = counts.get(v, 0) + 1
    return b"".join(out), counts


# ---------------------------------------------------------------------------------------------------------------- hash windows
# A window hash is XXH64(canonical k-mer words) % window + window * partition, mod 2^64 (kmx.h; hash.hpp's HashWindow): both the
# window and the partition id are u64, so keys reach every value of 64 bits, the all-ones key included.
WINDOW_SHAPES = ("small", "2^32-1", "2^32", "2^32+64", "2^40", "below-2^63", "above-2^63", "below-2^64", "above-2^64", "sparse-ids",
                 "all-ones-top", "all-ones-one")
SPARSE_IDS = (0, 65535, 1 << 32, U64)


def value_xxh64(v, k):
    """XXH64 (seed 0) over the 8 * ceil(k / 32) little-endian bytes of a canonical k-mer value's words"""
    import orc      # (the oracle's XXH64, pinned to the specification's vectors; imported here: plain draws need no oracle)
    return orc.xxh64(b"".join(w.to_bytes(8, "little") for w in key_words(v, (k + 31) // 32)))


def hash_key(s, window, partition):
    """the window hash of k-mer string `s`, restated with Python integers"""
    return (value_xxh64(canonical_value(s), len(s)) % window + window * partition) & U64


def hash_counts(counts, k, window, partition, hard_min=1, xxh=None):
    """{canonical value: count} (synth_superk_stream) -> sorted [(window hash, count)] with count >= hard_min; k-mers whose hashes
    meet are one key.  xxh: {value: value_xxh64(value, k)} computed once by the caller"""
    out = {}
    for v, c in counts.items():
        h = ((xxh[v] if xxh is not None else value_xxh64(v, k)) % window + window * partition) & U64
        out[h] = out.get(h, 0) + c
    return sorted((h, c) for h, c in out.items() if c >= hard_min)


def hash_window(shape, P, x=None, at=0):
    """-> (window, partition ids[P]) of one of WINDOW_SHAPES.  `all-ones-*` build the all-ones key for a k-mer whose XXH64 is x, kept
    in partition `at`: window x + 1 at partition id 2^64 - 1 (x < 2^64 - 1), or window 2^64 - 1 - x at partition id 1 (x < 2^63)"""
    assert P >= 2
    ids = list(range(P))
    if shape == "small":
        return 100003, [(3 * p + 7) % 11 for p in range(P)]
    if shape in ("2^32-1", "2^32", "2^32+64", "2^40"):
        return {"2^32-1": (1 << 32) - 1, "2^32": 1 << 32, "2^32+64": (1 << 32) + 64, "2^40": 1 << 40}[shape], ids
    if shape == "below-2^63":              # window * P just below 2^63 / 2^64, and just above (the keys of the last partitions wrap)
        return ((1 << 63) - 1) // P, ids
    if shape == "above-2^63":
        return (1 << 63) // P + 1, ids
    if shape == "below-2^64":
        return U64 // P, ids
    if shape == "above-2^64":
        return (1 << 64) // P + 1, ids
    if shape == "sparse-ids":
        return (1 << 20) + 7, [SPARSE_IDS[p % 4] for p in range(P)]
    if shape == "all-ones-top":
        assert x is not None and x < U64
        return x + 1, [U64 if p == at else p for p in range(P)]
    if shape == "all-ones-one":           # (partition `at` takes id 1, partition 1 id `at`)
        assert x is not None and x < 1 << 63
        return U64 - x, [1 if p == at else at if p == 1 else p for p in range(P)]
    raise ValueError(shape)
