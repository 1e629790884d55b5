"""What `kmx combine` (kmx_combine_dev / kmx_combine_host) computes, restated from its definition with a dictionary keyed by the
key's integer value (numpy only for the byte layout).

Input: B blocks in column order.  Block i: rows with strictly ascending keys (kw u64 words, low word first; keys compare most
significant word first) and n_cols_i columns.
  MODE_COUNT  a row's payload is n_cols_i counts of count_bytes_i (1, 2 or 4) bytes, little endian
  MODE_PA     a row's payload is ceil(n_cols_i / 8) bytes, column j = bit j & 7 of byte j >> 3; the padding bits of the last byte
              are ignored
Output: one row per distinct key of the union of the blocks, ascending.  N = sum of n_cols_i, pos_i = sum of n_cols_j over j < i.
  MODE_COUNT  key + N u32: column pos_i + c = block i's count c widened to 32 bits, 0 where block i lacks the key
  MODE_PA     key + ceil(N / 8) bytes: bit pos_i + c = block i's bit c, 0 where block i lacks the key; padding bits of the last byte 0
drop_last (KMX_COMBINE_DROP_LAST, the driver's --reference-compat): the greatest key of the union is not written when exactly one
block holds it; it is written when two or more do.
Worked example (COUNT, one-word keys): block 0, 2 columns, rows 3:(1,2) 9:(5,6); block 1, 1 column of 1-byte counts, rows 3:(7)
4:(8) -> 3:(1,2,7) 4:(0,0,8) 9:(5,6,0); with drop_last the row of key 9 is missing."""
import numpy as np

MODE_COUNT, MODE_PA = 0, 1
COUNT_DTYPE = {1: np.dtype("<u1"), 2: np.dtype("<u2"), 4: np.dtype("<u4")}


def _value(words):
    """a key's words (low word first) as one integer: comparing the integers compares the most significant word first"""
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


def payload_bytes(n_cols, mode, count_bytes=4):
    return n_cols * count_bytes if mode == MODE_COUNT else (n_cols + 7) // 8


def block_body(keys, payload):
    """the bytes of a block: per row the key words, then the payload"""
    keys = np.asarray(keys, np.uint64)
    if not len(keys):
        return b""
    payload = np.asarray(payload, np.uint8).reshape(len(keys), -1)
    return np.concatenate([keys.reshape(len(keys), -1).view(np.uint8).reshape(len(keys), -1), payload], axis=1).tobytes()


def combine_expected(blocks, kw, mode, drop_last=False):
    """blocks: [(keys uint64[n, kw], payload uint8[n, payload bytes], n_cols[, count_bytes])] -> (body bytes, rows)"""
    union = {}      # key value -> {block: its payload row}
    pos, total = [], 0
    for i, b in enumerate(blocks):
        keys = np.asarray(b[0], np.uint64).reshape(-1, kw)
        n_cols, cb = b[2], (b[3] if len(b) > 3 else 4)
        payload = np.asarray(b[1], np.uint8).reshape(len(keys), payload_bytes(n_cols, mode, cb)) if len(keys) else np.zeros((0, 0), np.uint8)
        pos.append(total)
        total += n_cols
        for k, pl in zip(keys, payload):
            union.setdefault(_value(k), {})[i] = pl
    order = sorted(union)
    if drop_last and order and len(union[order[-1]]) == 1:
        order.pop()
    out = []
    for v in order:
        held = union[v]
        key = b"".join(((v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little") for w in range(kw))
        if mode == MODE_COUNT:
            row = np.zeros(total, np.dtype("<u4"))
            for i, pl in held.items():
                n_cols, cb = blocks[i][2], (blocks[i][3] if len(blocks[i]) > 3 else 4)
                row[pos[i]:pos[i] + n_cols] = np.frombuffer(pl.tobytes(), COUNT_DTYPE[cb]).astype(np.uint32)
            out.append(key + row.tobytes())
        else:
            bits = 0
            for i, pl in held.items():
                n_cols = blocks[i][2]
                bits |= (int.from_bytes(pl.tobytes(), "little") & ((1 << n_cols) - 1)) << pos[i]
            out.append(key + bits.to_bytes((total + 7) // 8, "little"))
    return b"".join(out), len(order)


def combine_expected_np(blocks, kw, mode, drop_last=False):
    """the same body by another road, for blocks too long for the dictionary: numpy over whole columns -- the union is np.unique over
    the keys' words, most significant first; a block's payload goes to its rows of the union at once.  tests/test_combine_cpu.py holds
    the two against each other.  -> (body bytes, rows)"""
    keys = [np.asarray(b[0], np.uint64).reshape(-1, kw) for b in blocks]
    total = sum(b[2] for b in blocks)
    if not sum(len(k) for k in keys):
        return b"", 0
    union, inv = np.unique(np.concatenate(keys)[:, ::-1], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    rows = len(union)
    if drop_last and rows and int((inv == rows - 1).sum()) == 1:
        rows -= 1
    wide = np.zeros((len(union), total), np.uint32 if mode == MODE_COUNT else np.uint8)      # a count, or a bit, per column
    at, pos = 0, 0
    for b, k in zip(blocks, keys):
        n_cols, cb = b[2], (b[3] if len(b) > 3 else 4)
        if len(k):
            pl = np.ascontiguousarray(np.asarray(b[1], np.uint8).reshape(len(k), payload_bytes(n_cols, mode, cb)))
            vals = pl.view(COUNT_DTYPE[cb]).astype(np.uint32) if mode == MODE_COUNT else np.unpackbits(pl, axis=1, bitorder="little")[:, :n_cols]
            wide[inv[at:at + len(k)], pos:pos + n_cols] = vals
        at += len(k)
        pos += n_cols
    pay = wide.astype("<u4").view(np.uint8).reshape(len(union), 4 * total) if mode == MODE_COUNT else \
        np.packbits(wide, axis=1, bitorder="little").reshape(len(union), (total + 7) // 8)
    low_first = np.ascontiguousarray(union[:, ::-1]).astype("<u8").view(np.uint8).reshape(len(union), 8 * kw)
    return np.concatenate([low_first, pay], axis=1)[:rows].tobytes(), rows


def sort_keys(keys):
    """distinct keys uint64[n, kw] in ascending order, most significant word first"""
    keys = np.unique(np.asarray(keys, np.uint64).reshape(len(keys), -1), axis=0)
    return np.ascontiguousarray(keys[np.lexsort([keys[:, j] for j in range(keys.shape[1])])])


def synth_case(seed, rows, n_cols, kw, mode, share=0.5, shape="uniform", count_bytes=None, extreme=False):
    """seeded blocks: block i has about rows[i] rows and n_cols[i] columns (count_bytes[i] bytes a count; 4 when left out).  A share
    `share` (0 ... 1) of a block's keys comes from the front of one list common to all blocks -- so a shorter block's shared keys
    are shared with every longer block -- the rest are its own.  Keys: one of synth.py's full-width SHAPES.  extreme: a fifth of
    the counts at the maximum of their width (0xFF, 0xFFFF, 2^32 - 1).  Presence/absence payloads are random bytes, padding bits
    included.  -> [(keys, payload, n_cols, count_bytes)]"""
    from synth import synth_wide_lists
    rng = np.random.default_rng(seed)
    B = len(rows)
    count_bytes = list(count_bytes) if count_bytes is not None else [4] * B
    n_shared = [min(int(round(r * share)), r) for r in rows]
    n_own = [r - s for r, s in zip(rows, n_shared)]
    want = max(n_shared + [0]) + sum(n_own)
    pool = sort_keys(np.concatenate([l[0] for l in synth_wide_lists(seed, 1, want + 8, 1.0, 0, kw=kw, shape=shape)])) if want else np.zeros((0, kw), np.uint64)
    pool = pool[rng.permutation(len(pool))]
    common, at, out = pool[:max(n_shared + [0])], max(n_shared + [0]), []
    for i in range(B):
        own = pool[at:at + n_own[i]]
        at += n_own[i]
        keys = sort_keys(np.concatenate([common[:n_shared[i]], own])) if n_shared[i] + len(own) else np.zeros((0, kw), np.uint64)
        n = len(keys)
        if mode == MODE_COUNT:
            cb = count_bytes[i]
            top = (1 << (8 * cb)) - 1
            cols = rng.integers(0, min(300, top + 1), (n, n_cols[i]), dtype=np.uint32)
            if extreme:
                cols[rng.random(cols.shape) < 0.2] = top
            payload = cols.astype(COUNT_DTYPE[cb]).view(np.uint8).reshape(n, n_cols[i] * cb)
        else:
            payload = rng.integers(0, 256, (n, (n_cols[i] + 7) // 8), dtype=np.uint8)
        out.append((keys, np.ascontiguousarray(payload), n_cols[i], count_bytes[i]))
    return out


def _payload(rng, n, n_cols, mode):
    if mode == MODE_COUNT:
        cols = rng.integers(0, 300, (n, n_cols), dtype=np.uint32)
        cols[rng.random(cols.shape) < 0.2] = 0xFFFFFFFF
        return np.ascontiguousarray(cols.view(np.uint8).reshape(n, 4 * n_cols))
    return rng.integers(0, 256, (n, (n_cols + 7) // 8), dtype=np.uint8)


def span_case(seed, kw, mode, n_b, n_a=200, cols=(3, 5)):
    """two blocks for the edge of k_combine_rank's staged span: block A has n_a rows (one rank tile), its smallest key below and its
    largest above every key of block B, so that the span of A's tile in B is all n_b rows of B; half of A's other keys are keys of B
    too (share 0.5).  -> [A, B] as synth_case gives blocks"""
    rng = np.random.default_rng(seed)
    own = n_a - (n_a - 2) // 2      # A's keys that B lacks, its two ends among them
    pool = sort_keys(rng.integers(0, 2 ** 64, (n_b + own + 64, kw), dtype=np.uint64, endpoint=False))[:n_b + own]
    assert len(pool) == n_b + own
    inner = rng.permutation(np.arange(1, len(pool) - 1))
    a_own = np.concatenate([[0, len(pool) - 1], inner[:own - 2]])
    b_idx = np.sort(inner[own - 2:])
    a_idx = np.sort(np.concatenate([a_own, rng.choice(b_idx, n_a - own, replace=False)]))
    assert len(a_idx) == n_a and len(b_idx) == n_b and a_idx[0] < b_idx[0] and a_idx[-1] > b_idx[-1]
    return [(pool[a_idx], _payload(rng, n_a, cols[0], mode), cols[0], 4), (pool[b_idx], _payload(rng, n_b, cols[1], mode), cols[1], 4)]
