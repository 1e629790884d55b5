"""What `kmx filter` computes, restated from its definition with a dictionary and a set (numpy only for the byte layout).

rows = a matrix's rows in file order, key = the new sample's (k-mer, count) list of the same partition:
  m  the rows whose k-mer is in `key`, in file order; a count row gets one more u32 column at its end, the k-mer's count in `key`;
     a presence/absence row is unchanged
  v  per input row, in file order: the count in `key` (count rows) or 1 (presence/absence rows) when its k-mer is in `key`, else 0
  k  the records of `key` whose k-mer is in no row, ascending (keys compare most significant word first)
Worked example: rows 3 5 9 12, key (1,4) (5,2) (9,7) (20,3) -> m = rows 5 and 9 with new column 2 and 7; v = 0 2 7 0; k = (1,4) (20,3)."""
import numpy as np

MODE_COUNT, MODE_PA = 0, 1


def _value(words):
    """a key's words (low word first) as one integer: comparing the integers compares the most significant word first"""
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


def filter_expected(row_keys, payload, key_keys, key_counts, mode):
    """row_keys uint64[n, kw] (low word first), payload uint8[n, bytes of a row behind its key], key_keys uint64[m, kw],
    key_counts uint32[m] -> (m body bytes, v uint32[n], k keys uint64[a, kw], k counts uint32[a])"""
    row_keys = np.asarray(row_keys, np.uint64)
    kw = row_keys.shape[1] if row_keys.ndim == 2 else np.asarray(key_keys).reshape(len(key_counts), -1).shape[1]
    row_keys = row_keys.reshape(-1, kw)
    key_keys = np.asarray(key_keys, np.uint64).reshape(-1, kw)
    payload = np.asarray(payload, np.uint8).reshape(len(row_keys), -1) if len(row_keys) else np.zeros((0, 0), np.uint8)
    count_of = {_value(k): int(c) for k, c in zip(key_keys, key_counts)}
    in_rows = {_value(k) for k in row_keys}
    body, v = [], np.zeros(len(row_keys), np.uint32)
    for i, k in enumerate(row_keys):
        c = count_of.get(_value(k))
        if c is None:
            continue
        v[i] = c if mode == MODE_COUNT else 1
        body.append(k.tobytes() + payload[i].tobytes() + (np.uint32(c).tobytes() if mode == MODE_COUNT else b""))
    absent = sorted(x for x in count_of if x not in in_rows)
    ak = np.array([[(x >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(kw)] for x in absent], np.uint64).reshape(-1, kw)
    ac = np.array([count_of[x] for x in absent], np.uint32)
    return b"".join(body), v, ak, ac


def sort_keys(keys):
    """distinct keys uint64[n, kw] in ascending order, most significant word first"""
    keys = np.unique(np.asarray(keys, np.uint64).reshape(len(keys), -1), axis=0)
    return np.ascontiguousarray(keys[np.lexsort([keys[:, j] for j in range(keys.shape[1])])])


def matrix_body(row_keys, payload):
    """the matrix body of those rows: key words, then the payload"""
    row_keys = np.asarray(row_keys, np.uint64)
    if not len(row_keys):
        return b""
    payload = np.asarray(payload, np.uint8).reshape(len(row_keys), -1)
    return np.concatenate([row_keys.view(np.uint8).reshape(len(row_keys), -1), payload], axis=1).tobytes()


def payload_bytes(n_cols, mode):
    return 4 * n_cols if mode == MODE_COUNT else (n_cols + 7) // 8


def split_body(body, kw, n_cols, mode):
    """a matrix body -> (row_keys uint64[n, kw], payload uint8[n, p])"""
    rb = 8 * kw + payload_bytes(n_cols, mode)
    a = np.frombuffer(body, np.uint8).reshape(-1, rb)
    return np.ascontiguousarray(a[:, :8 * kw]).view(np.uint64).reshape(-1, kw), np.ascontiguousarray(a[:, 8 * kw:])


def synth_case(seed, n_rows, n_cols, kw, mode, keep, key_ratio=1.0, shape="uniform", extreme=False):
    """a seeded matrix and key list: n_rows rows of one of synth.py's full-width key shapes; the key list holds a share `keep` of
    the rows' k-mers (0 ... 1) and is key_ratio times as long as the matrix (the rest of it k-mers of no row: the lists of two more
    draws of the same shape).  extreme: counts of 2^32 - 1 in the key and in the rows.
    -> (row_keys, payload, key_keys, key_counts)"""
    from synth import synth_wide_lists
    rng = np.random.default_rng(seed)
    n_key = max(int(n_rows * key_ratio), 0)
    pool = sort_keys(np.concatenate([l[0] for l in synth_wide_lists(seed, 1, n_rows + n_key + 8, 1.0, 0, kw=kw, shape=shape)]))
    idx = rng.permutation(len(pool))
    row_idx = np.sort(idx[:min(n_rows, len(pool))])
    row_keys = pool[row_idx]
    n_shared = min(int(round(len(row_keys) * keep)), n_key) if keep < 1 else len(row_keys)
    shared = rng.choice(row_idx, n_shared, replace=False) if n_shared else np.zeros(0, np.int64)
    other = idx[len(row_idx):len(row_idx) + max(n_key - n_shared, 0)]
    key_idx = np.sort(np.concatenate([shared, other]).astype(np.int64))
    key_keys = pool[key_idx]
    key_counts = rng.integers(1, 1000, len(key_keys), dtype=np.uint32)
    if mode == MODE_COUNT:
        cols = rng.integers(0, 300, (len(row_keys), n_cols), dtype=np.uint32)
        if extreme:
            cols[rng.random(cols.shape) < 0.2] = 0xFFFFFFFF
        payload = cols.view(np.uint8).reshape(len(row_keys), 4 * n_cols)
    else:
        payload = rng.integers(0, 256, (len(row_keys), (n_cols + 7) // 8), dtype=np.uint8)
    if extreme and len(key_counts):
        key_counts[rng.random(len(key_counts)) < 0.3] = 0xFFFFFFFF
    return row_keys, np.ascontiguousarray(payload), key_keys, key_counts
