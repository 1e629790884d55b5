"""The synthetic lists the parity tests draw (tests/synth.py): the draws of existing call signatures are pinned, so that a change to the
generator cannot quietly change what those tests merge; the full-width shapes hold what their names promise."""
import hashlib
import pytest

from synth import synth_lists, synth_wide_lists, SHAPES, max_canonical, key_value, canonical_value

# (arguments, keywords, sha256 of every list's keys, counts and key shape, first 16 hex digits)
PINNED = [((1, 64, 2000, 0.9, 40), {}, "7d7d4dfa17dec537"),
          ((1234 + 17, 17, 1500, 0.8, 50), dict(kw=1), "d827df4f3ada3fa8"),
          ((77 + 50, 50, 800, 0.9, 30), dict(kw=2, key_bits=126), "c777a2391a5e5c88"),
          ((31 * 3 + 50, 50, 800, 0.9, 30), dict(kw=3, key_bits=192), "0f663193b46a515f"),
          ((31 * 4 + 2, 2, 2500, 0.6, 700), dict(kw=4, key_bits=254), "c2b6172ceaaf54c3"),
          ((4000, 300, 3000, 0.95, 40), dict(kw=2, key_bits=100, ragged=True), "a4aa98af5adcbd95"),
          ((9100, 200, 3000, 0.9, 40), dict(kw=1, count_max=254), "850076756908fb07")]


def _digest(lists):
    h = hashlib.sha256()
    for k, c in lists:
        h.update(k.tobytes()); h.update(c.tobytes()); h.update(str(k.shape).encode())
    return h.hexdigest()[:16]


@pytest.mark.parametrize("args,kws,digest", PINNED)
def test_existing_synth_draws_are_unchanged(args, kws, digest):
    assert _digest(synth_lists(*args, **kws)) == digest


def test_max_canonical():
    """G^16 C^16 = 0xFFFFFFFF55555555 (k = 32); k = 64: an all-ones most significant word over 0x5555555555555555"""
    assert max_canonical(1) == 0xFFFFFFFF55555555
    assert max_canonical(2) == (0xFFFFFFFFFFFFFFFF << 64) | 0x5555555555555555
    assert max_canonical(3) == (0xFFFFFFFFFFFFFFFF << 128) | (0xFFFFFFFF55555555 << 64) | 0x5555555555555555
    assert canonical_value("G" * 16 + "C" * 16) == max_canonical(1)      # (its own reverse complement)
    assert canonical_value("G" * 32 + "C" * 32) == max_canonical(2)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kw", [1, 2, 3, 4])
def test_full_width_shapes(kw, shape):
    lists = synth_wide_lists(3, 12, 400, 0.9, 30, kw=kw, shape=shape)
    assert len(lists) == 12 and all(k.shape[1] == kw and len(k) == len(c) for k, c in lists)
    vals = []
    for k, _ in lists:
        v = [key_value(r) for r in k]
        assert all(a < b for a, b in zip(v, v[1:]))          # strictly ascending, most significant word first
        vals += v
    top = [v >> (64 * (kw - 1)) for v in vals]
    lo = [v & ((1 << 64) - 1) for v in vals]
    if shape == "uniform":
        assert sum(t >> 63 for t in top) > len(top) // 3 and sum(((t >> 62) & 1) for t in top) > len(top) // 3
    elif shape == "straddle":
        assert min(top) < 1 << 63 <= max(top) and max(abs(t - (1 << 63)) for t in top) < 1 << 20
    elif shape == "near-max":
        mx = max_canonical(kw)
        assert max(vals) == mx and mx - 1 in vals and min(vals) > mx - (1 << 66)
    elif shape == "low-word-only":
        assert kw == 1 or (len(set(top)) == 1 and top[0] >> 63)
        s = set(lo)
        assert sum(1 for x in s if x >> 63 and (x ^ (1 << 63)) in s) > 10      # low words that differ in bit 63 alone
    else:
        assert min(vals) == 0 and 1 in vals and max(top) == (max(vals) if kw == 1 else 0)


@pytest.mark.parametrize("args,digest", [((21, 21, 300, 28), "30ed913cd81c4971"), ((127, 127, 300, 124), "5c0d5aa55f083807")])
def test_existing_superk_streams_are_unchanged(args, digest):
    """the record streams the count restatements draw (synth_superk_stream) are pinned as well"""
    from synth import synth_superk_stream
    recs, cnt = synth_superk_stream(*args)
    h = hashlib.sha256(recs); h.update(repr(sorted(cnt.items())).encode())
    assert h.hexdigest()[:16] == digest


def test_window_shapes():
    """the hash windows are what their names promise: window * P on the named side of 2^63 / 2^64, the sparse ids, and the all-ones key
    for the chosen hash in the chosen partition (both constructions)"""
    from synth import WINDOW_SHAPES, hash_window, U64
    x = 0x1234_5678_9ABC_DEF0
    for P in (2, 3, 4, 8, 37):
        got = {s: hash_window(s, P, x, at=P - 1) for s in WINDOW_SHAPES}
        assert all(len(ids) == P and all(0 <= i <= U64 for i in ids) and 0 < W <= U64 for W, ids in got.values())
        assert got["2^32-1"][0] == (1 << 32) - 1 and got["2^32"][0] == 1 << 32 and got["2^32+64"][0] == (1 << 32) + 64 and got["2^40"][0] == 1 << 40
        assert got["below-2^63"][0] * P < 1 << 63 < got["above-2^63"][0] * P and got["above-2^63"][0] * P - (1 << 63) <= P
        assert got["below-2^64"][0] * P < 1 << 64 < got["above-2^64"][0] * P and got["above-2^64"][0] * P - (1 << 64) <= P
        assert {0, 65535, 1 << 32, U64} <= set(got["sparse-ids"][1]) or P < 4
        for s in ("all-ones-top", "all-ones-one"):
            W, ids = got[s]
            assert (x % W + W * ids[P - 1]) & U64 == U64
