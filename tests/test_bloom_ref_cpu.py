"""The judge of the Bloom merge tests, judged (CPU): oracle/kmx_oracle.c's Bloom writers against tests/bloom_ref.py, a restatement per
hash with Python integers.  The hand-worked vectors of test_merge_independent.py pin three samples, 15 rows and field widths 2 and 3;
here the two restatements meet at every field width the product writes, at windows that are no multiple of 8, at one to 513 samples,
at counts where to_n_b changes or caps, and on the list layouts of test_merge_bloom_gpu.py at that file's sizes."""
import pytest

import orc
from bloom_ref import bloom_expected, layout, cohort, arrays, soft_mins, MODE_BF, MODE_BFC, MODE_BFT
from test_merge_independent import BLOOM_LISTS, BLOOM_SOFT, BLOOM_LOWER, BLOOM_UPPER, bloom_cases

PAIRS = [(1, 0), (0, 0), (2, 0), (2, 2), (1, 1), (3, 1)]
BITW = [1, 2, 3, 4, 5, 6, 7, 8, 13, 16, 17, 31, 32]


def agree(lists, soft, r, s, mode, lower, W, bitw=2):
    exp = bloom_expected(lists, soft, r, s, mode, lower, lower + W - 1, bitw)
    got = orc.merge_matrix(arrays(lists), 1, soft, r, s, mode, lower, lower + W - 1, bitw)
    assert got[1] == exp[1], (mode, r, s, bitw)
    assert got[0] == exp[0], (mode, r, s, bitw)
    assert got[2].tolist() == exp[2], (mode, r, s, bitw)
    return exp


@pytest.mark.parametrize("case", range(12))
def test_second_restatement_reproduces_the_hand_worked_bloom_vectors(case):
    mode, r, s, w, body, stats = bloom_cases()[case]
    got, rows, st = bloom_expected(BLOOM_LISTS, BLOOM_SOFT, r, s, mode, BLOOM_LOWER, BLOOM_UPPER, w)
    assert got == body and st == stats
    assert rows == (8 if mode == orc.MODE_BFT else 15)


def test_modes_are_the_oracles():
    assert (MODE_BF, MODE_BFC, MODE_BFT) == (orc.MODE_BF, orc.MODE_BFC, orc.MODE_BFT)


@pytest.mark.parametrize("W", [1, 7, 8, 63, 64, 65, 200])
@pytest.mark.parametrize("N", [1, 2, 3, 7, 8, 9, 13, 64, 65, 77, 513])
def test_oracle_bloom_writers_against_the_second_restatement(N, W):
    """every (recurrence-min, share-min) pair; BF, BFT and BFC -- at every field width up to 77 samples, at two widths per pair
    beyond --; soft-mins up to 2^32 - 1, a tenth of the counts extreme; window at 0 and at 3 W"""
    lists = cohort(1000 * N + W, N, 0, W, 0.3, extreme=True)
    soft = soft_mins(N)
    some = 0
    for k, (r, s) in enumerate(PAIRS):
        lower = 3 * W * (k & 1)
        ls = [{h + lower: c for h, c in l.items()} for l in lists]
        e = agree(ls, soft, r, s, orc.MODE_BF, lower, W)
        some += any(e[0])
        agree(ls, soft, r, s, orc.MODE_BFT, lower, W)
        for w in (BITW if N <= 77 else (BITW[k], BITW[k + 6], 32)):
            agree(ls, soft, r, s, orc.MODE_BFC, lower, W, w)
    assert some or W * N < 8      # (not all of it trivially empty)


def test_to_n_b_of_the_two_restatements():
    """min(bit length, 2^w - 1) at every power of two and its neighbours, every width: w = 4 caps from 2^15, w = 5 from 2^31"""
    for w in range(1, 33):
        for k in range(32):
            for c in {max(1, (1 << k) - 1), 1 << k, (1 << k) + 1, 0xFFFFFFFF}:
                exp = min(c.bit_length(), (1 << w) - 1)
                assert orc.to_n_b(c, w) == exp, (c, w)
                body, _, _ = bloom_expected([{5: c}], [1], 1, 0, orc.MODE_BFC, 5, 5, w)
                assert int.from_bytes(body, "big") >> (8 * len(body) - w) == exp
    assert orc.to_n_b((1 << 15) - 1, 4) == 15 and orc.to_n_b(1 << 15, 4) == 15 and orc.to_n_b(1 << 14, 4) == 15 and orc.to_n_b((1 << 14) - 1, 4) == 14
    assert orc.to_n_b((1 << 31) - 1, 5) == 31 and orc.to_n_b(1 << 31, 5) == 31 and orc.to_n_b(1 << 31, 6) == 32


# the layouts at the sizes test_merge_bloom_gpu.py runs them at
@pytest.mark.parametrize("kind", ["uniform", "clustered", "ends", "edges"])
@pytest.mark.parametrize("mode,bitw,N,W,per,step", [(orc.MODE_BF, 2, 64, 12 * 5120 + 37, 2200, 64), (orc.MODE_BFC, 2, 64, 12 * 2560 + 37, 2200, 64),
                                                    (orc.MODE_BFT, 2, 100, 20 * 1024 + 100, 400, 256)])
def test_oracle_on_the_layouts(kind, mode, bitw, N, W, per, step):
    lower = 3 * W
    lists = layout(kind, 7 + N, N, lower, W, per, step)
    rows = sorted(h - lower for l in lists for h in l)
    assert rows[0] >= 0 and rows[-1] < W and (rows[-1] == W - 1 or kind != "edges")
    if kind == "clustered":
        assert all(max(l) - min(l) < per * 4 // 3 and len(l) == per for l in lists)
    if kind == "ends":
        assert all((max(l) - lower < per * 9 // 8) if i % 2 == 0 else (min(l) - lower >= W - per * 9 // 8) for i, l in enumerate(lists))
    if kind == "edges":
        have = set(rows)
        assert sum(1 for m in range(step, W, step) if {m - 1, m} <= have) > 0.7 * (W // step)      # records on both sides of the tile boundaries
    soft = soft_mins(N)
    for r, s in [(1, 0), (2, 1), (3, 2)]:
        e = agree(lists, soft, r, s, mode, lower, W, bitw)
        assert any(e[0]) and (s == 0 or sum(e[2][1]) > 0)
