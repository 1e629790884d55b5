"""tests/tied_reads.py's sweep against the oracle, without a GPU: every case lies in the class it names (measured from the oracle's output),
the sweep covers every size class of every key type and every tie word, a plain restatement of the count (a dict, integers sorted) equals
the oracle, and three wrong restatements -- the mistakes the sweep is there to catch -- differ from it on every case they apply to."""
import numpy as np
import pytest

import orc
import tied_reads as T

IDS = [c["id"] for c in T.CASES]


def _ints(keys):
    keys = np.asarray(keys, dtype=np.uint64).reshape(len(keys), -1)
    return [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in keys.tolist()]


def _oracle(case, hard_min):
    p = T.tied_partition(case)
    ek, ec = orc.count_kmer(T.batch(case)[2][p][0], case["k"], hard_min)
    return list(zip(_ints(ek), ec.tolist()))


def _decoded(case):
    p = T.tied_partition(case)
    return _ints(orc.superk_decode(T.batch(case)[2][p][0], case["k"]))


def _runs(vals, same):
    out = []
    for v in vals:
        if out and same(out[-1][0], v):
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(v, n) for v, n in out]


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_case_lies_in_its_class(case):
    k, kt, kind = case["k"], T.key_type(case["k"]), case["kind"]
    d = T.batch(case)[3][T.tied_partition(case)]
    kw = orc.kw_of_k(k)
    assert d["nkeys"] > T.CS_TARGET, d                       # (a partition of several buckets)
    assert T.size_class(kt, d["group_keys"]) == case["cls"], d
    if kind == "tied" and case["cls"] != "above-cap":        # (the group's bucket also holds the other keys up to the next splitter: half the aimed size of room)
        assert T.size_class(kt, d["group_keys"] + T.CS_TARGET // 2) == case["cls"], d
    if kind == "tied" and k != 16:
        assert d["words"] == {case["word"]} and 0.1 <= d["kept2"] <= 0.9, d
        assert case["word"] < (kw - 2 if kw >= 3 else kw - 1 if kw == 2 else 1)      # (below the splitter's words)
    if kind == "top-only":                                   # the top word ties, the splitters' second word decides: more than one bucket kernel's worth
        assert d["top_group"] > T.LDS_MID and d["top_words"] == {kw - 2} and case["word"] == kw - 2, d
    if kind == "lut-same":
        assert d["tvals"] == 1 and d["tspan"] == 0 and d["distinct"] == d["group"], d
    if kind == "lut-narrow":
        assert d["tvals"] > 1 and d["tspan"] < T.CS_LUT, d
    if kind == "lut-wide":
        assert T.CS_LUT <= d["tspan"] < 4 * T.CS_LUT, d
    if kind.startswith("lut-"):                              # the partition holds the tied reads' k-mers alone
        assert d["distinct"] == case["n"] and k <= 32, d


def test_sweep_covers_every_class():
    seen = {kt: set() for kt in T.KEY_TYPES}
    words = {kt: set() for kt in T.KEY_TYPES}
    ks = {kt: set() for kt in T.KEY_TYPES}
    top_only, luts = set(), set()
    for c in T.CASES:
        kt = T.key_type(c["k"])
        d = T.batch(c)[3][T.tied_partition(c)]
        ks[kt].add(c["k"])
        if c["kind"] == "tied":
            seen[kt].add(T.size_class(kt, d["group_keys"]))
            words[kt] |= d["words"]
        if c["kind"] == "top-only":
            top_only.add(kt)
        if c["kind"].startswith("lut-"):
            luts.add(c["kind"])
    for kt in T.KEY_TYPES:
        assert seen[kt] == set(T.classes_of(kt)), (kt, seen[kt])
    assert words["wide3"] == {0} and words["wide4"] == {0, 1} and words["u128"] == {0}
    assert top_only == {"wide3", "wide4"} and luts == {"lut-same", "lut-narrow", "lut-wide"}
    assert ks["wide3"] >= {65, 80, 96} and ks["wide4"] >= {97, 111, 127} and ks["u128"] >= {33, 47, 63} and ks["u64"] >= {16, 31, 32}
    assert T.CAP == {"u64": 4096, "u128": 4096, "wide3": 2048, "wide4": 2048}


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_plain_restatement_equals_the_oracle(case):
    tally = {}
    for v in _decoded(case):
        tally[v] = tally.get(v, 0) + 1
    for hard_min in (1, 2):
        assert sorted((v, n) for v, n in tally.items() if n >= hard_min) == _oracle(case, hard_min)
    kept1, kept2 = len(_oracle(case, 1)), len(_oracle(case, 2))
    assert 0 < kept2 < kept1


def _splitter_int(v, k):
    kw = orc.kw_of_k(k)
    return v >> (64 * (kw - 2)) if kw >= 3 else v >> 64 if kw == 2 else v >> T.tshift_of(k)


WRONG = {
    # a compare that ignores word 0 (sort and run boundaries)
    "compare-ignores-word-0": lambda vals, k: _runs(sorted(vals, key=lambda v: v >> 64), lambda a, b: a >> 64 == b >> 64),
    # the order right, a run boundary decided on the splitter's words alone
    "run-boundary-on-the-splitter": lambda vals, k: _runs(sorted(vals), lambda a, b: _splitter_int(a, k) == _splitter_int(b, k)),
    # the top word sorted, the words below it left in input order: what a low-word radix pass that is not stable leaves
    "top-word-then-input-order": lambda vals, k: _runs(sorted(vals, key=lambda v: v >> (64 * (orc.kw_of_k(k) - 1))), lambda a, b: a == b),
}


def applies(wrong, case):
    """the key types a wrong restatement can be told apart on: keys of one word have no word below the top one, and at k = 16 the
    splitter's table bits are the whole key; a compare that ignores word 0 is right where every pair of keys differs in a word above it
    (the word-1 cases of four-word keys, the top-only cases); a run boundary on the splitter is right where no two keys share it"""
    if wrong == "run-boundary-on-the-splitter":
        return case["k"] > 16 and case["kind"] != "top-only"
    if wrong == "compare-ignores-word-0":
        return case["k"] > 32 and case["kind"] == "tied" and case["word"] == 0
    return case["k"] > 32


@pytest.mark.parametrize("wrong,case", [(w, c) for w in sorted(WRONG) for c in T.CASES if applies(w, c)],
                         ids=[f"{w}-{c['id']}" for w in sorted(WRONG) for c in T.CASES if applies(w, c)])
def test_wrong_restatements_differ_from_the_oracle(wrong, case):
    assert WRONG[wrong](_decoded(case), case["k"]) != _oracle(case, 1)


def test_wrong_restatements_apply_to_every_key_type_they_can():
    for w in WRONG:
        kts = {T.key_type(c["k"]) for c in T.CASES if applies(w, c)}
        assert kts >= {"u128", "wide3", "wide4"} and (w != "run-boundary-on-the-splitter" or "u64" in kts)
