"""The super-k-mer split restated over STRINGS and Python integers (no words, no bit planes, no rolling state; nothing shared with
oracle/kmx_oracle.c), and the inputs of the phase sweep: `PAIRS`, one (k, m) for every window width nbm = k - m + 1 the two
split kernels can be given, and `phase_batch`, reads that move every event of the split through every lane of a chunk.

The rules (Model.hpp:1010-1070, 1220-1251; Sequence2SuperKmer.hpp:80-158; fill_partitions.hpp:59-105):
  * a k-mer is valid when it holds only ACGT (lower case counts as upper case);
  * an m-mer's value is the smaller of forward and reverse complement in the code A0 C1 T2 G3, replaced by 4^m - 1 when AA occurs
    anywhere but at the leading position;
  * a k-mer's minimizer is the minimum over its k - m + 1 m-mers;
  * a super-k-mer is a maximal run of valid k-mers with one minimizer, cut every maxs k-mers;
  * a k-mer is forward when it is smaller than its reverse complement (a palindrome counts as reverse); a super-k-mer's k-mers fall into
    runs of one strand, those into pieces of at most 5: the kx-mers.
A nucleotide is a digit character here ("0123" = ACTG), a k-mer a string of them: strings of one length compare as their values do."""
import itertools

import numpy as np

_DIGITS = str.maketrans("ACTG", "0123")
_COMP = str.maketrans("0123", "2301")      # A <-> T, C <-> G
PINFO_WIDTH = 2 + 5 * 256
WHY = ("min", "invalid", "maxs", "end")
EVENTS = WHY + ("strand", "five")
WRONG = ("short-window", "maxs+1", "phase")      # the deliberately wrong variants (test_superk_phases_cpu.py)


def maxs_of(k):
    """k-mers a super-k-mer holds at most: (bits of the k-mer type - 8) / 2, one byte for the number (Sequence2SuperKmer.hpp:146)"""
    bits = 64 if k < 32 else 128 if k < 64 else 192 if k < 96 else 256
    return min((bits - 8) // 2, 255)


def own_of(k, m):
    """k-mer positions a chunk of the split kernels owns (restated from superk.hip, not read from it): a wave holds 64 positions and looks
    one k-mer ahead; up to 32 m-mers a window, the window has to end inside the 64, beyond that the next 64 positions are at hand"""
    nbm = k - m + 1
    return 64 - nbm if nbm <= 32 else 63


def _mmer(s, dflt, cache):
    """the value of the m-mer s (digits), None when it is none"""
    v = cache.get(s)
    if v is None and s not in cache:
        if s.strip("0123"):
            v = None
        else:
            name = min(s, s[::-1].translate(_COMP))
            v = dflt if "00" in name[1:] else int(name, 4)
        cache[s] = v
    return v


def superkmers(read, k, m, wrong=None, _cache=None):
    """the super-k-mers of one read, in order: [(start, n, minimizer, why it ended, strands)], start = the position of its first k-mer,
    strands[t] = k-mer start + t is forward.  wrong: one of WRONG"""
    d = read.upper().translate(_DIGITS)
    L, nk = len(d), len(d) - k + 1
    if nk <= 0:
        return []
    rc = d[::-1].translate(_COMP)                  # the read's reverse complement: the one of d[j:j + k] is rc[L - j - k:L - j]
    cache = {} if _cache is None else _cache
    dflt, none = 4 ** m - 1, 4 ** m
    mv = [_mmer(d[i:i + m], dflt, cache) for i in range(L - m + 1)]
    mv = [none if v is None else v for v in mv]
    nbm = k - m + 1 - (1 if wrong == "short-window" else 0)
    maxs = maxs_of(k) + (1 if wrong == "maxs+1" else 0)
    own = own_of(k, m)
    bad = [0] * (L + 1)
    for i, c in enumerate(d):
        bad[i + 1] = bad[i] + (c not in "0123")
    out, start, cur = [], None, None

    def close(end, why):
        out.append((start, end - start, cur, why, tuple(d[t:t + k] < rc[L - t - k:L - t] for t in range(start, end))))

    for j in range(nk):
        if bad[j + k] - bad[j]:
            if start is not None:
                close(j, "invalid"); start = None
            continue
        mini = min(mv[j:j + nbm]) if nbm else dflt
        if start is not None:
            if mini != cur and not (wrong == "phase" and (j - 1) % own == 0):
                close(j, "min"); start = None
            elif j - start >= maxs:
                close(j, "maxs"); start = None
        if start is None:
            start, cur = j, mini
    if start is not None:
        close(nk, "end")
    return out


def pieces(strands):
    """a super-k-mer's kx-mers: [(first k-mer, k-mers, forward)], runs of one strand cut every 5"""
    out, t = [], 0
    for fwd, grp in itertools.groupby(strands):
        n = len(list(grp))
        for a in range(0, n, 5):
            out.append((t + a, min(5, n - a), fwd))
        t += n
    return out


def events(sks):
    """(event, position of the last k-mer before the cut) for a read's super-k-mers: the four ways a super-k-mer ends, a change of strand
    inside a super-k-mer, a cut of a strand run at 5 k-mers"""
    for start, n, _, why, strands in sks:
        yield why, start + n - 1
        ps = pieces(strands)
        for (a, x, fwd), (b, _, fwd2) in zip(ps, ps[1:]):
            yield ("five" if fwd == fwd2 else "strand"), start + b - 1


def record(d, k):
    """the record of the len(d) - k + 1 consecutive k-mers of d (digits): [u8 n][2-bit nucleotides], the first k-mer's value (its first
    nucleotide in the top digit) with the nucleotides that follow at digits k, k + 1, ..., little endian"""
    n = len(d) - k + 1
    S = int(d[:k], 4)
    if n > 1:
        S |= int(d[k:][::-1], 4) << (2 * k)
    return bytes([n]) + S.to_bytes((k + n - 1 + 3) // 4, "little")


class Split:
    """what the split of a batch leaves: streams[p] (bytes), nk[p], pinfo[p][PINFO_WIDTH], {minimizer: number} ms (super-k-mers),
    mk (k-mers), mx (kx-mers); sks[read] = superkmers(read)"""

    def __init__(self, reads, k, m, repart, nb_parts, wrong=None):
        self.k, self.m, self.P = k, m, nb_parts
        self.streams = [bytearray() for _ in range(nb_parts)]
        self.nk = [0] * nb_parts
        self.pinfo = [[0] * PINFO_WIDTH for _ in range(nb_parts)]
        self.ms, self.mk, self.mx = {}, {}, {}
        self.sks = []
        cache = {}
        for read in reads:
            if not isinstance(read, str):
                read = read.decode()
            sks = superkmers(read, k, m, wrong, cache)
            self.sks.append(sks)
            if not sks:
                continue
            d = read.upper().translate(_DIGITS)
            rc, L = d[::-1].translate(_COMP), len(d)
            for start, n, mini, _, strands in sks:
                p = int(repart[mini])
                self.streams[p] += record(d[start:start + n + k - 1], k)
                self.nk[p] += n
                self.ms[mini] = self.ms.get(mini, 0) + 1
                self.mk[mini] = self.mk.get(mini, 0) + n
                row = self.pinfo[p]
                for a, x, fwd in pieces(strands):
                    t = start + (a if fwd else a + x - 1)      # the piece's first k-mer if forward, its last one if reverse
                    radix = int(min(d[t:t + k], rc[L - t - k:L - t])[:4], 4)
                    row[0] += x; row[1] += 1; row[2 + (x - 1) * 256 + radix] += 1
                    self.mx[mini] = self.mx.get(mini, 0) + 1

    def table(self, which):
        """ms / mk / mx as the dense uint64[4^m] table the C ABIs fill"""
        t = np.zeros(4 ** self.m, dtype=np.uint64)
        for v, n in getattr(self, which).items():
            t[v] = n
        return t

    def pinfo_array(self):
        return np.array(self.pinfo, dtype=np.uint64).reshape(self.P, PINFO_WIDTH)


# ---- the inputs of the sweep -----------------------------------------------------------------------------------------------------------
def _bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def phase_batch(k, seed):
    """64 shifted copies of one base read -- random bases, a poly-A stretch longer than maxs k-mers (one minimizer, every k-mer forward: cuts
    at maxs and every 5), random bases, an N, random bases -- behind the last j = 0 .. 63 bases of one 64-mer: every event of the base read
    passes every position modulo a chunk's owned positions.  Then the edge reads."""
    rng = np.random.default_rng(seed)
    head = _bases(rng, 64)
    base = _bases(rng, 70) + "A" * (k + maxs_of(k) + 8) + _bases(rng, 40) + "N" + _bases(rng, k + 50)
    reads = [head[64 - j:] + base for j in range(64)]
    reads += ["", _bases(rng, k - 1), _bases(rng, k), "T" * k, "ACGTN" * 40, _bases(rng, 2 * k + 30).lower()]
    return reads


def seed_of(k, m):
    return 1000 * k + m


def _grid():
    pairs = []
    for nbm in range(1, 61):                      # k <= 63 (k_superk_wave): m varied over 4 .. 10 as far as 8 <= k <= 63 lets it
        m = min(max(4 + nbm % 7, 9 - nbm, 4), 10, 64 - nbm)
        pairs.append((nbm + m - 1, m))
    for nbm in range(50, 125):                    # k >= 64 (k_superk_wide); 50 .. 54 exist at k = 64, m = 15 .. 11 only
        m = min(max(4 + nbm % 7, 65 - nbm, 4), 10, 128 - nbm) if nbm >= 55 else 65 - nbm
        pairs.append((nbm + m - 1, m))
    pairs += [(41, 10), (42, 10)]                 # nbm = 32, 33 at the default m as well: the last narrow width and the first wide one
    pairs += [(k, m) for k in (8, 15, 31, 32, 63, 64, 95, 96, 127) for m in (4, 10) if m <= k]
    return sorted(set(pairs))


PAIRS = _grid()
