"""The helix base-pair score (align_bp_score_slv) restated plainly, as the yardstick of tests/test_bps_cpu.py and
tests/test_gpu_bps.py: a loop over the map's columns, the character of a column by bisection over the sequence's
words, the score in numpy float64 / float32.  Shares no code with the product."""
import bisect

import numpy as np

_UPPER = ".AGRCMSVUWKDYHBN"
TABLE = _UPPER + _UPPER.lower()          # the RNA IUPAC character of the five mask bits; no mask bits: '.'
WEIGHTS = (("AG", 0.5), ("AU", 1.1), ("CG", 1.5), ("GG", 0.4), ("GU", 0.9))


def char_at(cols, words, c):
    """cols: the words' columns (bits 0-23), in sequence order."""
    if c >= 1 << 24:
        return "-"                       # a column no word can hold
    i = bisect.bisect_left(cols, c)      # the first word whose column is >= c
    if i < len(cols) and cols[i] == c:
        return TABLE[(int(words[i]) >> 24) & 31]
    return "-"


def counts(words, pairs):
    """[num, AG, AU, CG, GG, GU] of one sequence (packed words) under the helix map `pairs`."""
    words = [int(w) for w in words]
    cols = [w & 0xFFFFFF for w in words]
    out = [0] * 6
    for i, p in enumerate(pairs):
        p = int(p)
        if p == 0:
            continue
        l, r = char_at(cols, words, i), char_at(cols, words, p)
        if l == "." or r == "." or (l == "-" and r == "-"):
            continue
        out[0] += 1
        pair = "".join(sorted((l, r)))
        for k, (name, _) in enumerate(WEIGHTS):
            if pair == name:
                out[1 + k] += 1
    return out


def score(c):
    """float32 score of the six counters: a double sum, left to right, rounded once; then a float32 division.
    num == 0 gives 0."""
    if c[0] == 0:
        return np.float32(0)
    s = np.float64(0)
    for k, (_, w) in enumerate(WEIGHTS):
        term = np.float64(c[1 + k]) * np.float64(w)
        s = term if k == 0 else s + term
    return np.float32(np.float32(s) / np.float32(c[0]))


def attr(sc):
    """align_bp_score_slv: the float32 product 100 * score, truncated."""
    return int(np.float32(100) * np.float32(sc))


def bits(x):
    return np.float32(x).tobytes()
