"""The k-mer search as a plain model (test infrastructure): what csrc/kmer.hip's header comment says the count and
select kernels compute, over any CSR index and any query of IUPAC masks, with no notion of how the kernels go about
it.  tests/test_kmer_cpu.py pins it to the oracle's Index.scores / Index.find; tests/kmer_cases.py takes every
expected result from here."""
import numpy as np


def window_values(qmask, k, fast):
    """K(query), with multiplicity: the value of every window of k unambiguous bases that does not end on the last
    base (base codes A G C T/U = 0 1 2 3 by the bit of the mask, first base most significant); with `fast` only the
    windows that start with A."""
    m = np.asarray(qmask, np.int64) & 0x0f
    code = np.full(len(m), -1, np.int64)
    for c in range(4):
        code[m == (1 << c)] = c
    n_win = len(m) - k                      # starts 0 .. len - k - 1: the window on the last base is never produced
    if n_win <= 0:
        return np.zeros(0, np.int64)
    v = np.zeros(n_win, np.int64)
    ok = np.ones(n_win, bool)
    for x in range(k):
        cx = code[x:x + n_win]
        ok &= cx >= 0
        v = (v << 2) | np.maximum(cx, 0)
    if fast:
        ok &= code[:n_win] == 0
    return v[ok]


def scores(csr_off, csr_ids, n_refs, qmask, k, fast):
    """score[r] = sum over K(query), with multiplicity, of [r in list(window)] -- int64."""
    off = np.asarray(csr_off, np.int64)
    out = np.zeros(n_refs, np.int64)
    vals, mult = np.unique(window_values(qmask, k, fast), return_counts=True)
    for v, c in zip(vals.tolist(), mult.tolist()):
        np.add.at(out, np.asarray(csr_ids[off[v]:off[v + 1]], np.int64), c)
    return out


def topk(score_row, mx):
    """The first min(mx, n_refs) references in the order (score descending, id descending): (ids uint32, scores
    float32)."""
    s = np.asarray(score_row, np.int64)
    ids = np.arange(len(s), dtype=np.int64)
    order = np.lexsort((-ids, -s))[:min(mx, len(s))]
    return order.astype(np.uint32), s[order].astype(np.float32)
