"""The k-mer index of a reference store as a plain build (test infrastructure): what sina_hip_build_index leaves on the
device (ref_kmer_keys, mark_unique, scatter_unique in sina_amd/csrc/kmer_index.hip), by its definition and with no
notion of how the kernels go about it -- no keys, no sort, no flags, no scan.  tests/test_index_cpu.py pins it to the
oracle's Index.csr(); tests/index_cases.py takes every expected index from here.

A reference is an array of mask bytes (iupac bits 0 .. 3, bit 4 lower case).  Reference r is in list v iff v is the value
of a window of k words of r that does not end on r's last word, every word of which has exactly one of its low four bits
set (an ambiguity code breaks the window, and so does a word without any bit), and -- in a fast index -- whose first base
is A.  Base codes A G C U = 0 1 2 3 by the bit, first base most significant.  r is in a list once, however often the
k-mer occurs in it; ids ascend.  The lower-case bit plays no part."""
import numpy as np

BASES = "AGCU"
CODE = np.full(16, -1, np.int64)                # by the low four mask bits: the base, or -1 for none and for several
CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]


def kmer_str(v, k):
    return "".join(BASES[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def window_values(mask, k, nofast):
    """The value of every window that counts, in the order of the windows (with repeats)."""
    code = CODE[np.asarray(mask, np.int64) & 0x0f]
    n_win = len(code) - k                       # the window on the last word is not one
    if n_win <= 0:
        return np.zeros(0, np.int64)
    v = np.zeros(n_win, np.int64)
    ok = np.ones(n_win, bool)
    for x in range(k):
        cx = code[x:x + n_win]
        ok &= cx >= 0
        v = v * 4 + np.maximum(cx, 0)
    if not nofast:
        ok &= code[:n_win] == 0
    return v[ok]


def build(seqs, k, nofast):
    """(off uint32[4^k + 1], ids uint32[n_postings]) of the references `seqs` (a list of mask arrays)."""
    lists = {}
    for r, mask in enumerate(seqs):
        for v in set(window_values(mask, k, nofast).tolist()):
            lists.setdefault(v, []).append(r)   # (r ascends with the loop)
    off = np.zeros((1 << (2 * k)) + 1, np.uint32)
    ids, lo = [], 0
    for v in sorted(lists):
        off[lo:v + 1] = len(ids)                # every list up to and including v starts here
        ids += lists[v]
        lo = v + 1
    off[lo:] = len(ids)
    return off, np.asarray(ids, np.uint32)


def first_difference(got_off, got_ids, want_off, want_ids, k):
    """None where the two indexes are equal, else a sentence that names the first differing list."""
    go, wo = np.asarray(got_off, np.int64), np.asarray(want_off, np.int64)
    if len(go) != len(wo):
        return "%d offsets, want %d" % (len(go), len(wo))
    if (go == wo).all() and len(got_ids) == len(want_ids) and (np.asarray(got_ids) == np.asarray(want_ids)).all():
        return None
    gl, wl = np.diff(go), np.diff(wo)
    bad = np.flatnonzero(gl != wl)
    if len(bad) == 0 and go[0] == wo[0] and len(got_ids) == len(want_ids):
        x = int(np.flatnonzero(np.asarray(got_ids) != np.asarray(want_ids))[0])
        bad = [int(np.searchsorted(wo, x, side="right")) - 1]
    if len(bad) == 0:
        return "offsets start at %d, want %d; %d ids, want %d" % (go[0], wo[0], len(got_ids), len(want_ids))
    v = int(bad[0])
    return "list %d (%s): got %s want %s; %d ids in all, want %d" % (
        v, kmer_str(v, k), np.asarray(got_ids)[go[v]:go[v + 1]][:20].tolist(), np.asarray(want_ids)[wo[v]:wo[v + 1]][:20].tolist(),
        len(got_ids), len(want_ids))
