"""Named reference stores for the tests of the device index build (ref_kmer_keys, mark_unique, scatter_unique, mark_dense,
fill_dense in sina_amd/csrc/kmer_index.hip) and of the store state around it, shared by tests/test_index_cpu.py (which
pins the plain build to the oracle on them) and tests/test_gpu_index.py (which builds them on the device).  Everything
here is CPU work.

A case is written down as text: one string per reference, A G C U (or T) and the ambiguity codes as letters, lower case
for the case bit, "." for a word without any base bit (mask 0).  A builder returns a Case -- the store's width, its
references, k, the nofast settings to build it under and its queries -- after asserting, in plain numpy over the masks
or over the plain index (tests/index_ref.py), that the store holds the edge it is named for.  The columns of the bases
play no part in the index: half the cases put gaps between them.

Numbers restated from the kernels: ref_kmer_keys runs one block of 256 threads per reference, each thread taking every
256th word; mark_unique and scatter_unique run 256 keys per block over all words of the store; fill_dense gives a list
to 64 lanes, 64 entries a trip, and sets bit r & 31 of word r >> 5."""
import functools

import numpy as np

from tests import index_ref
from tests import kmer_cases as kc
from tests import kmer_ref

BLOCK = 256                       # threads of ref_kmer_keys, keys per block of mark_unique / scatter_unique
LANES = 64                        # entries of a dense list per trip of fill_dense
LOWER = 16
MASK = {"A": 1, "G": 2, "C": 4, "U": 8, "T": 8, "M": 5, "R": 3, "W": 9, "S": 6, "Y": 12, "K": 10, "V": 7, "H": 13,
        "D": 11, "B": 14, "N": 15, ".": 0}
TWO_BIT, THREE_BIT, N = "R", "V", "N"
DENSE_DIVS = (None, "1", "1000000")
MAXES = (1, 41)
BOTH = (False, True)              # the nofast settings


def seq(text):
    """Mask bytes of a reference written as text."""
    return np.array([MASK[c.upper()] | (LOWER if c.islower() else 0) for c in text], np.uint8)


def text_of(rng, n, alphabet="AGCU"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n))


def value_of(kmer):
    v = 0
    for c in kmer:
        v = v * 4 + "AGCU".index(c)
    return v


def occurrences(text, kmer):
    """The starts at which `kmer` stands in `text`, by comparing strings."""
    return [s for s in range(len(text) - len(kmer) + 1) if text[s:s + len(kmer)].upper().replace("T", "U") == kmer]


def n_valid_windows(mask, k):
    """Windows of k words with exactly one base bit each that do not end on the last word, by a plain loop."""
    ok = [bin(int(m) & 15).count("1") == 1 for m in mask]
    return sum(all(ok[s:s + k]) for s in range(max(0, len(mask) - k)))


class Case:
    def __init__(self, name, texts, k, nofasts=BOTH, queries=(), gaps=False, mask0=False, dense_divs=DENSE_DIVS):
        self.name, self.k, self.nofasts, self.mask0 = name, int(k), tuple(nofasts), bool(mask0)
        self.dense_divs = tuple(dense_divs)
        self.texts = list(texts)
        self.seqs = [seq(t) if isinstance(t, str) else np.asarray(t, np.uint8) for t in texts]
        self.n_refs = len(self.seqs)
        assert self.n_refs >= 1
        rng = np.random.default_rng(len(name) + 7 * self.n_refs)
        self.cols = [np.cumsum(rng.integers(1, 4, size=len(s))) if gaps else np.arange(len(s)) for s in self.seqs]
        self.width = max([8] + [int(c[-1]) + 1 for c in self.cols if len(c)])
        self.maxes = MAXES
        # queries: every reference, one per distinct k-mer of the store (a seeded sample of 50 where there are more),
        # and the case's own; the same bytes once
        vals = np.flatnonzero(np.diff(self.plain(True)[0].astype(np.int64)))
        if len(vals) >= 50:
            vals = np.sort(rng.choice(vals, 50, replace=False))
        qs = [s.copy() for s in self.seqs] + [kc.query_of([int(v)], self.k) for v in vals] + [np.asarray(q, np.uint8) for q in queries]
        seen = {}
        for q in qs:
            seen.setdefault(q.tobytes(), q)
        self.qmasks = list(seen.values())
        for nofast in self.nofasts:
            kc.check_csr(_CsrView(self, nofast))

    # (sina_hip_kmer_topk takes the batch as one array)
    @property
    def qmask(self):
        return np.concatenate(self.qmasks) if self.qmasks else np.zeros(0, np.uint8)

    @property
    def qoff(self):
        off = np.zeros(len(self.qmasks) + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in self.qmasks])
        return off

    def packed(self):
        """(packed bases: column | mask << 24, offsets, width) for sina_hip_upload_refs."""
        off = np.zeros(self.n_refs + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in self.seqs])
        ab = np.zeros(int(off[-1]) + 1, np.uint32)                     # (never a null pointer: one word more than used)
        for r, (s, c) in enumerate(zip(self.seqs, self.cols)):
            ab[int(off[r]):int(off[r + 1])] = c.astype(np.uint32) | (s.astype(np.uint32) << 24)
        return ab[:int(off[-1])], off, self.width

    @functools.lru_cache(maxsize=None)
    def plain(self, nofast):
        return index_ref.build(self.seqs, self.k, nofast)

    def members(self, kmer, nofast=True):
        """The list of a k-mer given as text, from the plain index."""
        off, ids = self.plain(nofast)
        v = value_of(kmer)
        return ids[int(off[v]):int(off[v + 1])].tolist()

    def list_lengths(self, nofast):
        return np.diff(self.plain(nofast)[0].astype(np.int64))

    def n_dense_lists(self, nofast, dense_div):
        return int((self.list_lengths(nofast) > kc.dense_threshold(self.n_refs, dense_div)).sum())

    @functools.lru_cache(maxsize=None)
    def expected(self, nofast):
        """Per query the score vector and per max its (ids, scores): kmer_ref's over the plain index, computed once."""
        off, ids = self.plain(nofast)
        off = off.astype(np.int64)
        out = []
        for m in self.qmasks:
            s = kmer_ref.scores(off, ids, self.n_refs, m, self.k, not nofast)
            out.append(dict(scores=s, find={mx: kmer_ref.topk(s, mx) for mx in self.maxes}))
        return out

    def holds_mask0(self):
        return any(((s & 15) == 0).any() for s in self.seqs)

    def __repr__(self):
        return self.name


class _CsrView:
    """A plain index of a case in the shape kmer_cases.check_csr reads."""

    def __init__(self, case, nofast):
        self.name, self.k, self.n_refs, self.long_api = (case.name, nofast), case.k, case.n_refs, False
        self.off, self.ids = case.plain(nofast)
        self.qmasks, self.expected = case.qmasks, case.expected(nofast)


# ---------------------------------------------------------------- lengths around k

def lengths_around_k(k):
    """References of 0, 1, k - 1, k, k + 1 and k + 2 words: none, none, none, none, one and two windows."""
    rng = np.random.default_rng(9100 + k)
    lens = [0, 1, k - 1, k, k + 1, k + 2]
    c = Case("lengths_around_k_%d" % k, [text_of(rng, n) for n in lens], k, gaps=k % 4 == 2)
    assert [len(s) for s in c.seqs] == lens
    assert [n_valid_windows(s, k) for s in c.seqs] == [0, 0, 0, 0, 1, 2]
    off, ids = c.plain(True)
    assert set(ids.tolist()) == {4, 5} and 2 <= len(ids) <= 3
    return c


def empty_references():
    """An empty reference first, in the middle and last, and two in a row."""
    rng = np.random.default_rng(9110)
    texts = ["", text_of(rng, 30), "", "", text_of(rng, 9), text_of(rng, 41), ""]
    c = Case("empty_references", texts, 4, gaps=True)
    assert [len(s) for s in c.seqs] == [0, 30, 0, 0, 9, 41, 0]
    assert set(c.plain(True)[1].tolist()) == {1, 4, 5}
    return c


def last_window():
    """AGCU stands only in the last window of reference 0 (absent from its list), in the first window of reference 1
    (present), and in reference 2 both earlier and last (present); reference 3 is reference 1 with another last base:
    the two share every k-mer."""
    texts = ["GGGGGAGCU", "AGCUGGGGG", "AGCUCCAGCU", "AGCUGGGGC"]
    c = Case("last_window", texts, 4)
    assert occurrences(texts[0], "AGCU") == [len(texts[0]) - 4] and occurrences(texts[1], "AGCU") == [0]
    assert occurrences(texts[2], "AGCU") == [0, len(texts[2]) - 4]
    for nofast in BOTH:
        assert c.members("AGCU", nofast) == [1, 2, 3]
    assert texts[1][:-1] == texts[3][:-1] and texts[1][-1] != texts[3][-1]
    off, ids = c.plain(True)
    in_1 = {v for v in range(256) if 1 in ids[off[v]:off[v + 1]]}
    assert in_1 and in_1 == {v for v in range(256) if 3 in ids[off[v]:off[v + 1]]}
    assert c.members("GGGG") == [0, 1, 3] and c.members("GGGC") == []        # (GGGC: reference 3's last window only)
    return c


# ---------------------------------------------------------------- windows that break

def _planted(k, code, name, mask0=False):
    """One unambiguous text of 3 k + 2 words, once clean and once per place p = 0 .. k with `code` at word k + p: places
    0 .. k - 1 of the window that starts at word k, and the word right behind it; then `code` as first and as last word.
    A reference keeps exactly the windows that do not cover the planted word."""
    rng = np.random.default_rng(9120 + k)
    base = text_of(rng, 3 * k + 2)
    texts = [base]
    at = [None]
    for p in list(range(k + 1)):
        texts.append(base[:k + p] + code + base[k + p + 1:])
        at.append(k + p)
    texts += [code + base[1:], base[:-1] + code]
    at += [0, len(base) - 1]
    c = Case(name, texts, k, mask0=mask0, gaps=not mask0)
    n = len(base)
    for r, (t, a) in enumerate(zip(texts, at)):
        starts = [s for s in range(n - k) if a is None or not s <= a < s + k]
        assert n_valid_windows(c.seqs[r], k) == len(starts), (name, r)
        want = sorted({value_of(base[s:s + k]) for s in starts})
        off, ids = c.plain(True)
        assert [v for v in range(1 << (2 * k)) if r in ids[off[v]:off[v + 1]]] == want, (name, r)
    assert n_valid_windows(c.seqs[0], k) == n - k
    assert n_valid_windows(c.seqs[-1], k) == n - k                   # (the last word is in no window that counts)
    assert n_valid_windows(c.seqs[1], k) == n - 2 * k
    return c


def ambiguity_at_each_place(k, kind):
    code = {"two": TWO_BIT, "three": THREE_BIT, "n": N}[kind]
    assert bin(MASK[code]).count("1") == {"two": 2, "three": 3, "n": 4}[kind]
    return _planted(k, code, "ambiguity_%s_k%d" % (kind, k))


def mask0_at_each_place(k):
    """The same with a word that has no base bit.  Outside the reference's domain (the oracle reads an arbitrary base
    from it): compared with the plain build and the device only."""
    c = _planted(k, ".", "mask0_k%d" % k, mask0=True)
    assert c.holds_mask0()
    return c


def n_runs():
    """A run of N longer than k inside a reference, at its start and at its end, and references of N only (shorter than
    k, of k and longer)."""
    rng = np.random.default_rng(9130)
    k = 6
    a, b = text_of(rng, 20), text_of(rng, 20)
    texts = [a + "N" * (k + 3) + b, "N" * (k + 1) + a, b + "N" * (k + 1), "N" * 3, "N" * k, "N" * 40, a + b]
    c = Case("n_runs", texts, k, gaps=True)
    assert [n_valid_windows(s, k) for s in c.seqs] == [(20 - k + 1) + (20 - k), 20 - k, 20 - k + 1, 0, 0, 0, 40 - k]
    assert not set(c.plain(True)[1].tolist()) & {3, 4, 5}
    return c


def lower_case():
    """12 references three times: upper case, every base lower case, single bases lower case.  The lists of the three
    groups are the same (ids shifted by 12 and 24)."""
    rng = np.random.default_rng(9140)
    g, k = 12, 4
    upper = [text_of(rng, int(n), "AGCUN" if x % 3 == 0 else "AGCU") for x, n in enumerate(rng.integers(3, 60, size=g))]
    some = [t[0].lower() + t[1] + "".join(ch.lower() if rng.random() < 0.2 else ch for ch in t[2:]) for t in upper]
    c = Case("lower_case", upper + [t.lower() for t in upper] + some, k)
    assert all(((s & LOWER) == 0).all() for s in c.seqs[:g]) and all(((s & LOWER) != 0).all() for s in c.seqs[g:2 * g])
    assert all(0 < ((s & LOWER) != 0).sum() < len(s) for s in c.seqs[2 * g:])
    for nofast in BOTH:
        off, ids = c.plain(nofast)
        for v in np.flatnonzero(np.diff(off.astype(np.int64))):
            lst = ids[off[v]:off[v + 1]]
            first = lst[lst < g]
            assert lst.tolist() == first.tolist() + (first + g).tolist() + (first + 2 * g).tolist()
    return c


# ---------------------------------------------------------------- duplicates

def kmer_three_times():
    """One k-mer three times in a reference: one posting."""
    texts = ["ACGUGACGUCACGUGG", "GGACGUGG"]
    c = Case("kmer_three_times", texts, 4, gaps=True)
    assert len(occurrences(texts[0], "ACGU")) == 3
    for nofast in BOTH:
        assert c.members("ACGU", nofast) == [0, 1]
    return c


def poly_a_300(k):
    """Poly-A of 300 bases: 300 - k equal keys of one reference, across the 256-thread stride of ref_kmer_keys and --
    sorted -- across a 256-key block of mark_unique; with a second poly-A behind it, and poly-U, the table's last list
    (no-fast)."""
    texts = ["A" * 300, "GCGC", "A" * 300, "U" * 300]
    c = Case("poly_a_300_k%d" % k, texts, k)
    assert n_valid_windows(c.seqs[0], k) == 300 - k > BLOCK and len(set(texts[0])) == 1
    nk = 1 << (2 * k)
    off, ids = c.plain(True)
    assert ids[off[0]:off[1]].tolist() == [0, 2] and ids[off[nk - 1]:off[nk]].tolist() == [3]
    off, ids = c.plain(False)
    assert ids[off[0]:off[1]].tolist() == [0, 2] and off[nk] == off[1]
    return c


def same_reference(n):
    """The same reference n times: every list is 0 .. n - 1, ascending, one posting each."""
    rng = np.random.default_rng(9150)
    t = text_of(rng, 25)
    c = Case("same_reference_%d" % n, [t] * n, 6, gaps=True)
    off, ids = c.plain(True)
    ln = np.diff(off.astype(np.int64))
    assert set(ln.tolist()) == {0, n} and (ids.reshape(-1, n) == np.arange(n)).all()
    return c


# ---------------------------------------------------------------- block boundaries

def block_lengths():
    """References of 255, 256, 257 and 513 bases (and one of 3 between them)."""
    rng = np.random.default_rng(9160)
    lens = [255, 256, 3, 257, 513]
    c = Case("block_lengths", [text_of(rng, n) for n in lens], 6)
    assert [len(s) for s in c.seqs] == lens and {BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1} <= set(lens)
    return c


def total_bases(total):
    """A store of `total` words in all: the last block of mark_unique and scatter_unique is full, holds one key, or
    lacks one."""
    rng = np.random.default_rng(9170 + total)
    lens = [100, 0, 55, total - 155]
    c = Case("total_bases_%d" % total, [text_of(rng, n) for n in lens], 4, gaps=total % 2 == 1)
    assert sum(len(s) for s in c.seqs) == total and int(c.packed()[1][-1]) == total
    return c


def one_reference():
    rng = np.random.default_rng(9180)
    c = Case("one_reference", [text_of(rng, 40)], 6)
    assert c.n_refs == 1 and set(c.plain(True)[1].tolist()) == {0}
    return c


def last_key(kind):
    """The end of the sorted keys.  Every word of a reference gives a key and the window on a reference's last word never
    counts, so a store with a base always ends, sorted, on keys without a window; in front of them stands the largest
    (k-mer, reference) pair.  "first": that pair occurs once.  "duplicate": its k-mer stands twice in its reference, so
    the last key with a window is a repeat.  "invalid": the store's last references have no window at all.  The build
    sizes the id array from the flag and the position of the last key: n_postings must come out right in all three."""
    k = 4
    top = "UUUU"
    texts = {"first": ["GCAGCAGG", "ACGCUUUUG"],
             "duplicate": ["GCAGCAGG", "UUUUGUUUUG"],
             "invalid": ["GCAGCAGG", "ACGCUUUUG", "NNNNNNNN", "GC"]}[kind]
    c = Case("last_key_%s" % kind, texts, k)
    assert c.members(top) == [1] and len(occurrences(texts[1], top)) == (2 if kind == "duplicate" else 1)
    off, ids = c.plain(True)
    assert off[-1] == len(ids) and off[-2] == len(ids) - 1 and ids[-1] == 1      # (the last posting: UUUU in reference 1)
    if kind == "invalid":
        assert n_valid_windows(c.seqs[2], k) == n_valid_windows(c.seqs[3], k) == 0
    return c


# ---------------------------------------------------------------- the table's ends, fast and no-fast, k

def table_ends(k):
    """Poly-A (list 0) and poly-U (list 4^k - 1, no-fast only), a reference that ends on poly-A and a random one; k =
    1, 2, 6, 8, 10 and 12."""
    rng = np.random.default_rng(9190 + k)
    texts = ["A" * (k + 3), "U" * (k + 3), text_of(rng, 20) + "A" * (k + 1), text_of(rng, 2 * k + 9)]
    c = Case("table_ends_k%d" % k, texts, k, gaps=k in (2, 8), dense_divs=DENSE_DIVS if k < 12 else (None,))
    nk = 1 << (2 * k)
    off, ids = c.plain(True)
    assert len(off) == nk + 1 and off[nk] == len(ids)
    assert ids[off[0]:off[1]].tolist()[:2] == [0, 2] and 1 in ids[off[nk - 1]:off[nk]]
    foff, fids = c.plain(False)
    assert foff[nk] == len(fids) < len(ids) and fids[foff[0]:foff[1]].tolist()[:2] == [0, 2]
    return c


def fast_and_nofast():
    """The fast and the no-fast index of one store of 60 references: the fast one has no list outside the first quarter of
    the table, and there the two are the same."""
    rng = np.random.default_rng(9200)
    texts = [text_of(rng, int(n), "AGCUAGCUAGCUN") for n in rng.integers(0, 120, size=60)]
    c = Case("fast_and_nofast", texts, 6, gaps=True)
    quarter_lists_equal(c)
    assert c.plain(False)[0][-1] > 100
    return c


def quarter_lists_equal(c):
    """A-first k-mers are the first quarter of the table: a fast index ends there and equals the no-fast one up to it."""
    q = 1 << (2 * (c.k - 1))
    (foff, fids), (noff, nids) = c.plain(False), c.plain(True)
    assert (foff[q:] == foff[q]).all() and foff[q] == len(fids)
    assert (foff[:q + 1] == noff[:q + 1]).all() and (fids == nids[:int(noff[q])]).all()


def no_a_first():
    """Every window that counts starts with G, C or U (A stands only inside windows, behind an N's reach, or last): the
    fast index is empty, the no-fast one is not."""
    rng = np.random.default_rng(9210)
    k = 4
    texts = [text_of(rng, 30, "GCU") for _ in range(5)]
    texts += ["GCUA" + "N" + "CCCA" + "A", "GGGAN" + "GGGGG", "A" * k, "GGGGA"]
    c = Case("no_a_first", texts, k)
    assert any("A" in t for t in texts)
    foff, fids = c.plain(False)
    assert len(fids) == 0 and (foff == 0).all() and len(c.plain(True)[1]) > 20
    return c


# ---------------------------------------------------------------- nothing to index

def nothing(kind):
    """Stores without a single window that counts: n_postings = 0, every offset 0, every score 0."""
    rng = np.random.default_rng(9220)
    k = 6
    texts = {"empty": ["", "", ""],
             "short": [text_of(rng, n) for n in (1, k - 1, k, 0, k, 2)],
             "all_n": ["N" * 40, "N" * k, "N" * (k + 1), "RYRYRYRYRY"],
             "mixed": ["", text_of(rng, k), "N" * 300, "", text_of(rng, 3), "ACGUANACGUAC"]}[kind]
    queries = [seq(text_of(rng, 50)), seq("A" * 20), seq("N" * 9), np.zeros(0, np.uint8)]
    c = Case("nothing_%s" % kind, texts, k, queries=queries, gaps=kind == "mixed")
    for nofast in BOTH:
        off, ids = c.plain(nofast)
        assert len(ids) == 0 and (off == 0).all()
        assert all(e["scores"].max() == 0 for e in c.expected(nofast))
    assert sum(n_valid_windows(s, k) for s in c.seqs) == 0
    if kind == "empty":
        assert int(c.packed()[1][-1]) == 0
    return c


# ---------------------------------------------------------------- the bitmap threshold, built on the device

def _by_members(n_refs, lists, k):
    """References that hold exactly the k-mers they are listed under: each k-mer followed by one N (the window in front
    of an N counts; no window crosses it)."""
    return [kc.query_of([value_of(km) for km, ids in lists.items() if r in ids], k) for r in range(n_refs)]


def _all_but(n_refs, out):
    return [r for r in range(n_refs) if r not in set(out)]


def threshold_300():
    """300 short references.  AGCA in exactly 256 of them (a list under every setting), AGCC in exactly 257 (a bitmap
    unless bitmaps are off), AGCG in all 300, UGCA (no-fast only) in 257.  References 31, 32, 63, 64 and 299 -- the ends
    of fill_dense's 32-bit words and of its first trip of 64 lanes -- are in one bitmap and out of the other.  A query
    holds AGCA, AGCC and AGCG once, twice and three times."""
    n, k = 300, 4
    lists = {"AGCA": _all_but(n, list(range(100, 141)) + [32, 63, 298]),
             "AGCC": _all_but(n, list(range(200, 239)) + [31, 64, 1, 298]),
             "AGCG": list(range(n)),
             "UGCA": _all_but(n, list(range(150, 189)) + [0, 32, 63, 299]),
             "ACCC": [0, 31, 299]}
    q = kc.query_of([value_of(x) for x in ("AGCA", "AGCC", "AGCC", "AGCG", "AGCG", "AGCG")], k)
    c = Case("threshold_300", _by_members(n, lists, k), k, queries=[q])
    for km, ids in lists.items():
        assert c.members(km) == ids, km
        assert km[0] != "A" or c.members(km, False) == ids
    assert [len(lists[x]) for x in ("AGCA", "AGCC", "AGCG", "UGCA")] == [256, 257, 300, 257]
    assert kc.dense_threshold(n, None) == kc.dense_threshold(n, "1000000") == 256 and kc.dense_threshold(n, "1") == 300
    edge = (31, 32, 63, 64, 299)
    assert [r in lists["AGCC"] for r in edge] == [False, True, True, False, True]
    assert [r in lists["UGCA"] for r in edge] == [True, False, False, True, False]
    assert [r in lists["AGCA"] for r in edge] == [True, False, False, True, True]
    assert [c.n_dense_lists(nf, dd) for nf in BOTH for dd in DENSE_DIVS] == [2, 0, 2, 3, 0, 3]
    s = c.expected(True)[next(i for i, m in enumerate(c.qmasks) if m.tobytes() == q.tobytes())]["scores"]
    assert set(np.unique(s).tolist()) == {3, 4, 5, 6} and s[31] == 4 and s[32] == 5 and s[298] == 3 and s[299] == 6
    return c


def threshold_330():
    """330 references (a list of 257 + 64 entries does not fit into 300): AGCA in 321 of them -- the bitmap's lanes make
    a sixth trip, for one entry -- AGCC in 257, AGCG in 256, the last reference in all three."""
    n, k = 330, 4
    lists = {"AGCA": _all_but(n, range(5, 14)), "AGCC": _all_but(n, range(64, 137)), "AGCG": _all_but(n, range(30, 104)),
             "GGGG": [0, 329]}
    c = Case("threshold_330", _by_members(n, lists, k), k)
    for km, ids in lists.items():
        assert c.members(km) == ids, km
    assert [len(lists[x]) for x in ("AGCA", "AGCC", "AGCG")] == [257 + LANES, 257, 256]
    assert -(-(257 + LANES) // LANES) == 6 and (257 + LANES) % LANES == 1
    assert kc.dense_threshold(n, None) == 256 and kc.dense_threshold(n, "1") == 330
    assert [c.n_dense_lists(nf, dd) for nf in BOTH for dd in DENSE_DIVS] == [2, 0, 2, 2, 0, 2]
    return c


# ---------------------------------------------------------------- the matrix

K_SET = (1, 2, 6, 8, 10)
CASES = {}
for _k in K_SET:
    CASES["lengths_around_k_%d" % _k] = functools.partial(lengths_around_k, _k)
CASES.update({"empty_references": empty_references, "last_window": last_window})
for _k in (1, 4, 6):
    for _kind in ("two", "three", "n"):
        CASES["ambiguity_%s_k%d" % (_kind, _k)] = functools.partial(ambiguity_at_each_place, _k, _kind)
    CASES["mask0_k%d" % _k] = functools.partial(mask0_at_each_place, _k)
CASES.update({"n_runs": n_runs, "lower_case": lower_case, "kmer_three_times": kmer_three_times})
CASES.update({"poly_a_300_k%d" % _k: functools.partial(poly_a_300, _k) for _k in (1, 6)})
CASES.update({"same_reference_%d" % _n: functools.partial(same_reference, _n) for _n in (2, 130)})
CASES.update({"block_lengths": block_lengths, "one_reference": one_reference})
CASES.update({"total_bases_%d" % _n: functools.partial(total_bases, _n) for _n in (255, 256, 257, 512, 513)})
CASES.update({"last_key_%s" % _x: functools.partial(last_key, _x) for _x in ("first", "duplicate", "invalid")})
CASES.update({"table_ends_k%d" % _k: functools.partial(table_ends, _k) for _k in K_SET + (12,)})
CASES.update({"fast_and_nofast": fast_and_nofast, "no_a_first": no_a_first})
CASES.update({"nothing_%s" % _x: functools.partial(nothing, _x) for _x in ("empty", "short", "all_n", "mixed")})
CASES.update({"threshold_300": threshold_300, "threshold_330": threshold_330})
MASK0_CASES = ("mask0_k1", "mask0_k4", "mask0_k6")


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    assert c.name == name
    return c


# ---------------------------------------------------------------- fuzz

@functools.lru_cache(maxsize=None)
def fuzz_world(seed):
    """A seeded store (the ORDER of the draws is part of it: a seed names a case): 1 to 400 references of 0 to 300
    words, single bases with 0 to 30 % ambiguity codes, lower-case bits, k from 1, 2, 4, 6, 8, both nofast settings, one
    dense_div."""
    rng = np.random.default_rng(9300 + seed)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    n_refs = int(pick([1, 2, 7, 60, 257, 300, 400, 400]))
    k = int(pick([1, 2, 4, 6, 8]))
    dd = pick([None, "1", "8", "1000000"])
    amb, low = float(pick([0.0, 0.02, 0.3])), float(pick([0.0, 0.1, 1.0]))
    max_len = int(pick([k + 2, 40, 300]))
    codes = np.array([3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 15, 15], np.uint8)
    alphabet = np.array(pick([[1, 2, 4, 8], [1, 1, 1, 2, 4, 8], [1, 8]]), np.uint8)       # (few letters: long lists at small k)
    seqs = []
    for _ in range(n_refs):
        n = int(rng.integers(0, max_len + 1))
        m = alphabet[rng.integers(0, len(alphabet), size=n)]
        a = rng.random(n) < amb
        m = np.where(a, codes[rng.integers(0, len(codes), size=n)], m)
        m = m | np.where(rng.random(n) < low, LOWER, 0).astype(np.uint8)
        seqs.append(m.astype(np.uint8))
    c = Case("fuzz_%d" % seed, seqs, k, gaps=bool(rng.integers(0, 2)), dense_divs=(dd,))
    assert not c.holds_mask0()
    return c
