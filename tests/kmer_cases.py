"""The inputs of the k-mer kernel tests, shared by tests/test_kmer_cpu.py (which pins tests/kmer_ref.py to the oracle and
asserts that every case reaches the edge it is there for) and tests/test_gpu_kmer.py (which runs them through
sina_hip_upload_index / sina_hip_kmer_scores / sina_hip_kmer_topk).  No biology here: sina_hip_upload_index adopts any
CSR index and a query is mask bytes, so a case writes down exact posting lists and exact queries and the score row is
its own.  A query whose windows are the distinct k-mers k_0 .. k_m-1 (each followed by one N: query_of) gives reference
r the score |{j : r in list(k_j)}|; to give r the score s, put r into the first s lists (index_for_scores).

A case: n_refs (the store is n_refs one-base dummies: only the count matters to these kernels), k, nofast, the CSR, the
query masks of one batch, the `max` values, and the SINA_HIP_TEST knobs to run it under.  Every CSR goes through
check_csr -- the contract the kernels rely on; an index outside it can send an LDS atomic out of bounds, so no case is
built to see what the kernels do with bad input.  Each builder asserts the edge it exists for; where the edge is a branch
of a kernel, a small restatement of that branch's arithmetic (dense_threshold, n_dense_windows, shortcut_model,
cand_model) says whether the case reaches it.  Those decide reachability only: every expected result comes from
kmer_ref.  Everything here is CPU work."""
import functools

import numpy as np

from sina_amd import capi
from tests import kmer_ref

TILE = 32768                      # references per tile of the count kernels
THREAD_REFS = 32                  # references per thread of a tile (candidate path, bit-sliced path)
MAX_DENSE_Q = 1023                # dense windows of one query (or chunk) counted bit-sliced; the rest by cursor
SEL_MAX = 4096                    # candidates the select kernels sort
CAND_MAX_M = 128                  # largest `max` of the candidate-list path
FAST_MAX = capi.MAX_QUERY_LEN
LONG_MAX = capi.MAX_LONG_QUERY_LEN
N_MASK = 15
BASE_MASK = {"A": 1, "G": 2, "C": 4, "T": 8}
DENSE_DIVS = (None, "1", "1000000")
EDGE_N_REFS = (1, 2, 9, 32767, 32768, 32769, 65535, 65536, 65537)
DENSE_ND = (1, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023)
PLANT_IDS = (0, 1, 2, 3, 31, 32, 32767, 32768, 65535, 65536, 69999)


# ---------------------------------------------------------------- helpers

def kmer_mask(v, k):
    return np.array([1 << ((v >> (2 * (k - 1 - i))) & 3) for i in range(k)], np.uint8)


def query_of(kmers, k):
    """Each k-mer followed by one N: exactly these windows, in this order, and no others."""
    if len(kmers) == 0:
        return np.zeros(0, np.uint8)
    return np.concatenate([np.append(kmer_mask(int(v), k), np.uint8(N_MASK)) for v in kmers])


def poly(base, n):
    """n times one base: as a whole query the k-mer of k such bases with multiplicity n - k (the window on the last base
    is never produced); in front of an N, n - k + 1."""
    return np.full(n, BASE_MASK[base], np.uint8)


def pad_n(mask, length):
    """Trailing Ns up to `length`: raises len - k (the select kernel's bound on the scores) without adding windows."""
    assert len(mask) <= length
    return np.concatenate([np.asarray(mask, np.uint8), np.full(length - len(mask), N_MASK, np.uint8)])


def poly_kmer(base, k):
    code = {"A": 0, "G": 1, "C": 2, "T": 3}[base]
    v = 0
    for _ in range(k):
        v = (v << 2) | code
    return v


def index_for_scores(score_row, kmers):
    """Posting lists that give reference r the score score_row[r] against query_of(kmers): r is in the first
    score_row[r] lists."""
    row = np.asarray(score_row, np.int64)
    assert row.min() >= 0 and row.max() <= len(kmers)
    return {int(kmers[j]): np.flatnonzero(row > j).astype(np.uint32) for j in range(int(row.max()))}


def build_csr(lists, k):
    nk = 1 << (2 * k)
    ln = np.zeros(nk, np.int64)
    for v, ids in lists.items():
        ln[v] = len(ids)
    off = np.zeros(nk + 1, np.uint32)
    off[1:] = np.cumsum(ln)
    parts = [np.asarray(lists[v], np.uint32) for v in sorted(lists) if len(lists[v])]
    return off, (np.concatenate(parts) if parts else np.zeros(0, np.uint32))


class Case:
    def __init__(self, name, n_refs, k, nofast, lists, qmasks, maxes, dense_divs=DENSE_DIVS, kmer_rows=(None,),
                 long_api=False, labels=None):
        self.name, self.n_refs, self.k, self.nofast = name, int(n_refs), k, bool(nofast)
        self.off, self.ids = build_csr(lists, k)
        self.qmasks = [np.ascontiguousarray(m, np.uint8) for m in qmasks]
        self.maxes = tuple(int(m) for m in maxes)
        self.dense_divs, self.kmer_rows, self.long_api = tuple(dense_divs), tuple(kmer_rows), long_api
        self.labels = list(labels) if labels else ["q%d" % i for i in range(len(self.qmasks))]
        check_csr(self)

    @property
    def qmask(self):
        return np.concatenate(self.qmasks) if self.qmasks else np.zeros(0, np.uint8)

    @property
    def qoff(self):
        off = np.zeros(len(self.qmasks) + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in self.qmasks])
        return off

    def ref_store(self):
        """(packed bases, offsets, width) of n_refs one-base references."""
        return np.full(self.n_refs, 1 << 24, np.uint32), np.arange(self.n_refs + 1, dtype=np.uint64), 8

    def list_lengths(self):
        return np.diff(self.off.astype(np.int64))

    @functools.cached_property
    def expected(self):
        """Per query the score vector, and per max its (ids, scores): kmer_ref's, computed once."""
        out = []
        for m in self.qmasks:
            s = kmer_ref.scores(self.off, self.ids, self.n_refs, m, self.k, not self.nofast)
            out.append(dict(scores=s, find={mx: kmer_ref.topk(s, mx) for mx in self.maxes}))
        return out


def check_csr(case):
    """The contract the kernels rely on (include/sina_hip.h, sina_hip_upload_index)."""
    off, ids = case.off.astype(np.int64), case.ids.astype(np.int64)
    assert len(off) == (1 << (2 * case.k)) + 1 and off[0] == 0 and off[-1] == len(ids), case.name
    assert (np.diff(off) >= 0).all(), case.name
    assert len(ids) == 0 or (ids.min() >= 0 and ids.max() < case.n_refs), case.name
    if len(ids) > 1:
        inner = np.ones(len(ids) - 1, bool)            # pairs (x, x + 1) inside one list
        starts = off[1:-1]
        inner[starts[(starts > 0) & (starts < len(ids))] - 1] = False
        assert (np.diff(ids)[inner] > 0).all(), case.name
    for m, e in zip(case.qmasks, case.expected):
        assert len(m) <= (LONG_MAX if case.long_api else FAST_MAX), case.name
        top = int(e["scores"].max()) if case.n_refs else 0
        assert top <= max(0, len(m) - case.k) and top <= 32767, case.name


# ---------------------------------------------------------------- restatements of the kernels' branch arithmetic
# (reachability only: no expected result comes from these)

def dense_threshold(n_refs, dense_div):
    """kmer_dense_threshold (csrc/kmer_plan.h): a list LONGER than this is also kept as a bitmap."""
    return max(256, n_refs // (64 if dense_div is None else max(1, int(dense_div))))


def n_dense_lists(case, dense_div):
    return int((case.list_lengths() > dense_threshold(case.n_refs, dense_div)).sum())


def n_dense_windows(case, qi, dense_div):
    """How many windows of query qi (with multiplicity) have a dense list: the kernel counts min(this, 1023) of them
    bit-sliced -- `nd` -- and the rest by cursor."""
    w = kmer_ref.window_values(case.qmasks[qi], case.k, not case.nofast)
    return int((case.list_lengths()[w] > dense_threshold(case.n_refs, dense_div)).sum())


def nhi_of(nd):
    """The dense_path<NHI> variant a query of nd dense windows runs."""
    nd = min(nd, MAX_DENSE_Q)
    return max(0, nd.bit_length() - 3) if nd else None


def shortcut_model(row, mx, qlen, k):
    """kmer_select_kernel's sampled short cut on one score row: None where it is not tried (fewer than 2048 vectors of 8
    scores, or a query of 8192 windows and more); else T0 (-1: the sample holds too few positive scores), usable,
    n_ge_t0 = count(>= T0) over the whole row, and the exit taken: "unusable", "found" (at least M scores reach T0; with
    n_ge_cut, take_all) or "fewer"."""
    row = np.asarray(row, np.int64)
    n = len(row)
    nvec, M = (n + 7) // 8, min(mx, n)
    top = min(max(0, qlen - k), FAST_MAX)
    if nvec < 2048 or top >= 2 * SEL_MAX:
        return None
    s = row[(np.arange(n) // 8) % 16 == 0]
    hist = np.bincount(np.minimum(s[s > 0], top), minlength=top + 1)
    suffix = np.cumsum(hist[::-1])[::-1]
    target = 2 * M // 16 + 8
    at = np.flatnonzero(suffix >= target)
    T0 = int(at.max()) if len(at) else -1
    usable = T0 >= 1 and int(suffix[T0]) <= 8 * target
    out = dict(T0=T0, usable=usable, exit="unusable")
    if usable:
        out["n_ge_t0"] = n_ge = int((row >= T0).sum())
        if n_ge >= M:
            cut = int(np.sort(row)[::-1][M - 1])
            out.update(exit="found", cut=cut, n_ge_cut=int((row >= cut).sum()))
            out["take_all"] = out["n_ge_cut"] <= SEL_MAX
        else:
            out["exit"] = "fewer"
    return out


def cand_model(row, mx):
    """kmer_count_kernel<true>: t0 = the mx-th largest of the 1024 per-thread maxima of tile 0 (each over 32
    references), n_cand = how many references of the whole row reach it; more than 4096 overflow the list."""
    row = np.asarray(row, np.int64)
    assert len(row) >= 2 * TILE and mx <= CAND_MAX_M
    maxima = row[:TILE].reshape(TILE // THREAD_REFS, THREAD_REFS).max(axis=1)
    t0 = int(np.sort(maxima)[::-1][mx - 1])
    n_cand = int((row >= t0).sum())
    return dict(t0=t0, n_cand=n_cand, overflow=n_cand > SEL_MAX)


def takes_cand_path(case, mx, rows):
    return mx <= CAND_MAX_M and case.n_refs >= 2 * TILE and not rows and not case.long_api


def expected_launches(case, mx, rows):
    """By how much stats()["kmer_launches"] advances for one kmer_topk of the case's batch: one launch range, repeated
    with the score rows when a candidate list of the range overflowed."""
    if not takes_cand_path(case, mx, rows):
        return 1
    return 2 if any(cand_model(e["scores"], mx)["overflow"] for e in case.expected) else 1


# ---------------------------------------------------------------- count cases

def _bernoulli_lists(rng, n_refs, dens, force):
    """One random membership row per density; force = {id: bool per list} overrides columns.  Ascending id arrays."""
    out = []
    for lo in range(0, len(dens), 64):
        d = np.asarray(dens[lo:lo + 64], np.float32)
        m = rng.random((len(d), n_refs), dtype=np.float32) < d[:, None]
        for r, member in force.items():
            m[:, r] = member[lo:lo + 64]
        out += [np.flatnonzero(x).astype(np.uint32) for x in m]
    return out


DENSE_K = 6
DENSE_N = 70000
CURSOR_KMERS = tuple(range(3000, 3005))


@functools.lru_cache(maxsize=None)
def dense_world():
    """70 000 references (three tiles, the last one partial), k = 6, no-fast.  K-mers 0 .. 1022 (set A) and 1024 ..
    2046 (set B) have lists longer than the dense threshold 1093 with random membership of mixed density; five short
    cursor lists hit the same planted references.  Planted, by the number s of set A's FIRST lists a reference is in
    (so the query of A's first n k-mers gives it min(s, n)): s = 1023 ("in all") at PLANT_IDS, s = 0 at none_ids, and
    s = 2^p - 1, 2^p for every p in each tile.  In set B the PLANT_IDS are in the first list only ("in exactly one")."""
    rng = np.random.default_rng(8101)
    n = DENSE_N
    planted = {r: MAX_DENSE_Q for r in PLANT_IDS}
    none_ids = (4, 33, 32766, 32769, 65534, 69998)
    planted.update({r: 0 for r in none_ids})
    for base in (100, TILE + 100, 2 * TILE + 100):
        for p in range(10):
            planted[base + 2 * p] = (1 << p) - 1
            planted[base + 2 * p + 1] = 1 << p
    j = np.arange(MAX_DENSE_Q)
    dens_a = rng.choice([0.018, 0.02, 0.05, 0.5], p=[0.7, 0.25, 0.04, 0.01], size=MAX_DENSE_Q)
    lists_a = _bernoulli_lists(rng, n, dens_a, {r: j < s for r, s in planted.items()})
    force_b = {r: j < 0 for r in planted}
    force_b.update({r: j < 1 for r in PLANT_IDS})
    lists_b = _bernoulli_lists(rng, n, np.full(MAX_DENSE_Q, 0.018), force_b)
    lists = {v: lists_a[v] for v in range(MAX_DENSE_Q)}
    lists.update({1024 + v: lists_b[v] for v in range(MAX_DENSE_Q)})
    some = np.array(sorted(planted), np.uint32)
    for x, v in enumerate(CURSOR_KMERS):
        extra = rng.choice(n, size=120 + 40 * x, replace=False).astype(np.uint32)
        lists[v] = np.unique(np.concatenate([some[x % 2::2] if x else some, extra]))
    return lists, planted


def set_a(n):
    return list(range(n))


def set_b(n):
    return list(range(1024, 1024 + n))


@functools.lru_cache(maxsize=None)
def dense_nd():
    """Two queries per n of DENSE_ND, "dense_nd_<n>" over set A's first n k-mers and "dense_nd_<n>_one" over set B's,
    each with the five cursor k-mers behind them.  Default threshold only (the lists are dense by construction; under
    1000000 the cursor lists would turn dense and move nd), and "1" for equality."""
    lists, planted = dense_world()
    qs, labels = [], []
    for n in DENSE_ND:
        qs += [query_of(set_a(n) + list(CURSOR_KMERS), DENSE_K), query_of(set_b(n) + list(CURSOR_KMERS), DENSE_K)]
        labels += ["dense_nd_%d" % n, "dense_nd_%d_one" % n]
    c = Case("dense_nd", DENSE_N, DENSE_K, True, lists, qs, (41, 410), dense_divs=(None, "1"), labels=labels)
    ln = c.list_lengths()
    thr = dense_threshold(DENSE_N, None)
    assert thr == 1093 and (ln[:MAX_DENSE_Q] > thr).all() and (ln[1024:1024 + MAX_DENSE_Q] > thr).all()
    assert (ln[list(CURSOR_KMERS)] <= thr).all() and (ln[list(CURSOR_KMERS)] > 0).all()
    assert n_dense_lists(c, None) == 2 * MAX_DENSE_Q and n_dense_lists(c, "1") == 0
    assert ln[:MAX_DENSE_Q].max() > 20000 and ln[:MAX_DENSE_Q].min() < 1400          # mixed density
    cur = sum(np.bincount(lists[v], minlength=DENSE_N) for v in CURSOR_KMERS)
    for x, n in enumerate(DENSE_ND):
        assert n_dense_windows(c, 2 * x, None) == n_dense_windows(c, 2 * x + 1, None) == n
        sa, sb = c.expected[2 * x]["scores"] - cur, c.expected[2 * x + 1]["scores"] - cur
        for r, s in planted.items():
            assert sa[r] == min(s, n), (n, r)
        assert all(sa[r] == n and sb[r] == 1 for r in PLANT_IDS)     # every plane set / one bit, at the edges of tiles
        assert sa.max() == n and (cur[list(PLANT_IDS)] > 0).any()
    return c


@functools.lru_cache(maxsize=None)
def dense_overflow():
    """1024 and 1100 dense windows: the 1023 first to arrive are counted bit-sliced, the tail by cursors over long
    lists, in the LDS array the bitmap numbers grow down into.  27 of the 1100 repeat the dense k-mer AAAAAA."""
    lists, _ = dense_world()
    q1 = query_of(set_a(MAX_DENSE_Q) + set_b(1), DENSE_K)
    q2 = np.concatenate([query_of(set_a(MAX_DENSE_Q) + set_b(50), DENSE_K), poly("A", DENSE_K + 26), [N_MASK]])    # (behind an N: n - k + 1 windows)
    c = Case("dense_overflow", DENSE_N, DENSE_K, True, lists, [q1, q2], (41, 410))
    assert poly_kmer("A", DENSE_K) == 0
    for dd, want in ((None, [1024, 1100]), ("1", [0, 0]), ("1000000", [1024, 1100])):
        assert [n_dense_windows(c, i, dd) for i in range(2)] == want
    assert c.expected[1]["scores"][0] == MAX_DENSE_Q + 1 + 27    # (reference 0: all of set A, the first list of set B, AAAAAA 27 times more)
    return c


@functools.lru_cache(maxsize=None)
def multiplicity():
    """A dense k-mer 300 times in a row and a cursor k-mer 300 times, in one query."""
    rng = np.random.default_rng(8102)
    n, k = DENSE_N, 6
    a, cc_ = poly_kmer("A", k), poly_kmer("C", k)
    lists = {a: np.unique(np.concatenate([rng.choice(n, 5000, replace=False), PLANT_IDS])).astype(np.uint32),
             cc_: np.unique(np.concatenate([rng.choice(n, 190, replace=False), PLANT_IDS])).astype(np.uint32),
             77: np.sort(rng.choice(n, 900, replace=False)).astype(np.uint32)}
    q = np.concatenate([poly("A", k + 299), [N_MASK], poly("C", k + 299), [N_MASK], query_of([77], k)])
    c = Case("multiplicity", n, k, True, lists, [q], (1, 41, 410))
    for dd, want in ((None, 300), ("1", 0), ("1000000", 301)):
        assert n_dense_windows(c, 0, dd) == want
    s = c.expected[0]["scores"]
    assert s.max() >= 600 and set(np.unique(s)) >= {0, 300, 600}
    return c


CURSOR_PREFIXES = (0, 1, 63, 64, 65, 64 + 511, 64 + 512, 64 + 513, 64 + 1024 + 3)
CURSOR_TAILS = ((0, 0), (1, 1), (5, 5), (0, 1), (5, 0))


def _cursor_lists(rng, n_refs):
    """Lists by the number of their postings inside tile 0 (the 64-posting probe exits below 64, the 512-posting loop
    below 512, a scalar tail reads the last one to three) and, where there are further tiles, by their continuation
    there.  Returns (lists, {k-mer: (prefix, in tile 1, in tile 2)})."""
    pool0 = np.unique(np.concatenate([rng.choice(min(n_refs, TILE), 2400, replace=False), [0, min(n_refs, TILE) - 1]]))
    tails = CURSOR_TAILS if n_refs > 2 * TILE else ((0, 0),)
    lists, shape, v = {}, {}, 1
    for p in CURSOR_PREFIXES:
        for c1, c2 in tails:
            ids = [rng.choice(pool0, p, replace=False)]
            if c1:
                ids.append(TILE + rng.choice(600, c1, replace=False))
            if c2:
                ids.append(2 * TILE + rng.choice(n_refs - 2 * TILE, c2, replace=False))
            ids = np.unique(np.concatenate(ids)).astype(np.uint32)
            if len(ids):
                lists[v] = ids
            shape[v] = (p, c1, c2)
            v += 1
    return lists, shape, v


@functools.lru_cache(maxsize=None)
def cursor_lengths():
    """c.meant_for says per k-mer under which dense_div settings its list is read by cursor, which is what the list is
    there for: up to 256 postings under every setting; up to 1093 under the default and under "1"; 1094 and more only
    under "1" (bitmaps off).  The results are the same bytes under all three."""
    rng = np.random.default_rng(8103)
    n = DENSE_N
    lists, shape, v = _cursor_lists(rng, n)
    lists[v] = np.array([5, 32767, 32768, 40000], np.uint32)                     # the tile boundary inside one list
    lists[v + 1] = (2 * TILE + np.sort(rng.choice(n - 2 * TILE, 65, replace=False))).astype(np.uint32)   # wholly in tile 2
    kmers = sorted(shape) + [v, v + 1]
    c = Case("cursor_lengths", n, 6, True, lists, [query_of(kmers, 6)], (1, 41, 410))
    ln = c.list_lengths()
    for km, (p, c1, c2) in shape.items():
        ids = lists.get(km, np.zeros(0, np.uint32))
        assert (ids < TILE).sum() == p and ((ids >= TILE) & (ids < 2 * TILE)).sum() == c1 and (ids >= 2 * TILE).sum() == c2
    assert {p for p, _, _ in shape.values()} == set(CURSOR_PREFIXES)
    assert sum(1 for x in ln[ln > 0] if x % 4) >= 10 and {int(x) % 4 for x in ln[ln > 0]} == {0, 1, 2, 3}
    assert ln.max() > dense_threshold(n, None) and n_dense_lists(c, "1") == 0
    assert lists[v + 1].min() >= 2 * TILE
    c.meant_for = {km: tuple(dd for dd in DENSE_DIVS if 0 < ln[km] <= dense_threshold(n, dd)) for km in kmers}
    for km, (p, c1, c2) in shape.items():
        want = () if p + c1 + c2 == 0 else DENSE_DIVS if p + c1 + c2 <= 256 else (None, "1") if p + c1 + c2 <= 1093 else ("1",)
        assert c.meant_for[km] == want, km
    assert {c.meant_for[km] for km in shape} == {(), DENSE_DIVS, (None, "1"), ("1",)}
    return c


@functools.lru_cache(maxsize=None)
def cursor_one_tile():
    """The same prefix lengths with all references in one tile: 32 768 references, nothing behind the prefix."""
    rng = np.random.default_rng(8104)
    lists, shape, v = _cursor_lists(rng, TILE)
    c = Case("cursor_one_tile", TILE, 6, True, lists, [query_of(sorted(shape), 6)], (1, 41, 410))
    assert sorted(int(x) for x in c.list_lengths() if x) == sorted(p for p in CURSOR_PREFIXES if p)
    return c


def _random_lists(rng, n_refs, kmers, max_len):
    lists = {}
    for v in kmers:
        ln = int(rng.integers(1, max(2, min(n_refs, max_len) + 1)))
        lists[int(v)] = np.flatnonzero(rng.random(n_refs) < ln / n_refs).astype(np.uint32)
    return lists


@functools.lru_cache(maxsize=None)
def tile_geometry(n_refs):
    """A small random index at a reference count on either side of a tile end (odd counts: the row's last 32-bit word
    holds one score).  Query 0: the LAST reference alone carries the best score.  Query 1: it ties at the cut of max =
    41 (where there are that many references) and, having the largest id, is the first tie taken."""
    rng = np.random.default_rng(8200 + n_refs % 1000)
    k = 6
    s0 = list(range(100, 120))
    lists = _random_lists(rng, n_refs, s0, 600)
    for v in s0:
        lists[v] = np.unique(np.append(lists[v], n_refs - 1)).astype(np.uint32)
    row = np.zeros(n_refs, np.int64)
    if n_refs > 200:
        free = rng.permutation(n_refs - 1)
        row[free[:10]] = 3
        row[free[10:109]] = 2
        row[free[109:400]] = 1
        row[n_refs - 1] = 2
    else:
        row[:] = rng.integers(0, 3, size=n_refs)
    s1 = list(range(200, 203))
    lists.update(index_for_scores(row, s1))
    c = Case("tile_geometry_%d" % n_refs, n_refs, k, True, lists, [query_of(s0, k), query_of(s1, k)], (1, 41, 128, 129))
    e0, e1 = c.expected
    assert e0["find"][1][0][0] == n_refs - 1 and (n_refs == 1 or e0["scores"][:-1].max() < e0["scores"][-1] == 20)
    assert (e1["scores"] == row).all()
    if n_refs > 200:
        ids, sc = e1["find"][41]
        assert ids[10] == n_refs - 1 and sc[10] == 2 and sc[40] == 2 and (row == 2).sum() > 31
    return c


@functools.lru_cache(maxsize=None)
def fast_ignores_non_a():
    """A fast index (nofast = 0) that all the same holds lists for k-mers that do not start with A: the kernels must
    not count the query's windows on them."""
    rng = np.random.default_rng(8105)
    n, k = 5000, 6
    a_kmers = [int(x) for x in rng.choice(1 << (2 * (k - 1)), 12, replace=False)]
    other = [int(x) for x in (1 << (2 * (k - 1))) + rng.choice(3 << (2 * (k - 1)), 12, replace=False)]
    lists = _random_lists(rng, n, a_kmers + other, 800)
    mixed = [x for pair in zip(a_kmers, other) for x in pair]
    c = Case("fast_ignores_non_a", n, k, False, lists, [query_of(mixed, k), query_of(other, k)], (1, 41, 410))
    slow = kmer_ref.scores(c.off, c.ids, n, c.qmasks[0], k, False)
    assert (slow != c.expected[0]["scores"]).any() and c.expected[1]["scores"].max() == 0
    return c


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Lengths 0, k, k + 1 and 7 (no window, no window, one, one), a query of the fast kernel's longest length with
    1000 dense windows, and a short one behind it.  (Under "1000000" two of the short query's cursor lists are bitmaps
    too.)  A query without windows scores zero everywhere, so on the candidate path its t0 is 0, its list overflows and
    the whole batch is redone with score rows: max = 1 and 41 check that fallback here, and mixed_batch_cand the same
    long and short queries where the candidate lists hold."""
    lists, _ = dense_world()
    k = DENSE_K
    qs = [np.zeros(0, np.uint8), kmer_mask(0, k), np.append(kmer_mask(3000, k), np.uint8(N_MASK)), poly("A", 7),
          pad_n(query_of(set_a(1000), k), FAST_MAX), query_of(set_a(3) + list(CURSOR_KMERS), k)]
    c = Case("mixed_batch", DENSE_N, k, True, lists, qs, (1, 41, 410))
    assert [len(m) for m in qs[:4]] == [0, k, k + 1, 7] and len(qs[4]) == FAST_MAX
    assert [len(kmer_ref.window_values(m, k, False)) for m in qs] == [0, 0, 1, 1, 1000, 8]
    assert [n_dense_windows(c, 4, dd) for dd in DENSE_DIVS] == [1000, 0, 1000]
    assert n_dense_windows(c, 5, None) == 3 < n_dense_windows(c, 5, "1000000") < 8
    assert all(expected_launches(c, mx, None) == 2 for mx in (1, 41)) and expected_launches(c, 410, None) == 1
    return c


@functools.lru_cache(maxsize=None)
def mixed_batch_cand():
    """The long and the short query of mixed_batch (and the short one again in front) in a batch of their own: no
    candidate list overflows, so max = 1 and 41 are answered by kmer_count_kernel<true> with queries of 10 240 and of
    56 bases side by side; each also with the score rows forced."""
    lists, _ = dense_world()
    k = DENSE_K
    short = query_of(set_a(3) + list(CURSOR_KMERS), k)
    qs = [short, pad_n(query_of(set_a(1000), k), FAST_MAX), short]
    c = Case("mixed_batch_cand", DENSE_N, k, True, lists, qs, (1, 41, 410), kmer_rows=(None, 1))
    assert [len(m) for m in qs] == [8 * (k + 1), FAST_MAX, 8 * (k + 1)]
    for mx in (1, 41):
        assert takes_cand_path(c, mx, None) and expected_launches(c, mx, None) == 1
        assert all(cand_model(e["scores"], mx)["t0"] >= 1 for e in c.expected)
    return c


# ---------------------------------------------------------------- select cases (score rows)

def _score_case(name, n_refs, rows, maxes, k=6, pad=None, extra_lists=None, extra_queries=(), **kw):
    """One query per score row, each over k-mers of its own."""
    lists, qs, base = dict(extra_lists or {}), [], 16
    for row in rows:
        top = int(np.max(row)) if len(row) else 0
        kmers = list(range(base, base + top))
        base += top + 1
        lists.update(index_for_scores(row, kmers))
        q = query_of(kmers, k) if top else np.full(k + 3, N_MASK, np.uint8)
        qs.append(pad_n(q, pad) if pad else q)
    c = Case(name, n_refs, k, True, lists, qs + list(extra_queries), maxes, dense_divs=(None,), **kw)
    for row, e in zip(rows, c.expected):
        assert (e["scores"] == row).all(), name
    return c


def _row(rng, n_refs, counts):
    """A row with counts[s] references of score s (s >= 1) at random places, zeros elsewhere."""
    row = np.zeros(n_refs, np.int64)
    at = rng.permutation(n_refs)
    lo = 0
    for s, c in counts.items():
        row[at[lo:lo + c]] = s
        lo += c
    assert lo <= n_refs
    return row


def _spread_row(rng, n_refs, top=9):
    row = np.minimum(rng.geometric(0.45, size=n_refs) - 1, top).astype(np.int64)
    row[n_refs - 1] = top
    return row


def _models(c, qi, mx):
    return shortcut_model(c.expected[qi]["scores"], mx, len(c.qmasks[qi]), c.k)


@functools.lru_cache(maxsize=None)
def row_tail(n_refs):
    """16376: 2047 vectors, the short cut is off; 16377: 2048, on, with one score in the last vector; 16384: on, the
    last vector full.  The last reference carries the top score."""
    rng = np.random.default_rng(8300 + n_refs % 100)
    c = _score_case("row_tail_%d" % n_refs, n_refs, [_spread_row(rng, n_refs), _row(rng, n_refs, {3: 5, 2: 700, 1: 3000})],
                    (1, 41, 410, 4096))
    assert (_models(c, 0, 410) is None) == (n_refs == 16376)
    assert c.expected[0]["find"][1][0][0] == n_refs - 1
    return c


@functools.lru_cache(maxsize=None)
def zeros_fill(n_refs):
    """17 positive scores, max = 410 and 4096: the zeros with the largest ids fill the result.  At 20 000 references
    the short cut runs and its sample finds too few positives to place a threshold."""
    rng = np.random.default_rng(8310 + n_refs % 100)
    c = _score_case("zeros_fill_%d" % n_refs, n_refs, [_row(rng, n_refs, {5: 3, 2: 6, 1: 8})], (410, 4096))
    for mx in c.maxes:
        m = _models(c, 0, mx)
        assert (m is None) if n_refs == 5000 else (m["T0"] == -1 and not m["usable"])
        ids, sc = c.expected[0]["find"][mx]
        assert len(ids) == mx and (sc > 0).sum() == 17 and ids[17] == max(set(range(n_refs)) - set(ids[:17].tolist()))
    return c


def _place(row, ids, score):
    assert (row[ids] == 0).all()
    row[ids] = score


def _vector_ids(rng, n_refs, sampled, count, exclude=()):
    """`count` ids of vectors the short cut samples ((id // 8) % 16 == 0), or of vectors it does not."""
    ids = np.arange(n_refs)
    ok = ((ids // 8) % 16 == 0) == sampled
    ok[list(exclude)] = False
    return rng.choice(ids[ok], count, replace=False)


@functools.lru_cache(maxsize=None)
def sample_high():
    """The short cut's third exit: the sample overestimates the row.  64 references with the top score 9, all of them
    in sampled vectors, so T0 = 9, usable, and only 64 < M = 410 scores reach it: the search goes on below T0 with the
    64 as the count above.  Query 0: the cut (4) falls strictly between.  Query 1: the cut (8) is T0 - 1 and fewer than
    M references tie there -- the count carried out of the short cut is then the one the tie split uses."""
    rng = np.random.default_rng(8320)
    n = 20000
    rows = []
    for counts in ({8: 50, 7: 60, 6: 80, 5: 100, 4: 150, 3: 300, 2: 300, 1: 300},
                   {8: 400, 7: 100, 6: 100, 5: 100, 4: 100, 3: 100, 2: 100, 1: 100}):
        tops = _vector_ids(rng, n, True, 64)
        rest = np.setdiff1d(np.arange(n), tops)
        row = np.zeros(n, np.int64)
        row[rest] = _row(rng, len(rest), counts)
        _place(row, tops, 9)
        rows.append(row)
    c = _score_case("sample_high", n, rows, (410,))
    for qi, cut in ((0, 4), (1, 8)):
        m = _models(c, qi, 410)
        assert m["T0"] == 9 and m["usable"] and m["n_ge_t0"] == 64 < 410 and m["exit"] == "fewer"
        sc = c.expected[qi]["find"][410][1]
        assert sc[-1] == cut and 1 < cut < 9
    assert 410 - 64 <= (rows[1] == 8).sum() < 410
    return c


@functools.lru_cache(maxsize=None)
def sample_blind():
    """The mirror image: everything that matters sits in vectors the short cut does not sample.  Query 0: the sampled
    vectors hold zeros only (no threshold).  Query 1: they hold a hundred ones, so T0 = 1, far below the cut."""
    rng = np.random.default_rng(8330)
    n = 20000
    rows = []
    for ones in (0, 100):
        row = np.zeros(n, np.int64)
        hi = _vector_ids(rng, n, False, 1500)
        row[hi] = rng.integers(2, 10, size=len(hi))
        if ones:
            _place(row, _vector_ids(rng, n, True, ones), 1)
        rows.append(row)
    c = _score_case("sample_blind", n, rows, (41, 410))
    m0, m1 = _models(c, 0, 410), _models(c, 1, 410)
    assert m0["T0"] == -1 and m0["exit"] == "unusable"
    assert m1["T0"] == 1 and m1["exit"] == "found" and m1["cut"] > 1 and m1["take_all"]
    return c


@functools.lru_cache(maxsize=None)
def giant_group():
    """One score for all but a few references: the sample's threshold group is too large, the short cut refuses."""
    rng = np.random.default_rng(8340)
    n = 20000
    row = np.full(n, 5, np.int64)
    at = rng.permutation(n)
    row[at[:7]] = 7
    row[at[7:20]] = 0
    row[at[20:40]] = 4
    c = _score_case("giant_group", n, [row], (1, 41, 410, 4096))
    for mx in (1, 41, 410):
        m = _models(c, 0, mx)
        assert m["T0"] == 5 and not m["usable"]
    return c


@functools.lru_cache(maxsize=None)
def take_all_boundary():
    """Exactly 4096 and exactly 4097 scores at or above the cut, found by the short cut, for M = 410 (rows 0, 1) and M
    = 4096 (rows 2, 3): 4096 are sorted as they come, 4097 go through the ordered pass, which skips one tie."""
    rng = np.random.default_rng(8350)
    n = 40000
    rows = [_row(rng, n, {9: 400, 8: 3696 + x, 7: 5000, 6: 5000}) for x in (0, 1)]
    rows += [_row(rng, n, {9: 1000, 8: 3096 + x, 7: 5000, 6: 5000}) for x in (0, 1)]
    c = _score_case("take_all_boundary", n, rows, (410, 4096))
    for qi, mx, n_ge in ((0, 410, 4096), (1, 410, 4097), (2, 4096, 4096), (3, 4096, 4097)):
        m = _models(c, qi, mx)
        assert m["exit"] == "found" and m["cut"] == 8 and m["n_ge_cut"] == n_ge and m["take_all"] == (n_ge == 4096)
    return c


TIE_FIRST = {"wave_range": 5120, "iteration_end": 5120 + 3 * 512 - 1, "mid_vector": 7003, "last_only": 19999}


@functools.lru_cache(maxsize=None)
def tie_split():
    """20 000 references: 2500 vectors, which the ordered pass gives to its four waves in ranges of 640 / 640 / 640 /
    580 vectors, read 64 vectors at a time.  Query 0: more than 4096 ties at the cut (score 2), dense below id 5120 and
    sparse from there on; the `max` values are chosen so that the first tie taken is the first id of wave range 1
    (5120), the last id of a 64-vector iteration (6655), an id in the middle of a vector (7003), and the last
    reference alone (all ties but one skipped).  Query 1: no tie skipped -- 4000 ties, 96 above, max = 4096, and no
    score 1 for the sample to place a threshold on, so the ordered pass runs."""
    rng = np.random.default_rng(8360)
    n = 20000
    above = np.array([5121, 6001, 9999, 10001, 12345, 15000, 17777, 19001, 19990, 19998])
    ids = np.arange(n)
    tie = (ids < 5120) | (ids % 8 == 0) | np.isin(ids, list(TIE_FIRST.values()))
    tie[above] = False
    tie[[7, 100, 5000]] = False
    row = np.where(tie, 2, rng.integers(0, 2, size=n)).astype(np.int64)
    row[above] = 3
    maxes = {name: len(above) + int((tie & (ids >= x)).sum()) for name, x in TIE_FIRST.items()}
    row1 = _row(rng, n, {3: 96, 2: 4000})
    c = _score_case("tie_split", n, [row, row1], sorted(set(maxes.values()) | {4096}))
    c.tie_maxes = maxes
    assert (2500 + 3) // 4 <= 640 and 640 % 64 == 0 and 640 * 8 == TIE_FIRST["wave_range"]
    assert (TIE_FIRST["iteration_end"] + 1 - 5120) % 512 == 0 and TIE_FIRST["mid_vector"] % 8 == 3
    assert tie.sum() > SEL_MAX and maxes["last_only"] == len(above) + 1
    for name, mx in maxes.items():
        got, sc = c.expected[0]["find"][mx]
        assert got[sc == 2].min() == TIE_FIRST[name] and (sc == 3).sum() == len(above)
        m = _models(c, 0, mx)
        assert m["exit"] == "unusable" or (m["exit"] == "found" and not m["take_all"])      # the ordered pass
    m = _models(c, 1, 4096)
    assert m["exit"] == "unusable" and (c.expected[1]["find"][4096][1] >= 2).all()
    return c


@functools.lru_cache(maxsize=None)
def narrow(n_refs):
    """Largest score 1, 2, 7, 8, 9: 8-way steps over fewer than 8 values."""
    rng = np.random.default_rng(8370 + n_refs % 100)
    c = _score_case("narrow_%d" % n_refs, n_refs, [_spread_row(rng, n_refs, top) for top in (1, 2, 7, 8, 9)], (1, 41, 410))
    assert [int(e["scores"].max()) for e in c.expected] == [1, 2, 7, 8, 9]
    return c


@functools.lru_cache(maxsize=None)
def no_windows():
    c = _score_case("no_windows", 5000, [np.zeros(5000, np.int64)], (1, 41, 410),
                    extra_lists={5: np.arange(0, 5000, 3, dtype=np.uint32)})
    assert len(kmer_ref.window_values(c.qmasks[0], c.k, False)) == 0 and (c.qmasks[0] == N_MASK).all()
    assert (c.expected[0]["find"][41][0] == np.arange(4999, 4958, -1)).all()
    return c


@functools.lru_cache(maxsize=None)
def top_8192():
    """Rows of the cases above behind queries padded with N to 10 240 bases: len - k = 10 234 >= 8192 bins, the short
    cut is skipped.  And AAAA...A of 10 240 bases against one list: the score 10 234."""
    rng = np.random.default_rng(8380)
    n = 20000
    rows = [_spread_row(rng, n), giant_group().expected[0]["scores"], sample_high().expected[1]["scores"]]
    lst = np.sort(rng.choice(n, 3000, replace=False)).astype(np.uint32)
    c = _score_case("top_8192", n, rows, (1, 41, 410, 4096), pad=FAST_MAX, extra_lists={0: lst},
                    extra_queries=[poly("A", FAST_MAX)])
    assert all(_models(c, qi, 410) is None for qi in range(4))
    assert _models(sample_high(), 1, 410) is not None
    s = c.expected[3]["scores"]
    assert s.max() == FAST_MAX - c.k == 10234 and (s > 0).sum() == 3000
    return c


@functools.lru_cache(maxsize=None)
def long_select():
    """Through kmer_topk_any / kmer_scores_any: AAAA...A of 32 767 bases, and a two-block query A...A N C...C of more
    than 10 240 bases whose lists give the four scores {0, a, c, a + c} in giant groups."""
    rng = np.random.default_rng(8390)
    n, k = 20000, 6
    la, lc = 6000, 6500
    in_a, in_c = rng.random(n) < 0.5, rng.random(n) < 0.4
    lists = {poly_kmer("A", k): np.flatnonzero(in_a).astype(np.uint32), poly_kmer("C", k): np.flatnonzero(in_c).astype(np.uint32)}
    qs = [poly("A", LONG_MAX), np.concatenate([poly("A", la), [N_MASK], poly("C", lc)]), poly("A", 40)]
    c = Case("long_select", n, k, True, lists, qs, (1, 41, 410, 4096), dense_divs=(None, "1"), long_api=True)
    a, cc_ = la - k + 1, lc - k          # (a block before an N keeps the window on its last base)
    assert set(np.unique(c.expected[1]["scores"])) == {0, a, cc_, a + cc_} and len(qs[1]) > FAST_MAX
    assert c.expected[0]["scores"].max() == LONG_MAX - k == 32761
    c.n_long = 2
    return c


# ---------------------------------------------------------------- candidate-list cases

CAND_N = 70000


def _cand_case(name, n_refs, rows, maxes=(1, 41, 128)):
    return _score_case(name, n_refs, rows, maxes, kmer_rows=(None, 1))


@functools.lru_cache(maxsize=None)
def winners_elsewhere():
    """Tile 0 holds only zeros: t0 = 0, every reference is a candidate, the list overflows and the host repeats the
    launch with the score rows."""
    rng = np.random.default_rng(8400)
    row = np.zeros(CAND_N, np.int64)
    at = TILE + rng.permutation(CAND_N - TILE)
    row[at[:300]] = rng.integers(1, 9, size=300)
    c = _cand_case("winners_elsewhere", CAND_N, [row])
    for mx in c.maxes:
        m = cand_model(row, mx)
        assert m["t0"] == 0 and m["overflow"] and expected_launches(c, mx, None) == 2
        assert (c.expected[0]["find"][mx][0] >= TILE).all()
    return c


@functools.lru_cache(maxsize=None)
def one_thread():
    """The top 128 lie inside the 32-reference blocks of two threads of tile 0 (plus 64 of a third's in tile 1); the
    M-th largest per-thread maximum is then a low score, which a few thousand references reach: the list holds them."""
    rng = np.random.default_rng(8410)
    row = np.zeros(CAND_N, np.int64)
    others = rng.permutation(CAND_N)[:3000]
    row[others] = 1
    for b in (32 * 5, 32 * 700):
        row[b:b + 32] = rng.integers(5, 10, size=32)
    row[TILE + 64:TILE + 128] = rng.integers(3, 5, size=64)
    c = _cand_case("one_thread", CAND_N, [row])
    for mx in c.maxes:
        m = cand_model(row, mx)
        assert not m["overflow"] and expected_launches(c, mx, None) == 1
    assert cand_model(row, 41)["t0"] == 1 and cand_model(row, 128)["t0"] == 1
    ids = c.expected[0]["find"][128][0]
    assert set(ids[:64].tolist()) == set(range(160, 192)) | set(range(22400, 22432))
    return c


@functools.lru_cache(maxsize=None)
def cap(n_cand):
    """Exactly n_cand references reach t0 = 5: 4096 fit the list (one launch), 4097 do not (two)."""
    rng = np.random.default_rng(8420)
    row = rng.integers(0, 5, size=CAND_N).astype(np.int64)
    row[np.arange(200) * THREAD_REFS * 3 + 7] = 5                   # 200 threads of tile 0
    rest = np.setdiff1d(np.arange(CAND_N), np.flatnonzero(row == 5))
    more = rng.choice(rest[rest >= TILE], n_cand - 200, replace=False)
    row[more] = rng.integers(5, 8, size=len(more))
    c = _cand_case("cap_%d" % n_cand, CAND_N, [row])
    for mx in c.maxes:
        m = cand_model(row, mx)
        assert m["t0"] == 5 and m["n_cand"] == n_cand and expected_launches(c, mx, None) == (1 if n_cand <= SEL_MAX else 2)
    return c


@functools.lru_cache(maxsize=None)
def ties_three_tiles():
    """The ties of the cut (score 5) in all three tiles: 10 in tile 2, 10 in tile 1, 110 in tile 0; with 20 scores
    above, max = 41 takes both upper tiles' ties and the largest id of tile 0's."""
    rng = np.random.default_rng(8430)
    row = rng.integers(0, 4, size=CAND_N).astype(np.int64)
    t0_ids = np.arange(130) * THREAD_REFS * 7 + 11                     # 130 threads of tile 0
    row[t0_ids[:110]] = 5
    row[t0_ids[110:]] = 6
    t1 = TILE + rng.choice(TILE, 10, replace=False)
    t2 = 2 * TILE + rng.choice(CAND_N - 2 * TILE, 10, replace=False)
    row[t1] = 5
    row[t2] = 5
    c = _cand_case("ties_three_tiles", CAND_N, [row])
    for mx in (41, 128):
        assert cand_model(row, mx)["t0"] == 5 and expected_launches(c, mx, None) == 1
    ids, sc = c.expected[0]["find"][41]
    assert (sc[:20] == 6).all() and (sc[20:] == 5).all()
    assert set(ids[20:40].tolist()) == set(t1.tolist()) | set(t2.tolist()) and ids[40] == t0_ids[109]
    return c


@functools.lru_cache(maxsize=None)
def two_full_tiles(n_refs):
    """65 536 references: exactly two tiles; 65 537: a third tile of one reference, which carries the top score.  max =
    128 takes the candidate path, 129 the score rows."""
    rng = np.random.default_rng(8440 + n_refs % 10)
    c = _cand_case("two_full_tiles_%d" % n_refs, n_refs, [_spread_row(rng, n_refs)], maxes=(128, 129))
    assert takes_cand_path(c, 128, None) and not takes_cand_path(c, 129, None) and not takes_cand_path(c, 128, 1)
    assert c.expected[0]["find"][128][0][0] == n_refs - 1
    return c


# ---------------------------------------------------------------- the matrix

COUNT_CASES = {"dense_nd": dense_nd, "dense_overflow": dense_overflow, "multiplicity": multiplicity,
               "cursor_lengths": cursor_lengths, "cursor_one_tile": cursor_one_tile,
               "fast_ignores_non_a": fast_ignores_non_a, "mixed_batch": mixed_batch,
               "mixed_batch_cand": mixed_batch_cand}
COUNT_CASES.update({"tile_geometry_%d" % n: functools.partial(tile_geometry, n) for n in EDGE_N_REFS})
SELECT_CASES = {"sample_high": sample_high, "sample_blind": sample_blind, "giant_group": giant_group,
                "take_all_boundary": take_all_boundary, "tie_split": tie_split, "no_windows": no_windows,
                "top_8192": top_8192, "long_select": long_select}
SELECT_CASES.update({"row_tail_%d" % n: functools.partial(row_tail, n) for n in (16376, 16377, 16384)})
SELECT_CASES.update({"zeros_fill_%d" % n: functools.partial(zeros_fill, n) for n in (5000, 20000)})
SELECT_CASES.update({"narrow_%d" % n: functools.partial(narrow, n) for n in (5000, 20000)})
CAND_CASES = {"winners_elsewhere": winners_elsewhere, "one_thread": one_thread, "cap_4096": functools.partial(cap, 4096),
              "cap_4097": functools.partial(cap, 4097), "ties_three_tiles": ties_three_tiles}
CAND_CASES.update({"two_full_tiles_%d" % n: functools.partial(two_full_tiles, n) for n in (65536, 65537)})
ALL_CASES = {**COUNT_CASES, **SELECT_CASES, **CAND_CASES}


def case(name):
    return ALL_CASES[name]()


# ---------------------------------------------------------------- fuzz

FUZZ_N_REFS = EDGE_N_REFS + (16376, 16377, 16384, 20000, 70000)


@functools.lru_cache(maxsize=None)
def fuzz_world(seed):
    """A seeded world (the ORDER of the draws is part of it: a seed names a case): n_refs from the edge list, k 6 or 8,
    fast or not, heavy-tailed list lengths on both sides of the dense threshold, 3 to 6 queries of random k-mers with
    multiplicities and N padding, a random dense_div, three random max values."""
    rng = np.random.default_rng(8500 + seed)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    n_refs = int(pick(FUZZ_N_REFS))
    k, nofast = int(pick([6, 8])), bool(rng.integers(0, 2))
    dd = pick([None, None, "1", "8", "1000000"])
    thr = dense_threshold(n_refs, dd)
    first = (1 << (2 * k)) if nofast else (1 << (2 * (k - 1)))            # (a fast index: k-mers that start with A)
    kmers = [int(x) for x in rng.choice(first, 240, replace=False)]
    lists = {}
    for v in kmers:
        ln = min(n_refs, int(thr * float(pick([0.01, 0.1, 0.5, 0.9, 1.1, 2.0, 8.0])) * float(rng.pareto(2.0) + 0.5)) + 1)
        ids = np.flatnonzero(rng.random(n_refs) < ln / n_refs).astype(np.uint32)
        if len(ids):
            lists[v] = ids
    qs = []
    for _ in range(int(rng.integers(3, 7))):
        parts = []
        for v in rng.choice(kmers + [int(x) for x in rng.integers(0, 1 << (2 * k), size=8)], int(pick([1, 5, 40, 200]))):
            parts.append(np.tile(query_of([int(v)], k), int(pick([1, 1, 1, 2, 9]))))
        q = np.concatenate(parts)[:9000 // (k + 1) * (k + 1)]
        qs.append(pad_n(q, len(q) + int(pick([0, 0, 1, 500]))))
    maxes = sorted(int(x) for x in rng.choice([1, 2, 40, 41, 128, 129, 400, 1000, 4096], size=3, replace=False))
    c = Case("fuzz_%d" % seed, n_refs, k, nofast, lists, qs, maxes, dense_divs=(dd,))
    return c
