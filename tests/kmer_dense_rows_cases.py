"""Cases for the bit-sliced bitmap loop of the k-mer count kernels (csrc/kmer_count_tile.inc) as it fetches its rows: a
wave reads the query's bitmap numbers 64 at a time, one per lane, pads them to a multiple of eight with the number of
an all-zero row, takes each number and its row's address on the scalar unit, and skips the loop in the waves of the last
tile that lie wholly behind the store's end.  Built on tests/kmer_cases.py (Case, _bernoulli_lists, dense_threshold,
query_of) with expected results from tests/kmer_ref.py alone; every builder asserts on the CPU that its case reaches
the edge it is there for.

Two things the kernels leave to the order of their atomics, and how the cases stand on either side of them: which
slot of the number list a window's bitmap lands in (so every list has a reference of its own that is in no other list:
whichever list is fetched last, its reference must score exactly one), and which number a dense k-mer gets (so every
dense k-mer that a query does not contain holds the references that must stay at zero: whichever of them is bitmap
number 0, a padding that read it would count them)."""
import functools

import numpy as np

from tests import kmer_cases as kc
from tests import kmer_ref

TILE = kc.TILE
WAVE_REFS = 2048                   # references of a tile that one wave of the bitmap loop owns: 64 lanes x 32
CHUNK = 64                         # bitmap numbers a wave fetches with one LDS read
K = 6
DECOYS = (0, 1, 2, 3)              # dense k-mers no query contains (AAAAAA first: the lowest k-mer value)
FIRST_KMER = 16


def wave_edges(n_refs):
    """(first, last) reference of every wave's range in every tile, as far as the store goes."""
    out = []
    for lo in range(0, n_refs, WAVE_REFS):
        out.append((lo, min(lo + WAVE_REFS, n_refs) - 1))
    return out


def live_waves_of_last_tile(n_refs):
    """How many of the 16 waves of the last tile own a reference below n_refs."""
    in_last = n_refs - (n_refs - 1) // TILE * TILE
    return (in_last + WAVE_REFS - 1) // WAVE_REFS


def _dense_kmers(c):
    return np.flatnonzero(c.list_lengths() > kc.dense_threshold(c.n_refs, None))


def _assert_decoys(c, qi):
    """A dense k-mer that query qi does not contain exists, and the lowest dense k-mer value is one."""
    w = set(kmer_ref.window_values(c.qmasks[qi], c.k, False).tolist())
    dense = _dense_kmers(c)
    assert int(dense.min()) == DECOYS[0] and not (w & set(DECOYS)) and len(set(DECOYS) & set(dense.tolist())) >= 2


# ---------------------------------------------------------------- the number fetch: chunk edges and the padding

ROWS_N = 70000
ROWS_ND = (9, 17, 65, 72, 129)
ROWS_ALL = (0, 2047, 2048, 32767, 32768, 69631, 69632, 69999)
ROWS_NONE = (4095, 4096, 65535, 65536, 67583, 67584)


@functools.lru_cache(maxsize=None)
def rows_world():
    """70 000 references (three tiles, the last with two whole waves and a partial third), k = 6.  133 dense lists of
    random membership: four decoys and 129 query lists.  ROWS_ALL are in every list, ROWS_NONE in the decoys only, and
    query list j has one reference of its own, singles[j], in no other list -- the first 56 of them first or last
    references of a wave's range, the rest the one or two references next to these."""
    rng = np.random.default_rng(9101)
    n, nl = ROWS_N, max(ROWS_ND)
    edges = wave_edges(n)
    flat = [r for pair in edges for r in pair]
    assert set(ROWS_ALL) | set(ROWS_NONE) <= set(flat) and {0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1} <= set(flat)
    used = set(ROWS_ALL) | set(ROWS_NONE)
    at_edge = [r for r in flat if r not in used]
    inner = [r for d in (1, 2) for lo, hi in edges for r in (lo + d, hi - d)]
    singles = (at_edge + [r for r in inner if r not in used])[:nl]
    assert len(singles) == nl == len(set(singles)) and len(at_edge) == 56 and not (set(singles) & used)
    j = np.arange(len(DECOYS) + nl)
    decoy, query = j < len(DECOYS), j >= len(DECOYS)
    force = {r: decoy | query for r in ROWS_ALL}
    force.update({r: decoy for r in ROWS_NONE})
    force.update({r: j == len(DECOYS) + x for x, r in enumerate(singles)})
    dens = rng.choice([0.02, 0.05, 0.3], p=[0.9, 0.08, 0.02], size=len(j))
    rows = kc._bernoulli_lists(rng, n, dens, force)
    lists = {v: rows[x] for x, v in enumerate(DECOYS)}
    lists.update({FIRST_KMER + x: rows[len(DECOYS) + x] for x in range(nl)})
    return lists, tuple(singles)


@functools.lru_cache(maxsize=None)
def rows_nd():
    """One query per nd of ROWS_ND over the first nd query lists: one number more than a body of eight (9, 17), than a
    chunk of 64 (65), than two (129), and a chunk plus exactly one body (72).  9, 17, 65 and 129 are 1 mod 8 -- seven
    numbers of padding -- and 72 is 0 mod 8, none.  Candidate lists and score rows."""
    lists, singles = rows_world()
    qs = [kc.query_of(range(FIRST_KMER, FIRST_KMER + nd), K) for nd in ROWS_ND]
    c = kc.Case("rows_nd", ROWS_N, K, True, lists, qs, (1, 41), dense_divs=(None,), kmer_rows=(None, 1),
                labels=["rows_nd_%d" % nd for nd in ROWS_ND])
    assert kc.dense_threshold(ROWS_N, None) == 1093 and len(_dense_kmers(c)) == len(DECOYS) + max(ROWS_ND) == kc.n_dense_lists(c, None)
    assert [nd % 8 for nd in ROWS_ND] == [1, 1, 1, 0, 1] and [nd > CHUNK for nd in ROWS_ND] == [False, False, True, True, True]
    assert ROWS_ND[2] == CHUNK + 1 and ROWS_ND[3] == CHUNK + 8 and ROWS_ND[4] == 2 * CHUNK + 1
    for qi, nd in enumerate(ROWS_ND):
        assert kc.n_dense_windows(c, qi, None) == nd
        _assert_decoys(c, qi)
        s = c.expected[qi]["scores"]
        assert all(s[r] == nd for r in ROWS_ALL) and all(s[r] == 0 for r in ROWS_NONE) and s.max() == nd
        assert all(s[r] == (1 if x < nd else 0) for x, r in enumerate(singles))
        assert kc.takes_cand_path(c, 41, None) and kc.expected_launches(c, 41, None) == 1
    return c


# ---------------------------------------------------------------- the last tile's dead waves

LAST_TILE_R = (1, 31, 32, 33, 2047, 2048, 2049)
LAST_TILE_N = tuple(TILE + r for r in LAST_TILE_R) + (2 * TILE,) + (2 * TILE + 1, 2 * TILE + 2049)


@functools.lru_cache(maxsize=None)
def last_tile(n_refs):
    """A store that ends 1 .. 2049 references into its last tile (or exactly on a tile end: 65 536): one wave live, one
    wave live and full, two.  Twenty dense query lists and two decoys.  The store's last reference is in all twenty,
    the first reference of the last live wave in every second one, the last reference of the wave before it in the
    others.  Query 0 takes all twenty lists -- its best reference is the store's last -- and query 1 the first nine."""
    rng = np.random.default_rng(9200 + n_refs % 4099)
    nl = 20
    last = n_refs - 1
    live = live_waves_of_last_tile(n_refs)
    first_live = last // TILE * TILE + WAVE_REFS * (live - 1)
    j = np.arange(2 + nl)
    query = j >= 2
    force = {last: query}
    if first_live != last:
        force[first_live] = query & (j % 2 == 0)
    force[first_live - 1] = query & (j % 2 == 1)
    rows = kc._bernoulli_lists(rng, n_refs, np.full(len(j), 0.04), force)
    lists = {v: rows[x] for x, v in enumerate(DECOYS[:2])}
    lists.update({FIRST_KMER + x: rows[2 + x] for x in range(nl)})
    qs = [kc.query_of(range(FIRST_KMER, FIRST_KMER + nl), K), kc.query_of(range(FIRST_KMER, FIRST_KMER + 9), K)]
    c = kc.Case("last_tile_%d" % n_refs, n_refs, K, True, lists, qs, (1, 41), dense_divs=(None,), kmer_rows=(None, 1))
    assert len(_dense_kmers(c)) == 2 + nl and [kc.n_dense_windows(c, qi, None) for qi in range(2)] == [nl, 9]
    assert first_live <= last < first_live + WAVE_REFS and first_live % WAVE_REFS == 0 and last // TILE == first_live // TILE
    assert (live < 16) == (n_refs % TILE != 0) and live == {1: 1, 31: 1, 32: 1, 33: 1, 2047: 1, 2048: 1, 2049: 2, 0: 16}[n_refs % TILE]
    s0, s1 = c.expected[0]["scores"], c.expected[1]["scores"]
    assert s0[last] == nl and s0[:last].max() < nl and c.expected[0]["find"][1][0][0] == last and s1[last] == 9
    assert s0[first_live - 1] == nl // 2 and (first_live == last or s0[first_live] == nl // 2)
    for qi in range(2):
        _assert_decoys(c, qi)
    assert kc.takes_cand_path(c, 41, None) == (n_refs >= 2 * TILE)
    return c


# ---------------------------------------------------------------- the long kernel: chunks that add to the row

LONG_N = 33000
LONG_ALL = (0, 2047, 2048, 32767, 32768, 32999)
LONG_NONE = (1, 4095, 32769)


def _chunks(mask):
    return [mask[lo:lo + kc.capi.KMER_LONG_CHUNK] for lo in range(0, len(mask), kc.capi.KMER_LONG_CHUNK)]


@functools.lru_cache(maxsize=None)
def long_rows():
    """Through sina_hip_kmer_scores_any / kmer_topk_any on the long count kernel: a query of 10 241 bases with 65 dense
    windows, and one of 20 550 bases whose three chunks hold 9, 65 and 9 -- the third chunk the k-mers of the first
    again -- so that the second and third chunk ADD to a row the first has written.  Every chunk ends on Ns: no window
    lies across a chunk end, a chunk's windows are those of its slice."""
    rng = np.random.default_rng(9301)
    n, nl = LONG_N, 74
    j = np.arange(2 + nl)
    force = {r: j >= 0 for r in LONG_ALL}
    force.update({r: j < 2 for r in LONG_NONE})
    rows = kc._bernoulli_lists(rng, n, np.full(len(j), 0.04), force)
    lists = {v: rows[x] for x, v in enumerate(DECOYS[:2])}
    lists.update({FIRST_KMER + x: rows[2 + x] for x in range(nl)})
    km = list(range(FIRST_KMER, FIRST_KMER + nl))
    C = kc.capi.KMER_LONG_CHUNK
    q1 = kc.pad_n(kc.query_of(km[:65], K), C + 1)
    q2 = kc.pad_n(np.concatenate([kc.pad_n(kc.query_of(km[:9], K), C), kc.pad_n(kc.query_of(km[9:], K), C), kc.query_of(km[:9], K)]),
                  2 * C + 70)
    c = kc.Case("long_rows", n, K, True, lists, [q1, q2], (1, 41), dense_divs=(None,), long_api=True)
    c.n_long = 2
    assert len(q1) == 10241 and len(q2) == 20550 and C == kc.FAST_MAX == 10240 and len(_dense_kmers(c)) == 2 + nl
    ln = c.list_lengths()
    thr = kc.dense_threshold(n, None)
    per_chunk = [[int((ln[kmer_ref.window_values(part, K, False)] > thr).sum()) for part in _chunks(q)] for q in (q1, q2)]
    assert per_chunk == [[65, 0], [9, 65, 9]]
    assert [kc.n_dense_windows(c, qi, None) for qi in range(2)] == [65, 83]       # (no window lost at a chunk end)
    s1, s2 = c.expected[0]["scores"], c.expected[1]["scores"]
    assert all(s1[r] == 65 and s2[r] == 83 for r in LONG_ALL) and all(s1[r] == 0 and s2[r] == 0 for r in LONG_NONE)
    assert (s2 >= 2).sum() > 1000                   # (references the first chunk and a later one both count)
    for qi in range(2):
        _assert_decoys(c, qi)
    return c


# ---------------------------------------------------------------- the matrix

CASES = {"rows_nd": rows_nd, "long_rows": long_rows, "dense_overflow": kc.dense_overflow}
CASES.update({"last_tile_%d" % n: functools.partial(last_tile, n) for n in LAST_TILE_N})


def case(name):
    return CASES[name]()
