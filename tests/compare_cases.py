"""Named inputs of the comparison tests, shared by tests/test_compare_cpu.py (which pins tests/compare_ref.py to the
oracle on every one of them) and tests/test_gpu_compare.py (which runs them through sina_hip_compare).

A case is a function returning (width, reference list, query list, candidate id lists): packed base lists
(column | mask << 24, bit 4 of the mask byte = lower case, columns strictly ascending) and, per query, the ids of the
references it is compared with.  Every builder asserts, in plain numpy, the property it exists for before anything is
compared -- a case that stops reaching its edge fails on any machine.  Everything here is CPU work."""
import functools
import itertools

import numpy as np

from tests import compare_ref

KCT = 256          # threads per workgroup of compare_kernel: the prefix scan gives each ceil(nwords / 256) words
LC = 0x10


def seq(cols, masks=None, lower=None):
    """Packed base list from columns (sorted here) and masks (default: A G C U by base index).  lower: indices, in
    column order, of the bases that get the lower-case bit."""
    cols = np.asarray(list(cols), np.int64)
    order = np.argsort(cols, kind="stable")
    cols = cols[order]
    assert len(np.unique(cols)) == len(cols) and (len(cols) == 0 or (cols[0] >= 0 and cols[-1] < (1 << 24)))
    if masks is None:
        masks = np.array([1, 2, 4, 8], np.uint32)[np.arange(len(cols)) % 4]
    else:
        masks = np.asarray(list(masks), np.uint32)[order]      # (a mask stays with its column)
    m = np.asarray(masks, np.uint32).copy()
    assert len(m) == len(cols)
    if lower is not None:
        m[np.asarray(lower)] |= LC
    return (cols.astype(np.uint32) | (m << 24)).astype(np.uint32)


def cols(s):
    return (np.asarray(s, np.uint32) & 0xFFFFFF).astype(np.int64)


def masks(s):
    return (np.asarray(s, np.uint32) >> 24).astype(np.int64)


def upper(s):
    """The bases the lower-case filter keeps."""
    s = np.asarray(s, np.uint32)
    return s[(masks(s) & LC) == 0]


def nwords(width):
    return (width + 31) // 32


def chunk(width):
    return (nwords(width) + KCT - 1) // KCT


def _all_pairs(width, refs, queries=None):
    queries = refs if queries is None else queries
    ids = np.arange(len(refs), dtype=np.uint32)
    return width, refs, queries, [ids.copy() for _ in queries]


# ---------------------------------------------------------------- word and width edges

def _width_case(width):
    def build():
        edge = sorted({c for c in (0, 31, 32, 63, width - 1) if 0 <= c < width})
        inner = [c for c in range(1, width - 1, max(1, width // 40)) if c not in edge][:40]
        E = seq(edge, [1 << (c % 4) for c in edge])
        E2 = seq(edge, [1 << ((c // 31) % 4) for c in edge])           # other masks: matches and mismatches
        I = seq(inner)
        EI = seq(edge + inner, lower=[0] if len(edge) + len(inner) > 2 else None)
        assert nwords(width) == (width + 31) // 32 and (width % 32 == 0) == (width in (32, 64))
        assert width - 1 in cols(E) and 0 in cols(E) and set(cols(E)) >= {c for c in (31, 32, 63) if c < width}
        assert not set(cols(I)) & set(edge)            # edge columns on one side only in E x I and I x E
        return _all_pairs(width, [E, E2, I, EI])
    return build


# ---------------------------------------------------------------- scan chunking

def _nwords_case(n):
    def build():
        width = 32 * n - 5                             # (not a multiple of 32: the last word is partial)
        ch = chunk(width)
        assert nwords(width) == n and width % 32 != 0
        borders = [t * ch for t in range(1, KCT) if t * ch < n]
        idle = [t for t in range(KCT) if min(n, t * ch) == min(n, min(n, t * ch) + ch)]   # threads with b == e == nwords
        assert (len(idle) > 0) == (n not in (256, 511, 512)) and (n % ch != 0) == (n in (257, 511, 1563))
        assert ch == {255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3, 1563: 7}[n]
        qc = {0, 5}
        for w in borders:                              # last bit of one thread's chunk, first bit of the next one's
            qc |= {32 * w - 1, 32 * w}
        qc |= set(range(32 * (n - 3), width))          # the last three words, full
        qc = sorted(qc)
        q = seq(qc)                                    # masks cycle with the rank: a rank off by one is a mismatch
        assert width - 1 in qc and all(32 * w in qc and 32 * w - 1 in qc for w in borders)
        half = len(qc) // 2
        qset = set(qc)
        # candidates with the query's own masks on shared columns, so that the plain walk finds no mismatch there
        def part(sel, extra):
            c = np.concatenate([cols(q)[sel], np.asarray(extra, np.int64)])
            m = np.concatenate([masks(q)[sel], np.full(len(extra), 15)])
            o = np.argsort(c)
            return seq(c[o], m[o])
        free = lambda lo, hi, k: list(itertools.islice((c for c in range(lo, hi) if c not in qset), k))  # noqa: E731
        second = part(slice(half, None), free(qc[half] + 1, width, 6))              # overlaps the query's second half
        first = part(slice(0, half), free(1, qc[half], 6))                          # ... its first half
        every_other = part(slice(1, None, 2), [])                                   # only_a needs rank(bL + 1) - rank(bF)
        mid = part(slice(half // 2, half + half // 2), free(qc[half // 2] + 1, qc[half], 3))
        for c in (second, mid):
            assert cols(q)[0] < cols(c)[0] <= cols(q)[-1]                            # partial overlap
        assert cols(first)[-1] < cols(q)[-1] and cols(every_other)[0] > cols(q)[0]
        for c in (second, first, every_other, mid):
            assert compare_ref.compare_ref(q, c, 2, False)[5] == 0                   # no mismatch by construction
        return width, [second, first, every_other, mid], [q, second], [np.arange(4, dtype=np.uint32)] * 2
    return build


# ---------------------------------------------------------------- range relations

def ranges():
    width = 203
    S = dict(
        left=seq(range(10, 41, 3)),                                  # 10 .. 40
        right=seq(range(50, 91, 2), [8, 4, 2, 1] * 5 + [8]),          # 50 .. 90
        touch=seq(range(40, 71, 2)),                                 # starts in left's last column
        big=seq(range(4, 181, 2)),
        big2=seq([4] + list(range(7, 178, 4)) + [180], lower=[3]),    # big's range, other interior
        inner=seq(range(60, 101, 3)),                                # nested in big, shares every second column
        one77=seq([77], [4]), one77b=seq([77], [2]), one78=seq([78], [4]),
    )
    lo = {k: int(cols(v)[0]) for k, v in S.items()}
    hi = {k: int(cols(v)[-1]) for k, v in S.items()}
    assert hi["left"] < lo["right"]                                           # A wholly left of B, and the reverse
    assert hi["left"] == lo["touch"]                                          # aL == bF; as (touch, left): bL == aF
    assert lo["big"] < lo["inner"] and hi["inner"] < hi["big"]                # nested either way
    assert (lo["big"], hi["big"]) == (lo["big2"], hi["big2"]) and set(cols(S["big"])) != set(cols(S["big2"]))
    assert len(S["one77"]) == len(S["one78"]) == 1 and 77 not in cols(S["big"]) and 78 in cols(S["big"])
    names = sorted(S)
    return _all_pairs(width, [S[k] for k in names])


# ---------------------------------------------------------------- the lower-case filter

def filter_cases():
    width = 100
    c = list(range(10, 61, 2))
    U = seq(c)
    allow = seq(c, lower=range(len(c)))
    ends = seq(range(0, 91, 3), lower=[0, 1, 2, 3, 27, 28, 29, 30])   # first 4 and last 4 bases lower case
    odd = seq(range(1, 96, 2))
    inner_lc = seq(c, lower=[5, 6, 12])                               # lower-case partners in the interior
    facing_gap = seq(c + [31], lower=[c.index(30) + 1])               # a lower-case base where U has no base
    assert len(upper(allow)) == 0 and len(upper(U)) == len(U)
    e_up = cols(upper(ends))
    assert len(ends) == 31 and e_up[0] == 12 and e_up[-1] == 78
    # bases of the other side between the whole and the trimmed range: inside without the filter, overhang with it
    for o in (odd, U):
        oc = cols(o)
        assert ((oc > 0) & (oc < e_up[0])).any() or ((oc > e_up[-1]) & (oc < 90)).any()
    assert ((cols(odd) > 0) & (cols(odd) < 12)).any() and ((cols(odd) > 78) & (cols(odd) < 90)).any()
    assert set(cols(inner_lc)) == set(cols(U)) and 0 < len(upper(inner_lc)) < len(U)
    lc_col = int(cols(facing_gap)[masks(facing_gap) & LC != 0][0])
    assert lc_col == 31 and lc_col not in cols(U) and cols(U)[0] < lc_col < cols(U)[-1]
    return _all_pairs(width, [U, allow, ends, odd, inner_lc, facing_gap])


# ---------------------------------------------------------------- masks

def _mask_table(lower):
    def build():
        c = np.arange(256)
        qm, rm = c >> 4, c & 15
        assert {(int(a), int(b)) for a, b in zip(qm, rm)} == {(a, b) for a in range(16) for b in range(16)}
        ql = np.flatnonzero(c * 7 % 5 == 0) if lower else None
        rl = np.flatnonzero(c * 11 % 3 == 0) if lower else None
        q, r = seq(c, qm, ql), seq(c, rm, rl)
        if lower:
            both = (masks(q) & LC != 0) & (masks(r) & LC != 0)
            assert both.any() and (masks(q) & LC != 0).sum() > both.sum() < (masks(r) & LC != 0).sum()
            assert masks(q)[0] & LC and masks(r)[0] & LC and masks(q)[255] & LC       # filtered ends are trimmed
        return 256, [r, q], [q, r], [np.array([0, 1], np.uint32)] * 2
    return build


# ---------------------------------------------------------------- lengths

def lengths():
    width = 1100
    rng = np.random.default_rng(5101)

    def rnd(n):
        c = np.sort(rng.choice(width, size=n, replace=False))
        m = rng.integers(1, 16, size=n)
        return seq(c, m, np.flatnonzero(rng.random(n) < 0.1))
    refs = [rnd(n) for n in (1, 63, 64, 65, 129)]
    qs = [rnd(n) for n in (1, 255, 256, 257, 513)]
    assert [len(r) for r in refs] == [1, 63, 64, 65, 129] and [len(q) for q in qs] == [1, 255, 256, 257, 513]
    return _all_pairs(width, refs, qs)


# ---------------------------------------------------------------- candidate lists

def _small_world(seed, n_refs, width=90):
    rng = np.random.default_rng(seed)
    anc = rng.choice([1, 2, 4, 8], size=width)
    out = []
    for _ in range(n_refs):
        lo = int(rng.integers(0, width // 2))
        hi = int(rng.integers(lo + 4, width + 1))
        c = np.flatnonzero(rng.random(hi - lo) < 0.6) + lo
        if len(c) == 0:
            c = np.array([lo])
        m = anc[c].copy()
        sub = rng.random(len(c)) < 0.2
        m[sub] = rng.choice([1, 2, 4, 8, 5, 15], size=int(sub.sum()))
        out.append(seq(c, m, np.flatnonzero(rng.random(len(c)) < 0.1)))
    return out


def cand_lists():
    refs = _small_world(5201, 12)
    qs = _small_world(5202, 11)
    L = lambda *ids: np.array(ids, np.uint32)  # noqa: E731
    cand = [L(), L(), L(3), L(0, 5, 11), L(), L(1, 2, 3, 4), L(4, 3, 2, 1, 0), L(*range(9)), L(), L(7, 3, 7, 9), L()]
    sizes = [len(x) for x in cand]
    assert set(sizes) == {0, 1, 3, 4, 5, 9}
    assert sizes[0] == sizes[1] == 0 and sizes[-1] == 0 and 0 in sizes[2:-1]   # empty lists first, inside and last
    assert list(cand[9]).count(7) == 2                                         # one id twice in a list
    assert sum(3 in x for x in cand) >= 4                                      # one id in several lists
    return 90, refs, qs, cand


def nq_1():
    refs = _small_world(5211, 3)
    return 90, refs, _small_world(5212, 1), [np.array([2], np.uint32)]


def nq_600():
    """More workgroups than the chip has compute units (256): 600 one-candidate queries of 3 to 6 bases."""
    refs = _small_world(5221, 7)
    rng = np.random.default_rng(5222)
    qs = []
    for _ in range(600):
        n = int(rng.integers(3, 7))
        qs.append(seq(rng.choice(90, size=n, replace=False), rng.choice([1, 2, 4, 8, 3], size=n),
                      np.flatnonzero(rng.random(n) < 0.15)))
    cand = [np.array([i % 7], np.uint32) for i in range(600)]
    assert len(qs) == 600 > 256 and all(3 <= len(q) <= 6 for q in qs) and all(len(c) == 1 for c in cand)
    return 90, refs, qs, cand


# ---------------------------------------------------------------- the top of the 16-bit rank

def rank_top():
    width = 65700
    qc = np.arange(100, 100 + 65535)
    q = seq(qc)
    assert len(q) == 65535 == 0xFFFF and qc[-1] < width and width >= 65535
    last40 = seq(list(qc[-40:]) + [65650, 65699], list(masks(q)[-40:]) + [1, 2])
    first40 = seq([0, 50] + list(qc[:40]), [1, 2] + list(masks(q)[:40]))
    span = seq(list(range(0, width - 1, 997)) + [width - 1])
    assert cols(last40)[0] == qc[-40] and cols(last40)[-1] > qc[-1]           # overlaps the last 40 bases only
    assert cols(first40)[0] < qc[0] and cols(first40)[-1] == qc[39]
    assert cols(span)[0] < qc[0] and cols(span)[-1] > qc[-1]
    return width, [last40, first40, span], [q], [np.arange(3, dtype=np.uint32)]


# ---------------------------------------------------------------- dynamic LDS above 64 KB

WIDE = 524288


def lds_bytes(width, max_la):
    """What sina_hip_compare asks for: bitmap, 16-bit ranks, masks by rank, alignment slack."""
    return 4 * nwords(width) + 2 * (nwords(width) + 2) + max_la + 31


def _wide_seq(rng, words, per_word, must=()):
    c = set(must)
    for w in words:
        c |= {32 * w + int(b) for b in rng.choice(32, size=per_word, replace=False)}
    c = sorted(c)
    return seq(c, rng.choice([1, 2, 4, 8, 5], size=len(c)), np.flatnonzero(rng.random(len(c)) < 0.1))


def lds_wide():
    rng = np.random.default_rng(5301)
    n = nwords(WIDE)
    mid = n // 2
    q0 = _wide_seq(rng, [0, 1, mid, n - 2, n - 1], 20, must=(0, 31, 32 * mid, WIDE - 1))
    q1 = _wide_seq(rng, [mid - 1, mid, mid + 1, n - 1], 25, must=(32 * mid + 31,))
    q2 = _wide_seq(rng, [0, 7, 4095, 8000], 24, must=(1,))
    refs = [_wide_seq(rng, [0, mid], 24, must=(0, 31)), _wide_seq(rng, [mid, n - 1], 24, must=(WIDE - 1,)),
            _wide_seq(rng, [1, 4095, mid + 1, n - 2], 16), seq(cols(q0)[::2], masks(q0)[::2] & 15)]
    assert lds_bytes(WIDE, max(len(q) for q in (q0, q1, q2))) > 64 * 1024
    assert {0, 31, 32 * mid, WIDE - 1} <= set(cols(q0)) and all(90 <= len(q) <= 110 for q in (q0, q1, q2))
    assert cols(refs[0])[-1] < cols(q0)[-1] and cols(refs[1])[0] > cols(q0)[0]   # partial overlap
    return _all_pairs(WIDE, refs, [q0, q1, q2])


LDS_LIMIT = 150 * 1024
LIMIT_LA = LDS_LIMIT - lds_bytes(WIDE, 0)      # the longest query the widest accepted alignment leaves room for


def lds_limit(extra=0):
    """One query of LIMIT_LA (+ extra) bases at width 524288: with extra = 0 the largest LDS request the entry point
    accepts, with extra = 1 the smallest it refuses."""
    la = LIMIT_LA + extra
    assert lds_bytes(WIDE, LIMIT_LA) == LDS_LIMIT and lds_bytes(WIDE, LIMIT_LA + 1) > LDS_LIMIT and la <= 65535
    qc = np.concatenate([np.arange(0, 6000), WIDE - 1 - np.arange(la - 6000)[::-1]])
    q = seq(qc)
    assert len(q) == la
    r0 = seq(list(qc[5990:6010:2]) + [300000], list(masks(q)[5990:6010:2]) + [15])
    r1 = seq([qc[0], 7000, int(qc[-1])], [int(masks(q)[0]), 1, int(masks(q)[-1])])
    return WIDE, [r0, r1], [q], [np.array([0, 1], np.uint32)]


# ---------------------------------------------------------------- registry

CASES = {}
for _w in (1, 31, 32, 33, 64, 65, 2500):
    CASES["width_%d" % _w] = _width_case(_w)
for _n in (255, 256, 257, 511, 512, 513, 1563):
    CASES["nwords_%d" % _n] = _nwords_case(_n)
CASES.update(ranges=ranges, filter=filter_cases, mask_table=_mask_table(False), mask_table_lc=_mask_table(True),
             lengths=lengths, cand_lists=cand_lists, nq_1=nq_1, nq_600=nq_600, rank_top=rank_top, lds_wide=lds_wide,
             lds_limit=lds_limit)
NAMES = sorted(CASES)
SETTINGS = [(rule, flc) for rule in (0, 1, 2) for flc in (False, True)]


@functools.lru_cache(maxsize=None)
def case(name):
    width, refs, qs, cand = CASES[name]()
    check_wellformed(width, refs, qs, cand)
    return width, refs, qs, cand


def check_wellformed(width, refs, qs, cand):
    assert len(cand) == len(qs)
    for s in list(refs) + list(qs):
        c = cols(s)
        assert s.dtype == np.uint32 and (np.diff(c) > 0).all() and (len(c) == 0 or c[-1] < width)
    for ids in cand:
        assert ids.dtype == np.uint32 and (len(ids) == 0 or ids.max() < len(refs))


@functools.lru_cache(maxsize=None)
def expected(name, seed=None):
    """{(rule, filter_lc): int array [n pairs][6]} of a named case (or of fuzz seed `seed`) by the plain walk, pairs in
    launch order.  Computed once per process and shared."""
    width, refs, qs, cand = case(name) if seed is None else fuzz_case(seed)
    return {(rule, flc): walk_all(refs, qs, cand, rule, flc) for rule, flc in SETTINGS}


def walk_all(refs, qs, cand, rule, flc):
    rows = [compare_ref.compare_ref(q, refs[int(i)], rule, flc) for q, ids in zip(qs, cand) for i in ids]
    return np.asarray(rows, np.int32).reshape(-1, 6)


def offsets(parts):
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return off


def flat(parts):
    return np.concatenate([np.asarray(p, np.uint32) for p in parts] + [np.zeros(0, np.uint32)])


# ---------------------------------------------------------------- the seeded fuzz generator

FUZZ_WIDTHS = (40, 333, 2500, 8224, 50000)


@functools.lru_cache(maxsize=None)
def fuzz_case(seed):
    """Random width, base density, ambiguity and lower-case rates (0 to 0.9); references drawn around a common
    ancestor; queries made from references the way _aligned_queries of tests/test_gpu_search.py makes them
    (substitutions, a trimmed window, bases dropped, bases moved to a free neighbouring column); candidate lists of 0
    to 40 ids (an id may repeat).  The two rates are the seed's ceilings: every sequence draws its own below them, so
    that a seed with a high ceiling still has pairs with bases left.  Every seed also carries a reference and a query
    that are lower case throughout and an empty reference, so that a side without a remaining base occurs with and
    without the filter."""
    rng = np.random.default_rng(77000 + seed)
    width = int(FUZZ_WIDTHS[int(rng.integers(len(FUZZ_WIDTHS)))])
    density = float(rng.uniform(0.05, 0.45))                  # (at least two columns per base: room to differ)
    amb_rate, lower_rate = float(rng.uniform(0, 0.9)), float(rng.uniform(0, 0.9))
    drop = float(rng.choice([0.03, 0.1, 0.25]))                # bases a sequence lacks against its source
    length = int(min(400, max(6, density * width)))            # bases per full reference
    stride = max(1, width // length)
    anc = rng.choice([1, 2, 4, 8], size=width)
    n_refs = int(rng.integers(20, 50))
    refs = []
    for _ in range(n_refs):
        a, b = sorted(int(x) for x in rng.integers(0, length + 1, size=2))
        if b - a < 3 or rng.random() < 0.3:
            a, b = 0, length
        c = np.arange(a, b) * stride + rng.integers(0, stride, size=b - a)
        c = c[rng.random(len(c)) > drop]
        m = anc[c].copy()
        sub = rng.random(len(c)) < 0.1
        m[sub] = rng.choice([1, 2, 4, 8], size=int(sub.sum()))
        amb = rng.random(len(c)) < rng.uniform(0, amb_rate)
        m[amb] = rng.choice([3, 5, 7, 15, 12], size=int(amb.sum()))
        refs.append(seq(c, m, np.flatnonzero(rng.random(len(c)) < rng.uniform(0, lower_rate))))
    refs[1] = refs[1] | np.uint32(LC << 24)
    refs[2] = np.zeros(0, np.uint32)
    qs = []
    for _ in range(int(rng.integers(4, 8))):
        for _ in range(50):                                    # (a few bases must remain)
            ab = refs[int(rng.integers(3, n_refs))].copy()
            if len(ab) >= 6:
                a, b = sorted(int(x) for x in rng.integers(0, len(ab), size=2))
                if b - a >= 3:
                    ab = ab[a:b]
            ab = ab[rng.random(len(ab)) > drop]
            if len(ab) >= 2:
                break
        pos, m = cols(ab), masks(ab).astype(np.uint32)
        sub = rng.random(len(ab)) < 0.05
        m[sub] = rng.choice([1, 2, 4, 8], size=int(sub.sum()))
        amb = rng.random(len(ab)) < rng.uniform(0, amb_rate) / 4
        m[amb] = rng.choice([3, 5, 7, 15, 12], size=int(amb.sum()))
        m[rng.random(len(ab)) < rng.uniform(0, lower_rate) / 4] |= LC
        for x in np.flatnonzero(rng.random(len(ab)) < 0.04):   # one column to the right when that column is free
            nxt = pos[x + 1] if x + 1 < len(pos) else width
            if pos[x] + 1 < nxt:
                pos[x] += 1
        qs.append((pos.astype(np.uint32) | (m << 24)).astype(np.uint32))
    qs[1] = qs[1] | np.uint32(LC << 24)
    sizes = [0 if rng.random() < 0.15 else int(rng.integers(1, 41)) for _ in qs]
    cand = [rng.integers(0, n_refs, size=n).astype(np.uint32) for n in sizes]
    # one mismatch and one match that no rule and no filter setting takes away: a column where query 0 has G and
    # reference 0 has A, and one where both have A
    assert len(qs[0]) >= 2
    for k, qmask in ((len(qs[0]) // 2, 2), (len(qs[0]) // 2 - 1, 1)):
        p0 = int(cols(qs[0])[k])
        qs[0][k] = np.uint32(p0 | (qmask << 24))
        keep = cols(refs[0]) != p0
        refs[0] = seq(list(cols(refs[0])[keep]) + [p0], list(masks(refs[0])[keep]) + [1])
    cand[0] = np.concatenate([np.array([1, 2, 0], np.uint32), cand[0]])[:40]
    cand[1] = np.concatenate([np.array([0, 3, 4], np.uint32), cand[1]])[:40]
    check_wellformed(width, refs, qs, cand)
    return width, refs, qs, cand


def fuzz_coverage(seed):
    """The condition on the generator: per setting every counter is nonzero for some pair, and a pair with a side
    that has no remaining base occurs (without the filter: the empty reference)."""
    width, refs, qs, cand = fuzz_case(seed)
    exp = expected("fuzz", seed)
    for (rule, flc), rows in exp.items():
        assert len(rows) == sum(len(c) for c in cand)
        assert (rows != 0).any(axis=0).all(), (seed, rule, flc, (rows != 0).any(axis=0))
        left = lambda s: len(upper(s)) if flc else len(s)  # noqa: E731
        assert any(left(q) == 0 or left(refs[int(i)]) == 0 for q, ids in zip(qs, cand) for i in ids), (seed, rule, flc)
    assert any(len(upper(q)) == 0 and len(q) > 0 for q, ids in zip(qs, cand) if len(ids))
