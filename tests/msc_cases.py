"""Named inputs of the match-count tests beyond tests/compare_cases.py: what a column -> nibble table, a (query, chunk)
grid and a streaming candidate loop can get wrong.  Shared by tests/test_msc_cpu.py (which checks the identity
reduction on every one of them) and tests/test_gpu_msc.py (which runs them through the kernel).

A case is a function returning (width, reference list, query list, candidate id lists) in compare_cases' format:
packed base lists (column | mask << 24, bit 4 of the mask byte = lower case, columns strictly ascending).  Unlike
compare_cases a query may have bases at or beyond `width` (a reference may not).  Every builder asserts its edge in
plain numpy before anything is compared.  Everything here is CPU work."""
import functools

import numpy as np

from tests import compare_cases as cc
from tests import compare_ref

CHUNK_FLOOR = 64       # kMatchChunkFloor (csrc/match_plan.h)
WG_PER_CU = 4          # kMatchWgPerCu
GRID_MAX = 0x7FFFFFFF  # kMatchGridMax
N_CU = 256             # compute units of an MI355X: what the chunk cases are built for
MAX_WIDTH = 327680     # the widest alignment whose table fits a workgroup's LDS (160 KiB of nibbles)

seq, cols, masks = cc.seq, cc.cols, cc.masks


def plan(nq, M, n_cu=N_CU):
    """(chunk, chunks) of csrc/match_plan.h's match_plan; tests/test_msc_cpu.py pins this mirror to the C++."""
    if nq == 0 or M == 0 or nq > GRID_MAX:
        return 0, 0
    per_query = max(1, -(-(WG_PER_CU * max(n_cu, 1)) // nq))
    chunk = max(CHUNK_FLOOR, -(-M // per_query))
    room = GRID_MAX // nq
    if -(-M // chunk) > room:
        chunk = -(-M // room)
    chunk = min(chunk, M)
    return chunk, -(-M // chunk)


def match_ref(a, b):
    """The `match` counter of a pair by set arithmetic (no walk): columns both have, masks sharing a base bit."""
    ca, cb = cols(a), cols(b)
    _, ia, ib = np.intersect1d(ca, cb, return_indices=True)
    return int(((masks(a)[ia] & masks(b)[ib] & 0xF) != 0).sum())


def _all(width, refs, qs):
    ids = np.arange(len(refs), dtype=np.uint32)
    return width, refs, qs, [ids.copy() for _ in qs]


# ---------------------------------------------------------------- the nibble table

def word_pairs():
    """Columns 2k and 2k + 1 (two nibbles of one byte): both present, and only one of them, on either side."""
    width = 40
    both, even, odd = seq([4, 5], [1, 2]), seq([4], [1]), seq([5], [2])
    other = seq([4, 5], [2, 1])                    # the neighbours' masks swapped: a nibble read from the wrong half matches
    refs, qs = [both, even, odd, other], [both, even, odd, other]
    assert match_ref(both, other) == 0 and match_ref(both, even) == 1 and match_ref(even, odd) == 0
    return _all(width, refs, qs)


def cols_7_8():
    """Columns 7 and 8: the last nibble of one 32-bit word and the first of the next."""
    width = 20
    a, b, ab = seq([7], [8]), seq([8], [8]), seq([7, 8], [8, 1])
    ba = seq([7, 8], [1, 8])
    assert 7 // 8 != 8 // 8 and match_ref(ab, ba) == 0 and match_ref(ab, a) == 1 and match_ref(ab, b) == 0
    return _all(width, [a, b, ab, ba], [a, b, ab, ba])


def _ends(width):
    def build():
        e = seq([0, width - 1], [1, 8])
        first, last = seq([0], [1]), seq([width - 1], [8])
        mid = seq([1, width - 2], [1, 8])
        assert (width % 2 == 1) == (width == 33) and (width + 7) // 8 == 5       # a partial last word either way
        assert match_ref(e, e) == 2 and match_ref(e, mid) == 0 and match_ref(e, last) == 1
        return _all(width, [e, first, last, mid], [e, first, last, mid])
    return build


def lower_neighbour():
    """A lower-case query base beside a present neighbour column: bit 4 of its mask byte, shifted with the nibble,
    would land on bit 0 (A) of the next column's nibble."""
    width = 24
    q = seq([2, 3, 7, 8], [8, 2, 4, 2], lower=[0, 2])          # lower case at 2 (beside 3) and at 7 (beside 8: next word)
    r = seq([2, 3, 7, 8], [8, 1, 4, 1])                        # A at 3 and at 8: the query has G there
    spilled = 0
    for c, m in zip(cols(q), masks(q)):
        spilled |= int(m) << (4 * int(c))                      # (the whole byte, not byte & 0xF)
    assert (spilled >> (4 * 3)) & 1 and (spilled >> (4 * 8)) & 1      # ... would make both a match with A
    assert match_ref(q, r) == 2 and compare_ref.compare_ref(q, r, 0, False)[4:] == (2, 2)
    rl = seq([2, 3], [8, 2], lower=[0, 1])                     # lower case on the candidate's side: plays no part
    assert match_ref(q, rl) == 2
    return _all(width, [r, rl], [q])


def mask_f():
    """Mask 0xF (N) on each side matches every base; on both sides too."""
    width = 16
    n4 = seq([1, 2, 3, 4], [15, 15, 15, 15])
    acgu = seq([1, 2, 3, 4], [1, 2, 4, 8])
    ugca = seq([1, 2, 3, 4], [8, 4, 2, 1])
    assert match_ref(n4, acgu) == 4 and match_ref(acgu, n4) == 4 and match_ref(n4, n4) == 4 and match_ref(acgu, ugca) == 0
    return _all(width, [n4, acgu, ugca], [n4, acgu, ugca])


def beyond_width():
    """Query bases at columns at and beyond the store's width: they meet no reference base and count for the
    denominator only."""
    width = 50
    r = seq([10, 48, 49], [1, 2, 4])
    q_at = seq([10, 49, 50], [1, 4, 1])
    q_far = seq([48, 49, 51, 60, 4000, (1 << 24) - 1], [2, 4, 1, 1, 1, 15])
    q_only = seq([50, 57], [1, 1])
    assert cols(q_at)[-1] == width and cols(q_far)[-1] >= 8 * ((width + 7) // 8) and cols(r)[-1] == width - 1
    assert (match_ref(q_at, r), match_ref(q_far, r), match_ref(q_only, r)) == (2, 2, 0)
    return _all(width, [r], [q_at, q_far, q_only])


def empties():
    """An empty candidate (match 0, identity 0) and an empty query (identity 0.f, not 0 / 0), alone and in lists."""
    width = 30
    full, empty = seq(range(0, 30, 3)), np.zeros(0, np.uint32)
    refs, qs = [full, empty, full[:3]], [full, empty, full[4:]]
    assert len(refs[1]) == 0 and len(qs[1]) == 0
    return _all(width, refs, qs)


def cand_lengths():
    """Candidates of 1, 63, 64 and 65 bases (the wave's tail loop), and of 255 .. 257 and 513 (its four-load body)."""
    width = 1100
    lens = (1, 63, 64, 65, 255, 256, 257, 513)
    refs = [seq(np.arange(n) * 2, ((1, 2, 4, 8) * (n // 4 + 1))[:n]) for n in lens]
    q = seq(np.arange(0, 1100, 2), [1, 2, 4, 1] * 137 + [1, 2])          # every fourth base differs
    assert [len(r) for r in refs] == list(lens) and len(q) == 550
    want = [match_ref(q, r) for r in refs]
    assert want[0] == 1 and all(0 < w < len(r) for w, r in zip(want[1:], refs[1:]))
    return _all(width, refs, [q, refs[5]])


def _short_world(n_refs=7, width=64):
    rng = np.random.default_rng(4242)
    refs = []
    for i in range(n_refs):
        c = np.sort(rng.choice(width, size=int(rng.integers(2, 9)), replace=False))
        refs.append(seq(c, rng.choice([1, 2, 4, 8, 15, 3], size=len(c))))
    return width, refs


def list_chunks_floor():
    """Lists of chunk - 1, chunk and chunk + 1 entries where the plan's chunk is the floor: three queries."""
    width, refs = _short_world()
    rng = np.random.default_rng(1)
    chunk, chunks = plan(3, CHUNK_FLOOR + 1)
    assert (chunk, chunks) == (CHUNK_FLOOR, 2) and all(plan(3, CHUNK_FLOOR + 1, cu)[0] == chunk for cu in (1, 64, 304))
    cand = [rng.integers(0, len(refs), size=n).astype(np.uint32) for n in (chunk - 1, chunk, chunk + 1)]
    return width, refs, [refs[0], refs[1], refs[2]], cand


def list_chunks_above_floor(n_cu=N_CU):
    """... and where the chunk is above the floor: 2 * n_cu queries want two workgroups each; the longest list has 131
    entries, so a chunk is 66.  Lists of 65, 66, 67, 131 and 132 - 1 entries, the rest short and ragged."""
    width, refs = _short_world()
    rng = np.random.default_rng(2)
    nq, M = 2 * n_cu, 131
    chunk, chunks = plan(nq, M, n_cu)
    assert chunks == 2 and chunk == 66 > CHUNK_FLOOR
    sizes = [chunk - 1, chunk, chunk + 1, M, M - 1, 0, 1] + [int(x) for x in rng.integers(0, 9, size=nq - 7)]
    cand = [rng.integers(0, len(refs), size=n).astype(np.uint32) for n in sizes]
    assert max(len(c) for c in cand) == M and len(cand) == nq
    qs = [refs[i % len(refs)] for i in range(nq)]
    return width, refs, qs, cand


def ragged():
    """Ragged list lengths across queries (a row's stride is the longest list's), an empty list first and last, and an
    id twice in one list."""
    width, refs = _short_world(9)
    sizes = (0, 1, 200, 3, 64, 0, 65, 0)
    rng = np.random.default_rng(3)
    cand = [rng.integers(0, len(refs), size=n).astype(np.uint32) for n in sizes]
    cand[3] = np.array([5, 2, 5], np.uint32)
    assert len(cand[0]) == 0 and len(cand[-1]) == 0 and (cand[3] == 5).sum() == 2
    qs = [refs[i % len(refs)] for i in range(len(sizes))]
    return width, refs, qs, cand


def ref_offsets():
    """References of more than a wave's width starting at every residue modulo 4 words (16 bytes), and short ones."""
    width = 100
    lens = [65, 66, 67, 64, 1, 2, 3, 5]
    refs = [seq(np.arange(n) + i, [1 << ((i + j) % 4) for j in range(n)]) for i, n in enumerate(lens)]
    off = np.concatenate([[0], np.cumsum(lens)])[:-1]
    assert set(int(o) % 4 for o, n in zip(off, lens) if n >= 64) == {0, 1, 2, 3}
    q = seq(range(0, 100), [1, 2, 4, 8] * 25)
    return _all(width, refs, [q, refs[2]])


CASES = dict(word_pairs=word_pairs, cols_7_8=cols_7_8, ends_odd=_ends(33), ends_even=_ends(34),
             lower_neighbour=lower_neighbour, mask_f=mask_f, beyond_width=beyond_width, empties=empties,
             cand_lengths=cand_lengths, list_chunks_floor=list_chunks_floor,
             list_chunks_above_floor=list_chunks_above_floor, ragged=ragged, ref_offsets=ref_offsets)
NAMES = sorted(CASES)


def check_wellformed(width, refs, qs, cand):
    assert len(cand) == len(qs) and width <= MAX_WIDTH
    for s in refs:
        c = cols(s)
        assert s.dtype == np.uint32 and (np.diff(c) > 0).all() and (len(c) == 0 or c[-1] < width)
    for s in qs:
        assert s.dtype == np.uint32 and (np.diff(cols(s)) > 0).all() and len(s) <= 65535
    for ids in cand:
        assert ids.dtype == np.uint32 and (len(ids) == 0 or ids.max() < len(refs))


@functools.lru_cache(maxsize=None)
def case(name):
    width, refs, qs, cand = CASES[name]()
    check_wellformed(width, refs, qs, cand)
    return width, refs, qs, cand


@functools.lru_cache(maxsize=None)
def expected(name):
    """int array [n pairs][6] of a named case by the plain walk (optimistic rule, no filter), pairs in launch order;
    distinct (query, reference) pairs are walked once."""
    width, refs, qs, cand = case(name)
    memo = {}
    rows = []
    for q, ids in zip(qs, cand):
        for i in ids:
            key = (q.tobytes(), int(i))
            if key not in memo:
                memo[key] = compare_ref.compare_ref(q, refs[int(i)], 0, False)
            rows.append(memo[key])
    return np.asarray(rows, np.int32).reshape(-1, 6)


def aligned_text(s, width):
    """A packed base list as an aligned string ('-' = no base), or None where it cannot be written as one: a base at
    or beyond `width`, or a mask that is no single upper- or lower-case letter of "AGCU" and N."""
    letters = {1: "A", 2: "G", 4: "C", 8: "U", 15: "N"}
    out = ["-"] * width
    for c, m in zip(cols(s), masks(s)):
        if c >= width or (int(m) & 0xF) not in letters:
            return None
        ch = letters[int(m) & 0xF]
        out[int(c)] = ch.lower() if int(m) & cc.LC else ch
    return "".join(out)


# ---------------------------------------------------------------- the leave-out world

LEAVEOUT_FF = {"fs-leave-query-out": 1, "fs-msc-max": 0.9, "fs-min-len": 100, "fs-full-len": 250}     # the stages' names
LO_MSC_MAX, LO_MIN_LEN, LO_FULL_LEN, LO_FS_MIN, LO_FS_MAX, LO_FS_MSC = np.float32(0.9), 100, 250, 40, 40, 0.7
LO_N_REFS, LO_WIDTH = 900, 3000


@functools.lru_cache(maxsize=None)
def leaveout_world():
    """900 references of about 300 bases in two clades a quarter of their columns apart, each within a few percent of
    its own ancestor: identity above 0.9 inside a clade, far below across.  Returns (refs, dense matrix of mask nibbles
    [n, width], clade of every reference).  Clade 0 is the larger one."""
    from sina_amd import synth
    refs = synth.make_refs(LO_N_REFS, length=300, width=LO_WIDTH, seed=9701, n_clades=2, clade_div=0.25, sub_lo=0.004,
                           sub_hi=0.02, del_rate=0.004, ins_rate=0.002, long_del_prob=0.0)
    dense = np.zeros((refs.n, LO_WIDTH), np.uint8)
    for i in range(refs.n):
        s = refs.seq(i)
        dense[i, cols(s)] = masks(s) & 0xF
    near0 = identities(dense, refs.seq(0)) > LO_MSC_MAX
    clade = np.where(near0, 0, 1)
    if (clade == 0).sum() < (clade == 1).sum():
        clade = 1 - clade
    return refs, dense, clade


def identities(dense, q):
    """float32 identity of a query (strictly ascending columns) against every reference of the dense matrix: matches
    over the query's base count -- by table look-up, no walk."""
    c, m = cols(q), masks(q) & 0xF
    inside = c < dense.shape[1]
    match = ((dense[:, c[inside]] & m[inside].astype(np.uint8)) != 0).sum(axis=1)
    return match.astype(np.float32) / np.float32(max(len(q), 1))


def walk_identity(q, r):
    """The host walk's value: match / (match + mismatch + only_a + only_a_overhang), 0 for an empty side."""
    oa_over, _, oa, _, match, mismatch = compare_ref.compare_ref(q, r, 0, False)
    base = match + mismatch + oa + oa_over
    return np.float32(match) / np.float32(base) if base else np.float32(0)


@functools.lru_cache(maxsize=None)
def leaveout_queries():
    """(names, packed base lists, kinds).  Six members of the dense clade under their own names; one more member with
    one base moved onto its left neighbour's column (two equal columns: not strictly ascending, the host walk's); and a
    member's bases once more, every one a column to the right, under a name of its own (equal bases at other columns:
    next to nothing matches, so it may not share the member's result)."""
    refs, dense, clade = leaveout_world()
    members = np.flatnonzero(clade == 0)
    picks = [int(members[i]) for i in (0, 7, 50, 123, 300, len(members) - 1)]
    names = ["ref%d" % i for i in picks]
    seqs = [refs.seq(i).copy() for i in picks]
    kinds = ["member"] * len(picks)
    dup = refs.seq(int(members[11])).copy()
    dup[40] = (dup[40] & np.uint32(0xFF000000)) | (dup[39] & np.uint32(0xFFFFFF))
    assert cols(dup)[40] == cols(dup)[39] and not (np.diff(cols(dup)) > 0).all()
    names.append("ref%d" % int(members[11]))
    seqs.append(dup)
    kinds.append("equal_columns")
    shifted = refs.seq(picks[1]) + np.uint32(1)
    assert (masks(shifted) == masks(seqs[1])).all() and (cols(shifted) == cols(seqs[1]) + 1).all()
    assert cols(shifted)[-1] < LO_WIDTH
    names.append("shifted")
    seqs.append(shifted)
    kinds.append("shifted")
    return names, seqs, kinds


def leaveout_cascade(lists, sizes, ident, self_id, n_refs):
    """famfinder's filter cascade with the leave-out options, in plain Python: lists(M) -> (ids, scores) of the top M,
    ident[id] the walk's identity, self_id the reference with the query's name (or -1).  Returns the family's ids."""
    max_results = LO_FS_MAX + 1
    while True:
        ids, scores = lists(min(max_results, n_refs))
        have = have_full = 0
        kept = []
        for i, sc in zip(ids, scores):
            i = int(i)
            full = sizes[i] >= LO_FULL_LEN
            if sizes[i] < LO_MIN_LEN or i == self_id or ident[i] > LO_MSC_MAX:
                continue
            min_reached, max_reached, score_good = have >= LO_FS_MIN, have >= LO_FS_MAX, sc < LO_FS_MSC
            adds_to_full = have_full < 1 and full
            if min_reached and (max_reached or not score_good) and not adds_to_full:
                continue
            have += 1
            have_full += int(full)
            kept.append(i)
        enough = not (have < LO_FS_MAX or have_full < 1)
        if enough or max_results >= n_refs:
            return kept
        max_results *= 10
