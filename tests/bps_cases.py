"""Hand-built cases of the helix base-pair score: name -> (q_ab, q_off, pairs), the packed words of a batch of
finished aligned sequences (column | mask << 24; mask: A 1, G 2, C 4, U 8, lower case 16), their offsets -- which
need not start at 0 -- and a helix map (pairs[i] = partner column, 0 = unpaired).  Plus seeded random batches."""
import numpy as np

_MASK = {c: i for i, c in enumerate(".AGRCMSVUWKDYHBN")}
_MASK["T"] = 8


def word(col, ch):
    m = _MASK[ch.upper()] | (16 if ch.islower() else 0)
    return col | (m << 24)


def words_of(text):
    """An aligned string ('-' and '.' are gaps) as packed words."""
    return np.array([word(i, ch) for i, ch in enumerate(text) if ch not in "-."], np.uint32)


def batch(seqs, lead=0, trail=0):
    """(q_ab, q_off) of the sequences, with `lead` / `trail` foreign words around them (q_off[0] == lead)."""
    seqs = [np.asarray(s, np.uint32) for s in seqs]
    junk = lambda n: np.full(n, word(3, "G"), np.uint32)
    q_ab = np.concatenate([junk(lead)] + seqs + [junk(trail)]) if seqs or lead or trail else np.zeros(0, np.uint32)
    q_off = np.zeros(len(seqs) + 1, np.uint64)
    q_off[0] = lead
    for i, s in enumerate(seqs):
        q_off[i + 1] = q_off[i] + len(s)
    return np.ascontiguousarray(q_ab, np.uint32), q_off


def sym(width, pairs_list):
    m = np.zeros(width, np.uint32)
    for a, b in pairs_list:
        m[a] = b
        m[b] = a
    return m


TABLE_SEQS = ["-GGCA--UGCU-", "-GGCA--U-CU-", "-gGNA--UGCC-", "------------"]
# num, AG, AU, CG, GG, GU, attribute
TABLE_EXPECT = [(8, 0, 2, 4, 0, 2, 125), (8, 0, 2, 2, 0, 2, 87), (8, 0, 2, 2, 0, 0, 65), (0, 0, 0, 0, 0, 0, 0)]
TABLE_MAP = sym(12, [(1, 10), (2, 9), (3, 8), (4, 7)])


def _rand_seq(rng, n_bases, width, fancy=True):
    cols = np.sort(rng.choice(width, size=n_bases, replace=False)).astype(np.uint32)
    masks = rng.choice([1, 2, 4, 8], size=n_bases).astype(np.uint32)
    if fancy and n_bases:
        odd = rng.random(n_bases) < 0.15
        masks[odd] = rng.integers(0, 32, size=int(odd.sum()))  # ambiguity codes, lower case, no mask bits
    return cols | (masks << 24)


def _nested_map(rng, width, n_pairs):
    """A symmetric map of n_pairs nested pairs over random columns 1 .. width - 1."""
    cols = np.sort(rng.choice(np.arange(1, width), size=2 * n_pairs, replace=False))
    return sym(width, [(int(cols[k]), int(cols[2 * n_pairs - 1 - k])) for k in range(n_pairs)])


def _entries_map(rng, width, n_entries):
    """An asymmetric map with exactly n_entries paired columns."""
    m = np.zeros(width, np.uint32)
    at = rng.choice(width, size=n_entries, replace=False)
    m[at] = rng.integers(1, width, size=n_entries)
    return m


def _build():
    rng = np.random.default_rng(20240611)
    c = {}
    c["table"] = batch([words_of(s) for s in TABLE_SEQS]) + (TABLE_MAP,)
    c["empty_sequence"] = batch([np.zeros(0, np.uint32)]) + (TABLE_MAP,)
    c["empty_between"] = batch([np.zeros(0, np.uint32), words_of(TABLE_SEQS[0]), np.zeros(0, np.uint32)]) + (TABLE_MAP,)
    c["one_base"] = batch([words_of("--G---------"), words_of("---------C--")]) + (TABLE_MAP,)
    seqs200 = [_rand_seq(rng, n, 200) for n in (0, 1, 2, 63, 64, 65, 150, 200)]
    for n_ent in (1, 63, 64, 65):
        c["map_%d_entries" % n_ent] = batch(seqs200) + (_entries_map(rng, 200, n_ent),)
    # partners outside the sequence: before its first base, after its last, beyond the map's length, beyond 24 bits
    s = words_of("-----ACGUACGU-------")
    m = np.zeros(12, np.uint32)
    m[5], m[6], m[7], m[8], m[9], m[1], m[2] = 2, 15, 400, 1 << 24, 0xFFFFFFFF, 5, (1 << 24) + 6
    c["partner_outside"] = batch([s]) + (m,)
    # the first and the last word as partners, and as the paired columns themselves
    m = np.zeros(20, np.uint32)
    m[1], m[2], m[5], m[12] = 5, 12, 12, 5
    c["first_last_word"] = batch([s, words_of("-----G------C-------")]) + (m,)
    m = TABLE_MAP.copy()
    m[0] = 9
    c["pairs0_set"] = batch([words_of("AGGCA--UGCU-"), words_of(TABLE_SEQS[0])]) + (m,)
    m = np.zeros(12, np.uint32)
    m[2], m[3], m[5], m[11] = 2, 3, 5, 11
    c["self_partner"] = batch([words_of(t) for t in TABLE_SEQS]) + (m,)
    m = np.zeros(12, np.uint32)
    m[1], m[2], m[3] = 10, 8, 8                       # no way back; two columns share one partner
    c["asymmetric"] = batch([words_of(t) for t in TABLE_SEQS]) + (m,)
    # all sixteen ordered pairs of A C G U: columns 2k + 1 -> 2k + 2, one way
    text, m = "-", np.zeros(34, np.uint32)
    for k, (x, y) in enumerate((x, y) for x in "ACGU" for y in "ACGU"):
        text += x + y
        m[2 * k + 1] = 2 * k + 2
    c["all_base_pairs"] = batch([words_of(text + "-")]) + (m,)
    c["all_base_pairs_both_ways"] = batch([words_of(text + "-")]) + (sym(34, [(2 * k + 1, 2 * k + 2) for k in range(16)]),)
    # lower case, ambiguity codes, a word without mask bits (upper and lower case)
    raw = np.array([1 | (0 << 24), 2 | (16 << 24), 3 | (2 << 24), 4 | (18 << 24), 7 | (8 << 24), 8 | (15 << 24), 9 | (4 << 24),
                    10 | (1 << 24)], np.uint32)
    c["lower_ambiguous_mask0"] = batch([raw, words_of("-aGgR--uKCY-"), words_of("-NNNN--NNNN-")]) + (TABLE_MAP,)
    # equal neighbouring columns: the first of them is the one that is read
    raw = np.array([1 | (2 << 24), 1 | (1 << 24), 4 | (1 << 24), 4 | (1 << 24), 4 | (4 << 24), 7 | (8 << 24), 10 | (4 << 24),
                    10 | (8 << 24)], np.uint32)
    c["equal_columns"] = batch([raw]) + (TABLE_MAP,)
    long_seq = (np.arange(10241, dtype=np.uint32) * 2 + 1) | (rng.choice([1, 2, 4, 8], size=10241).astype(np.uint32) << 24)
    c["long_10241"] = batch([long_seq, long_seq[:10240], long_seq[5:77]]) + (_nested_map(rng, 20500, 450),)
    c["offset_batch"] = batch([_rand_seq(rng, n, 300) for n in (40, 0, 299, 7)], lead=17, trail=5) + (_nested_map(rng, 300, 60),)
    return c


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


NAMES = ["table", "empty_sequence", "empty_between", "one_base", "map_1_entries", "map_63_entries", "map_64_entries",
         "map_65_entries", "partner_outside", "first_last_word", "pairs0_set", "self_partner", "asymmetric", "all_base_pairs",
         "all_base_pairs_both_ways", "lower_ambiguous_mask0", "equal_columns", "long_10241", "offset_batch"]


def case(name):
    return cases()[name]


def sequences(q_ab, q_off):
    return [q_ab[int(q_off[i]):int(q_off[i + 1])] for i in range(len(q_off) - 1)]


def random_batch(seed, n=200, width=1000, symmetric=True):
    """n sequences of 0..300 bases at `width`, and a symmetric nested map or an asymmetric one whose partners may lie
    beyond the width."""
    rng = np.random.default_rng(9000 + 2 * seed + (1 if symmetric else 0))
    seqs = [_rand_seq(rng, int(rng.integers(0, 301)), width) for _ in range(n)]
    if symmetric:
        m = _nested_map(rng, width, int(rng.integers(1, 200)))
    else:
        m = np.zeros(int(rng.integers(1, width + 1)), np.uint32)
        k = int(rng.integers(1, len(m) + 1))
        at = rng.choice(len(m), size=min(k, 400), replace=False)
        m[at] = rng.integers(1, width + 50, size=len(at))
    return batch(seqs) + (m,)
