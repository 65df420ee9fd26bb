"""famfinder's --turn on a batch as a plain model (test infrastructure): what csrc/turn.hip's header comment says the
orient and pick kernels compute around the k-mer search, with no notion of how they go about it.  The variants are made
with numpy, each is scored with kmer_ref.scores, top-1 and top-`max` are kmer_ref.topk's, and the pick is a four-step
loop.  tests/test_turn_cpu.py pins it to the oracle's so_turn_check, so_cseq_reverse and so_cseq_complement;
tests/turn_cases.py takes every expected result from here."""
import numpy as np

from tests import kmer_ref

ORDER = {False: (0, 3), True: (0, 3, 1, 2)}      # the orientations tried, in the order they are tried
NAMES = ("none", "reversed", "complemented", "reversed and complemented")


def complement(mask):
    """base_iupac::complement on mask bytes: bits 1 <-> 8 and 2 <-> 4, bit 16 (lower case) kept."""
    d = np.asarray(mask, np.uint8)
    return (((d & 2) << 1) | ((d & 4) >> 1) | ((d & 1) << 3) | ((d & 8) >> 3) | (d & 16)).astype(np.uint8)


def variant(mask, o):
    """The query in orientation o = (bit 0: reversed) | (bit 1: complemented)."""
    v = np.asarray(mask, np.uint8)
    if o & 1:
        v = v[::-1]
    if o & 2:
        v = complement(v)
    return np.ascontiguousarray(v)


def pick(score4):
    """Over o = 0, 1, 2, 3 the first strictly largest score above 0, else 0."""
    best, top = 0, 0.0
    for o in range(4):
        if score4[o] > top:
            top, best = score4[o], o
    return best


def rows_of(csr_off, csr_ids, n_refs, qmask, k, fast):
    """The score row of each of the four orientations of one query: {o: kmer_ref.scores of the variant}."""
    return {o: kmer_ref.scores(csr_off, csr_ids, n_refs, variant(qmask, o), k, fast) for o in range(4)}


def orient(rows, all_four, mx):
    """One query from its orientations' score rows: dict(turn, top1 float32 [4] by orientation (untried: 0), ids,
    scores: the top-`mx` of the chosen orientation)."""
    top1 = np.zeros(4, np.float32)
    for o in ORDER[bool(all_four)]:
        _, sc = kmer_ref.topk(rows[o], 1)
        top1[o] = sc[0] if len(sc) else 0
    turn = pick(top1)
    ids, sc = kmer_ref.topk(rows[turn], mx)
    return dict(turn=turn, top1=top1, ids=ids, scores=sc)
