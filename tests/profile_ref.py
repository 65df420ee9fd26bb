"""The family profile and what the DP kernel is handed of it, restated plainly (test infrastructure).

Pure Python / numpy: nothing here calls the oracle library or the product.  `build` is pseq::pseq (reference
src/pseq.cpp:44-115) as a walk over the occupied columns, column 0 first, with a gap flag per member; `table` is
base_profile::comp (src/pseq.h:100-113) of every node with the fifteen query masks, in float32 and in comp's order;
`chain_words` is the chain as sina_amd/csrc/profile_build.hip step 2 leaves it for the DP kernel, by way of
graph_ref.dp_words.

A member is a packed array: alignment column | 5-bit IUPAC mask << 24 per base, columns strictly ascending.  A base
whose mask has none of the four base bits (A 1, G 2, C 4, T/U 8) is consumed and changes nothing."""
import numpy as np

from tests import graph_ref as gr

NO_SUCCESSOR = gr.NO_SUCCESSOR
POINTS = 12          # per member and column, split evenly over the bases of its code
F32 = np.float32


def order_of(mask):
    return bin(int(mask) & 15).count("1")


def build(fam, width):
    """The profile of the members `fam` in an alignment of `width` columns.  Returns dict(n, pos [n] uint32,
    points [n, 6] int64: A, G, C, T/U, members whose gap opens * 12, members whose gap extends * 12)."""
    assert width > 0
    present = []   # per member: column -> mask
    occupied = {0}
    for ab in fam:
        ab = np.asarray(ab, np.uint32)
        col = (ab & 0xFFFFFF).astype(np.int64)
        assert (np.diff(col) > 0).all() and (len(col) == 0 or col[-1] < width), "a member's columns ascend, below the width"
        present.append({int(c): int(m) for c, m in zip(col, (ab >> 24) & 0x1F)})
        occupied.update(present[-1])
    pos = sorted(occupied)
    in_gap = [True] * len(fam)   # (a member's leading gap counts as extended)
    points = np.zeros((len(pos), 6), np.int64)
    for node, column in enumerate(pos):
        row = points[node]
        for j, bases in enumerate(present):
            mask = bases.get(column)
            if mask is None:
                row[5 if in_gap[j] else 4] += POINTS
                in_gap[j] = True
            elif order_of(mask):
                for bit in range(4):
                    if mask >> bit & 1:
                        row[bit] += POINTS // order_of(mask)
                in_gap[j] = False
    return dict(n=len(pos), pos=np.array(pos, np.uint32), points=points)


def shares(points):
    """base_profile(a, g, c, t, open, extend), pseq.h:54-63: every count as a float over the int sum as a float."""
    points = np.asarray(points, np.int64).reshape(-1, 6)
    with np.errstate(invalid="ignore", divide="ignore"):
        return points.astype(F32) / points.sum(axis=1).astype(F32)[:, None]


def shares_of_mask(mask):
    """base_profile(const base_iupac&), pseq.h:65-86"""
    out = np.zeros(6, F32)
    k = order_of(mask)
    if k:
        for bit in range(4):
            if mask >> bit & 1:
                out[bit] = F32(1) / F32(k)
    return out


def comp(a, b, match, mismatch, gap, gap_ext):
    """base_profile::comp of the columns a [n, 6] with the profile b [6]: sixteen products i-outer j-inner, then the two
    gap terms; every operation rounds to float32 on its own."""
    match, mismatch, gap, gap_ext = F32(match), F32(mismatch), F32(gap), F32(gap_ext)
    a = np.asarray(a, F32).reshape(-1, 6)
    res = np.zeros(len(a), F32)
    for i in range(4):
        for j in range(4):
            res = res + ((match if i == j else mismatch) * a[:, i]) * b[j]
    return (res + gap * a[:, 4]) + gap_ext * a[:, 5]


def table(points, match, mismatch, gap, gap_ext):
    """([n, 16] float32 match terms, entry 0 +inf; the 16 self terms, entry 0 0)."""
    col = shares(points)
    tab = np.full((len(col), 16), np.inf, F32)
    own = np.zeros(16, F32)
    for m in range(1, 16):
        b = shares_of_mask(m)
        tab[:, m] = comp(col, b, match, mismatch, gap, gap_ext)
        own[m] = comp(b, b, match, mismatch, gap, gap_ext)[0]
    return tab, own


def chain_graph(pos):
    """The chain as a DAG for graph_ref.dp_words / util's graph batches: mask 0, node weight 0, every node's one
    predecessor the node before it."""
    n = len(pos)
    pred_off = np.zeros(n + 1, np.uint32)
    pred_off[1:] = np.arange(n)
    sink = np.zeros(n, np.uint8)
    sink[n - 1] = 1
    return dict(n=n, pos=np.asarray(pos, np.uint32), mask=np.zeros(n, np.uint8), weight=np.zeros(n, F32), pred_off=pred_off,
                pred=np.arange(max(n, 1) - 1, dtype=np.uint32),
                succ_minpos=np.append(np.asarray(pos, np.uint32)[1:], np.uint32(NO_SUCCESSOR)), sink=sink,
                chain=np.zeros(0, np.uint16))


def chain_words(pos, ring=4):
    """What the DP kernel is handed: dict(rec [n, 4]: index of the node's predecessor entry, node weight (0.f), z, where
    the finished row is kept; succ_min [n]; pred [n - 1]; sizes: nodes, edges, spill rows, status, first sink, 0)."""
    g = chain_graph(pos)
    w = gr.dp_words(g, ring)
    n = g["n"]
    rec = np.zeros((n, 4), np.uint32)
    rec[1:, 0] = np.arange(n - 1)
    rec[:, 2], rec[:, 3] = w["z"], w["store"]
    return dict(rec=rec, succ_min=g["succ_minpos"], pred=w["pred"],
                sizes=np.array([n, len(g["pred"]), w["n_spill"], 0, w["first_sink"], 0], np.uint32))
