"""The family DAG and what the DP kernel is handed of it, restated plainly (test infrastructure).

Pure Python / numpy: nothing here calls the oracle library or the product.  `build` is mseq::mseq + sort + reduce_edges
(reference src/mseq.cpp:47-118) as a loop over the columns; `dp_words` is the row records, predecessor
entries and size words of sina_amd/csrc/common.h as dp_plan.h's prep_range and graph_build.hip's steps 6-8 make them.

A member is a packed array: alignment column | 5-bit IUPAC mask << 24 per base, columns strictly ascending."""
import numpy as np

from tests import util

# sina_amd/csrc/common.h
REC_SINK = 1 << 16
REC_FENCE = 1 << 17
REC_DIST_SHIFT = 18
REC_DIST_FAR = 63
ROW_NONE = 0xFFFFFFFF
ROW_SPILLED = 0x80000000
PRED_SPILLED = 0x80000000
MAX_SPILL_ROWS = 32768
FAR_LDS = 192
NO_SUCCESSOR = 1000000  # mesh.h:480


def char_key(mask):
    """What mseq keys a column's nodes by: the base's character (mseq.cpp:92-96).  bmask_to_iupac_rna_char gives every
    5-bit mask a character of its own, except that 0 and 16 (no base bit, upper / lower case) are both '.'."""
    return 0 if mask == 16 else mask


def node_weight(count, n_members, fs_weight):
    """mseq.cpp:113, `1.0/(weight+1) + weight * (node->weight/num_seqs)` with weight and node->weight floats: the
    reciprocal in double of a float sum, the product in float, their sum in double, stored as float."""
    w = np.float32(fs_weight)
    return np.float32(1.0 / float(w + np.float32(1)) + float(w * (np.float32(count) / np.float32(n_members))))


def build(fam, fs_weight=1.0):
    """The DAG of the members `fam` (packed arrays, family order).  Returns dict(n, pos, mask, weight (float32),
    pred_off, pred, succ_minpos, sink (uint8 per node), chain (the node of every base of member 0))."""
    F = len(fam)
    bases = []  # (column, member, mask, index in the member)
    for j, ab in enumerate(fam):
        ab = np.asarray(ab, np.uint32)
        col = (ab & 0xFFFFFF).astype(np.int64)
        assert (np.diff(col) > 0).all(), "a member's columns ascend"
        bases += [(int(c), j, int(m), i) for i, (c, m) in enumerate(zip(col, (ab >> 24) & 0x1F))]
    bases.sort(key=lambda b: (b[0], b[1]))  # column by column, the members of a column in family order
    pos, mask, count, preds = [], [], [], []
    last = [-1] * F
    chain = [0] * (len(fam[0]) if F else 0)
    col_nodes, col_now = {}, -1
    for c, j, m, i in bases:
        if c != col_now:
            col_nodes, col_now = {}, c
        k = char_key(m)
        if k not in col_nodes:  # the node keeps the base of the first member to show the character
            col_nodes[k] = len(pos)
            pos.append(c), mask.append(m), count.append(0), preds.append(set())
        node = col_nodes[k]
        count[node] += 1
        if last[j] >= 0:
            preds[node].add(last[j])
        last[j] = node
        if j == 0:
            chain[i] = node
    n = len(pos)
    pred_off = np.zeros(n + 1, np.uint32)
    pred_off[1:] = np.cumsum([len(p) for p in preds])
    pred = np.array([p for ps in preds for p in sorted(ps)], np.uint32)
    succ_min = np.full(n, NO_SUCCESSOR, np.uint32)
    sink = np.ones(n, np.uint8)
    for node in range(n):
        for p in preds[node]:
            succ_min[p] = min(succ_min[p], pos[node])
            sink[p] = 0
    return dict(n=n, pos=np.array(pos, np.uint32), mask=np.array(mask, np.uint8),
                weight=np.array([node_weight(k, F, fs_weight) for k in count], np.float32), pred_off=pred_off, pred=pred,
                succ_minpos=succ_min, sink=sink, chain=np.array(chain, np.uint16))


def last_successor(g):
    """Per node the id of its last successor (0: none -- a successor's id is never 0)."""
    last = np.zeros(g["n"], np.int64)
    for node in range(g["n"]):
        for p in g["pred"][g["pred_off"][node]:g["pred_off"][node + 1]]:
            last[p] = max(last[p], node)
    return last


def dp_words(g, ring, chain_len=None):
    """What mesh_dp_kernel reads of the DAG `g` (from `build`) on a ring of `ring` LDS row slots:
      store   where each finished row is kept (rec.w; util.row_store_model)
      z       rec.z: predecessors | mask << 8 | sink << 16 | fence << 17 | min(dist, 63) << 18 | (first spilled + 1) << 24
      pred    an entry per edge, id | (slot or spill row & 0x7FFF) << 16 | spilled << 31
      n, n_spill, first_sink, chain_len   the size words."""
    n = g["n"]
    store = util.row_store_model(g["pred_off"], g["pred"], ring, far_lds=FAR_LDS)
    last = last_successor(g)
    z = np.zeros(n, np.uint32)
    pw = np.zeros(len(g["pred"]), np.uint32)
    for m in range(n):
        lo, hi = int(g["pred_off"][m]), int(g["pred_off"][m + 1])
        first_spilled, dist = 0, (0 if hi > lo else REC_DIST_FAR)
        for e in range(lo, hi):
            p = int(g["pred"][e])
            w = int(store[p])
            if w == ROW_NONE:  # (handed over in registers: the entry's slot is not read)
                w = 0
            spilled = (w & ROW_SPILLED) != 0
            if spilled and first_spilled == 0:
                first_spilled = e - lo + 1
            dist = max(dist, m - p)
            pw[e] = p | ((w & 0x7FFF) << 16) | (PRED_SPILLED if spilled else 0)
        word = (hi - lo) | (int(g["mask"][m]) << 8) | (first_spilled << 24) | (min(dist, REC_DIST_FAR) << REC_DIST_SHIFT)
        if last[m] == 0:
            word |= REC_SINK
        if last[m] > m and last[m] - m > FAR_LDS:
            word |= REC_FENCE
        z[m] = word
    spilled_rows = (store != ROW_NONE) & ((store & ROW_SPILLED) != 0)
    sinks = np.flatnonzero(g["sink"])
    return dict(store=store, z=z, pred=pw, n=n, n_spill=int(spilled_rows.sum()),
                first_sink=int(sinks[0]) if len(sinks) else ROW_NONE,
                chain_len=len(g["chain"]) if chain_len is None else chain_len)
