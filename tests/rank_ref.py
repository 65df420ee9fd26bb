"""The search stage's scoring and ranking, restated plainly from the six counters of a pair (only_a_overhang,
only_b_overhang, only_a, only_b, match, mismatch): the nine cover rules' integer denominators, the score as one numpy
float32 division, and the order "score descending, then name descending".  tests/test_rank_cpu.py pins the score to the
host stage's comparator and the order to what search_filter returns; tests/test_gpu_rank.py holds the device's rows
against it.  No device, no library."""
import numpy as np

COVERS = ("abs", "query", "target", "overlap", "all", "average", "min", "max", "nogap")   # CMP_COVER_TYPE's order


def denom(counts, cover):
    oa_over, ob_over, oa, ob, match, mismatch = (int(x) for x in counts)
    paired = match + mismatch
    a_alone, b_alone = oa + oa_over, ob + ob_over
    cover = COVERS[cover] if not isinstance(cover, str) else cover
    if cover == "abs":
        return 1
    if cover == "query":
        return paired + a_alone
    if cover == "target":
        return paired + b_alone
    if cover == "overlap":
        return paired + oa + ob
    if cover == "all":
        return paired + oa + ob + oa_over + ob_over
    if cover == "average":
        return paired + (oa + ob + oa_over + ob_over) // 2     # (a sum of counts: never negative, so // is C's /)
    if cover == "min":
        return paired + min(a_alone, b_alone)
    if cover == "max":
        return paired + max(a_alone, b_alone)
    assert cover == "nogap"
    return paired


def score(counts, cover):
    """float32, or None where the host divides 0 by 0."""
    d = denom(counts, cover)
    if d == 0:
        assert int(counts[4]) == 0
        return None
    return np.float32(int(counts[4])) / np.float32(d)


def bits(x):
    return int(np.float32(x).view(np.uint32))


def rank_query(rows, ids, name_rank, cover, n_best):
    """One query: rows[i] the counters of candidate ids[i].  Gives (ids, score bits, flag) of the n_best best; a candidate
    without a score is left out and sets the flag.  An id listed twice competes twice."""
    keyed = []
    flag = 0
    for r, i in zip(rows, ids):
        s = score(r, cover)
        if s is None:
            flag = 1
            continue
        assert s >= 0 and np.isfinite(s)
        keyed.append((bits(s), int(name_rank[int(i)]), int(i)))
    keyed.sort(reverse=True)           # non-negative floats order like their bits; then the name, descending
    keyed = keyed[:n_best]
    return [k[2] for k in keyed], [k[0] for k in keyed], flag


def rank_call(rows, cand, name_rank, cover, n_best):
    """A call: rows the counters of all pairs in launch order, cand the id list per query.  Gives ids [nq, n_best],
    score bits [nq, n_best] (unused entries 0), n [nq], flag [nq]."""
    nq = len(cand)
    ids = np.zeros((nq, n_best), np.uint32)
    sb = np.zeros((nq, n_best), np.uint32)
    n = np.zeros(nq, np.uint32)
    flag = np.zeros(nq, np.uint32)
    at = 0
    for q, c in enumerate(cand):
        i, s, f = rank_query(rows[at:at + len(c)], c, name_rank, cover, n_best)
        at += len(c)
        ids[q, :len(i)] = i
        sb[q, :len(s)] = s
        n[q] = len(i)
        flag[q] = f
    assert at == len(rows)
    return ids, sb, n, flag


def name_order(names):
    """rank[id] = position of names[id] in ascending byte-wise order (what sina_hip_upload_name_order takes)."""
    enc = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
    assert len(set(enc)) == len(enc)
    order = sorted(range(len(enc)), key=lambda i: enc[i])
    rank = np.zeros(len(enc), np.uint32)
    rank[order] = np.arange(len(enc), dtype=np.uint32)
    return rank
