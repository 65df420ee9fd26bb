"""--show-dist restated plainly (the reference's Log::printer::show_dist, src/log.cpp:279-325, and the host stage's
show_dist_report): from an input alignment `orig`, a finished alignment `aligned` and a list of relatives to the
twenty-word row sina_hip_show_dist returns, and from a row to the report's floats and text.

The counters are tests/compare_ref.py's lock-step walk; the closest relative is the last of the relatives sorted by
(float32 score, name), the score being match / (match + mismatch + only_a + only_a_overhang) -- CMP_COVER_QUERY -- as
one numpy float32 division.  tests/test_showdist_cpu.py pins this to the oracle and to the host stage;
tests/test_gpu_showdist.py holds the device's rows against it.  No device, no library."""
import numpy as np

from tests import compare_ref

EXACT, OPTIMISTIC = 2, 0
ROW_WORDS = 20
SELF, BEFORE, AFTER, CLOSEST, FLAGS = 0, 6, 12, 18, 19
NONE = 0xFFFFFFFF
FLAG_NAN, FLAG_COMPUTED = 1, 2


def names_of(n):
    """The names a store built from packed references gives them."""
    return ["ref%d" % i for i in range(n)]


def denom(counts):
    oa_over, ob_over, oa, ob, match, mismatch = (int(x) for x in counts)
    return match + mismatch + oa + oa_over


def score(counts):
    """cseq_comparator::score under CMP_COVER_QUERY: float32; NaN where the host divides 0 by 0."""
    d = denom(counts)
    if d == 0:
        assert int(counts[4]) == 0
        return np.float32(np.nan)
    return np.float32(int(counts[4])) / np.float32(d)


def row(orig, aligned, refs, ids, names):
    """The row of one query: uint32 [20]."""
    out = np.zeros(ROW_WORDS, np.uint32)
    out[SELF:SELF + 6] = compare_ref.compare_ref(orig, aligned, EXACT, False)
    scored, flags = [], FLAG_COMPUTED
    for i in ids:
        c = compare_ref.compare_ref(orig, refs[int(i)], OPTIMISTIC, False)
        if denom(c) == 0:
            flags |= FLAG_NAN                       # the host's NaN: left out, the caller walks this query itself
            continue
        name = names[int(i)]
        scored.append((float(score(c)), name.encode() if isinstance(name, str) else bytes(name), int(i), c))
    out[CLOSEST] = NONE
    if scored:
        scored.sort(key=lambda s: (s[0], s[1]))     # std::sort by result_item::operator<: the score, then the name
        _, _, closest, before = scored[-1]
        out[BEFORE:BEFORE + 6] = before
        out[AFTER:AFTER + 6] = compare_ref.compare_ref(aligned, refs[closest], OPTIMISTIC, False)
        out[CLOSEST] = closest
    out[FLAGS] = flags
    return out


def rows(case):
    """uint32 [nq, 20] of a case of tests/showdist_cases.py."""
    out = [row(o, a, case["refs"], ids, case["names"]) for o, a, ids in zip(case["orig"], case["aligned"], case["lists"])]
    return np.asarray(out, np.uint32).reshape(-1, ROW_WORDS)


def report(r, list_len):
    """What show_dist_report makes of a row: dict(text, has_sps, has_closest, sps, idty, cpm, closest); floats float32.
    (The widths are equal here: the "Cannot show dist" line has no row.)"""
    sps = score(r[SELF:SELF + 6])
    out = dict(text="orig_idty: %.6f\n" % sps, has_sps=True, has_closest=False, sps=sps, idty=np.float32(0), cpm=np.float32(0),
               closest=NONE)
    if list_len == 0:
        out["text"] += "reference / search result empty?\n"
        return out
    assert int(r[CLOSEST]) != NONE                  # (a row without a closest relative of a list with members is flagged)
    before, after = score(r[BEFORE:BEFORE + 6]), score(r[AFTER:AFTER + 6])
    cpm = np.float32(before - after)
    out["text"] += "orig_closest_idty: %.6f\nclosest_idty: %.6f\ncpm: %.6f\n" % (before, after, cpm)
    out.update(has_closest=True, idty=before, cpm=cpm, closest=int(r[CLOSEST]))
    return out
