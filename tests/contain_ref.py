"""The plain restatement of the aligner's exact-relative test (boost::icontains / ifind_first at src/align.cpp:329-388;
sina_hip_find_bases on the device): bytes.find over the `mask & 0xF` strings of the two sequences.  A mask byte is a
base's four base bits (A 1, G 2, C 4, T/U 8, their unions the ambiguity codes) with the case in bit 4; the case is
ignored, the codes are compared for equality."""
import numpy as np

NONE = 0xFFFFFFFF


def codes(mask):
    """The string the search runs over: one byte per base, its four base bits."""
    return (np.asarray(mask, np.uint8) & 0xF).tobytes()


def find(query, ref):
    """std::string::find's answer: the lowest start of the query's codes in the reference's, NONE without one (a query of
    more bases than the reference has included).  The query has a base at least."""
    assert len(query) >= 1
    at = codes(ref).find(codes(query))
    return NONE if at < 0 else at


def expected(queries, refs, lists):
    """One word per candidate, the queries' candidates one after the other (sina_hip_find_bases' out_at)."""
    return np.array([find(q, refs[int(i)]) for q, ids in zip(queries, lists) for i in ids], np.uint32)


def is_query_itself(at, n_query, n_ref):
    """What the host derives from an answer: the reference's bases ARE the query's (boost::iequals)."""
    return at == 0 and n_query == n_ref
