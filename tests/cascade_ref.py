"""Famfinder's filter cascade (src/famfinder.cpp:497-612; match_pass of sina_amd/csrc/host/famfinder.cpp) as a plain
loop, for every option the device cascade takes: what tests/test_cascade_cpu.py pins to the oracle's famfinder and what
tests/test_gpu_cascade.py and tests/test_gpu_cascade_stage.py compare the kernel's rows with.  CPU work only."""
import collections

import numpy as np

Rule = collections.namedtuple("Rule", "fs_min fs_max fs_req_full fs_full_len fs_min_len fs_cover_gene fs_msc fs_msc_max",
                              defaults=(40, 40, 1, 1400, 150, 0, 0.7, 2.0))
FLAG_ENOUGH, FLAG_EMPTY = 1, 2
MAX_K = 1024            # kFamilyCascadeMaxK (csrc/family_plan.h)


def bound(rule):
    """K: the most entries a family can have under the rule."""
    return max(rule.fs_min, rule.fs_max) + rule.fs_req_full + 2 * rule.fs_cover_gene


def row_words(rule):
    return 2 + 2 * bound(rule)


def saturated(rule, have, have_full, have_left, have_right):
    """No later candidate can be kept."""
    return (have >= max(rule.fs_min, rule.fs_max) and have_full >= rule.fs_req_full and have_left >= rule.fs_cover_gene
            and have_right >= rule.fs_cover_gene)


Pass = collections.namedtuple("Pass", "kept have have_full have_left have_right enough stop")


def cascade(cands, rule, early_exit=False):
    """One pass over cands = [(size, first_pos, last_pos, score, identity, is_self)] in ranked order.  Returns
    Pass(kept = indices kept, the four counters, enough, stop = the number of candidates looked at -- with early_exit
    the loop leaves at the first candidate before which `saturated` holds)."""
    range_begin = range_end = 0
    fs_msc, fs_msc_max = np.float32(rule.fs_msc), np.float32(rule.fs_msc_max)
    have = have_full = have_left = have_right = 0
    kept = []
    stop = len(cands)
    for x, (size, first, last, score, identity, is_self) in enumerate(cands):
        if early_exit and saturated(rule, have, have_full, have_left, have_right):
            stop = x
            break
        is_full = size >= rule.fs_full_len
        is_left = bool(size) and first <= range_begin
        is_right = bool(size) and last >= range_end
        if size < rule.fs_min_len:
            continue
        if is_self:
            continue
        if fs_msc_max < 1 and np.float32(identity) > fs_msc_max:
            continue
        min_reached, max_reached = have >= rule.fs_min, have >= rule.fs_max
        score_good = np.float32(score) < fs_msc                     # sic
        adds_to_full = bool(rule.fs_req_full) and have_full < rule.fs_req_full and is_full
        adds_to_range = bool(rule.fs_cover_gene) and ((have_right < rule.fs_cover_gene and is_right) or
                                                      (have_left < rule.fs_cover_gene and is_left))
        if min_reached and (max_reached or not score_good) and not adds_to_full and not adds_to_range:
            continue
        have += 1
        if rule.fs_req_full and is_full:
            have_full += 1
        if rule.fs_cover_gene and is_right:
            have_right += 1
        if rule.fs_cover_gene and is_left:
            have_left += 1
        kept.append(x)
    enough = not (have < rule.fs_max or have_full < rule.fs_req_full or have_left < rule.fs_cover_gene or
                  have_right < rule.fs_cover_gene)
    return Pass(kept, have, have_full, have_left, have_right, enough, stop)


def identity(match, query_bases):
    """float32(match) / float32(|query|); 0 for a query without bases."""
    return np.float32(match) / np.float32(query_bases) if query_bases else np.float32(0)


def candidates(meta, ids, scores, match, query_bases, self_ids):
    """The cascade's view of a ranked list: meta [n_refs, 3] = size, first and last column of every reference; match
    None = no counts (identity 0: only read where fs_msc_max < 1)."""
    selfs = set(int(s) for s in self_ids) if self_ids is not None else ()
    return [(int(meta[int(i), 0]), int(meta[int(i), 1]), int(meta[int(i), 2]), np.float32(scores[x]),
             identity(int(match[x]), query_bases) if match is not None else np.float32(0), int(i) in selfs)
            for x, i in enumerate(ids)]


def row(meta, ids, scores, match, query_bases, self_ids, rule):
    """The device's row of a query: uint32 [2 + 2 K] = kept, flags, K ids, K score bit patterns."""
    K = bound(rule)
    p = cascade(candidates(meta, ids, scores, match, query_bases, self_ids), rule)
    assert p.have == len(p.kept) <= K
    out = np.zeros(2 + 2 * K, np.uint32)
    out[0] = p.have
    out[1] = (FLAG_ENOUGH if p.enough else 0) | (FLAG_EMPTY if len(ids) == 0 else 0)
    kept = np.asarray(p.kept, np.int64)
    out[2:2 + len(kept)] = np.asarray(ids, np.uint32)[kept]
    out[2 + K:2 + K + len(kept)] = np.asarray(scores, np.float32)[kept].view(np.uint32)
    return out


def meta_of(refs):
    """[n, 3] size, first column, last column of packed base lists (a reference without bases: zeros)."""
    m = np.zeros((len(refs), 3), np.uint32)
    for i, r in enumerate(refs):
        if len(r):
            m[i] = (len(r), int(r[0]) & 0xFFFFFF, int(r[-1]) & 0xFFFFFF)
    return m


def escalate(lists, n_refs, rule, view):
    """famfinder::impl::run's loop around the pass: lists(M) -> (ids, scores) of the M best; view(ids, scores) -> the
    cascade's candidate tuples.  Returns (ids kept, scores kept, rounds = the M of every round)."""
    max_results = rule.fs_max + 1
    rounds = []
    while True:
        M = min(max_results, n_refs)
        rounds.append(M)
        ids, scores = lists(M)
        if len(ids) == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.float32), rounds
        p = cascade(view(ids, scores), rule)
        if p.enough or max_results >= n_refs:
            kept = np.asarray(p.kept, np.int64)
            return np.asarray(ids, np.uint32)[kept], np.asarray(scores, np.float32)[kept], rounds
        max_results *= 10
