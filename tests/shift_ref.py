"""A plain restatement of the whole container path behind the trace-back walk, insertions that shift their neighbours
included: the append rule (src/cseq.cpp:79-95), setWidth + reverse (the mirror), the NAST fix-up with its widening loop
(src/cseq.cpp:456-594), the case bits, the log events and the log line's three facts -- what assemble_kernel<true>
(sina_amd/csrc/traceback.hip, sina_hip_align_params::assemble == 2) computes on the device.

Lists and integers only, one step of the reference per statement; tests/test_shift_cpu.py pins it against the oracle's
so_cseq_fix_duplicate_positions and the host's sina_host_fix_duplicates.  Besides the result it keeps what the reference
throws away: which way every widening went and what it took along, so that tests/shift_cases.py can say which branch a
case is there for.
"""
import numpy as np

ASSEMBLE_MAX = 4096     # include/sina_hip.h: more than 4096 bases are the host's
SHIFT_LOG = 32          # include/sina_hip.h, SINA_HIP_SHIFT_LOG: more shifted runs in one query are the host's
OVERHANG_ATTACH, OVERHANG_REMOVE, OVERHANG_EDGE = 0, 1, 2
LOWERCASE_NONE, LOWERCASE_ORIGINAL, LOWERCASE_UNALIGNED = 0, 1, 2


def append_rule(emitted):
    """cseq::append: a column left of the sequence's current end is moved up to it -- a running maximum."""
    out, cur = [], 0
    for c in emitted:
        cur = max(cur, int(c))
        out.append(cur)
    return out


def mirror(colm, width):
    """setWidth(width) + reverse(): sequence position j is append n-1-j, column c becomes width - 1 - c."""
    return [width - 1 - c for c in reversed(colm)]


def fix_up(col, width):
    """fix_duplicate_positions over the columns `col` (sequence order, non-descending).  Returns a dict: rc (0, or -1
    where the reference throws "no space to left and right"), col (the placed columns), moved (a flag per base: the
    fix-up positioned it), events [(N, B, E)], total / longest / last_run (the log line's numbers) and steps: one
    dict(run, side 'L' / 'R', tie, absorbed (bases taken along), dup_absorbed (of them, bases that shared a column
    with their left neighbour: a later run walked through), placed_absorbed (bases an earlier run had placed),
    reached_first, reached_last) per turn of the widening loop."""
    b = [int(c) for c in col]
    n = len(b)
    moved = [False] * n
    events, steps = [], []
    total = longest = orig = 0
    n_runs = 0
    last_it, curr_it = 0, 0
    while curr_it < n:
        if b[last_it] == b[curr_it]:
            if curr_it + 1 != n:
                curr_it += 1
                continue
            curr_it += 1
        num = curr_it - last_it - 1
        if num == 0:
            last_it = curr_it
            curr_it += 1
            continue
        range_begin = b[last_it] + 1
        range_end = width if curr_it == n else b[curr_it]
        last_it += 1
        curr_it -= 1
        orig = num
        n_runs += 1
        if range_end - range_begin < num:
            events.append((num, range_begin, range_end))
            while range_end - range_begin < num:
                left, right = last_it, curr_it
                if left == 0:
                    nlg = range_begin - 1 if range_begin > 0 else -1
                elif b[left - 1] + 1 < range_begin:
                    nlg = range_begin - 1
                else:
                    left -= 1
                    while left != 0 and b[left - 1] + 1 >= b[left]:
                        left -= 1
                    nlg = b[left] - 1
                if right + 1 == n:
                    nrg = range_end if range_end < width else -1
                else:
                    if b[right + 1] > range_end:
                        nrg = range_end
                    else:
                        right += 1
                        while right + 1 != n and b[right] + 1 >= b[right + 1]:
                            right += 1
                        nrg = b[right] + 1
                dl, dr = range_begin - nlg, nrg - (range_end - 1)
                if nrg == -1 or (nlg != -1 and dl <= dr):
                    if nlg == -1:
                        return dict(rc=-1, col=b, moved=moved, events=events, total=total, longest=longest,
                                    last_run=orig, steps=steps, n_runs=n_runs)
                    took = list(range(left, last_it))
                    steps.append(dict(run=n_runs - 1, side="L", tie=nrg != -1 and dl == dr, absorbed=len(took),
                                      dup_absorbed=0, placed_absorbed=sum(moved[t] for t in took),
                                      reached_first=left == 0 and len(took) > 0, reached_last=False))
                    num += last_it - left
                    range_begin = nlg
                    last_it = left
                else:
                    took = list(range(curr_it + 1, right + 1))
                    steps.append(dict(run=n_runs - 1, side="R", tie=False, absorbed=len(took),
                                      dup_absorbed=sum(b[t] == b[t - 1] for t in took), placed_absorbed=0,
                                      reached_first=False, reached_last=right == n - 1 and len(took) > 0))
                    num += right - curr_it
                    range_end = nrg + 1
                    curr_it = right
        else:
            range_begin = range_end - num
        curr_it += 1
        while last_it != curr_it:
            b[last_it] = range_begin
            moved[last_it] = True
            range_begin += 1
            last_it += 1
        total += num
        longest = max(longest, num)
        last_it = curr_it
        # (the reference's for loop steps on: the base at curr_it is the next anchor)
        curr_it += 1
    return dict(rc=0, col=b, moved=moved, events=events, total=total, longest=longest, last_run=orig, steps=steps,
                n_runs=n_runs)


def log_text(fx):
    """What the reference writes to the log: one "shifting" text per event, then the totals if anything was placed."""
    txt = "".join("shifting bases to fit in %d bases at pos %d to %d;" % e for e in fx["events"])
    if fx["rc"] == 0 and fx["total"] > 0:
        txt += "total inserted bases=%d;longest insertion=%d;total inserted bases before shifting=%d;" % (
            fx["total"], fx["longest"], fx["last_run"])
    return txt


def fix_words(ab, width, lowercase):
    """The fix-up over packed aligned bases (column | mask << 24), as so_cseq_fix_duplicate_positions and
    sina_host_fix_duplicates take them: (rc, words, log text, fix_up's dict)."""
    ab = np.asarray(ab, np.uint32)
    fx = fix_up([int(x) & 0xFFFFFF for x in ab], width)
    masks = [(int(x) >> 24) | (16 if lowercase and m else 0) for x, m in zip(ab, fx["moved"])]
    words = np.array([c | (m << 24) for c, m in zip(fx["col"], masks)], np.uint32)
    return fx["rc"], words, log_text(fx), fx


def finish(emitted, qmask, o, width, overhang, lowercase):
    """The whole path for one query as the device sees it: `emitted` are the columns handed to cseq::append (append
    order), qmask the query's masks, o a dict with end_s, cutoff_head, cutoff_tail, aligned_bases (n_out is
    len(emitted)).  Returns dict(colm, beyond, fx, words, must): words are the finished packed bases in sequence order
    (None where the fix-up throws or a column lies beyond the width), must what must_assemble_shift says."""
    n = len(emitted)
    colm = append_rule(emitted)
    beyond = any(c >= width for c in colm)
    if beyond:
        return dict(colm=colm, beyond=True, fx=None, words=None, must=False)
    fx = fix_up(mirror(colm, width), width)
    tail = o["cutoff_tail"] if overhang != OVERHANG_REMOVE else 0
    n_al = o["aligned_bases"]
    first_q = o["end_s"] + tail               # the query index of append 0
    keep = 0xFF if lowercase == LOWERCASE_ORIGINAL else 0xEF
    words = []
    for j in range(n):
        i = n - 1 - j
        over = i < tail or i >= tail + n_al
        bits = int(qmask[first_q - i]) & keep
        if lowercase == LOWERCASE_UNALIGNED and (over or fx["moved"][j]):
            bits |= 16
        words.append((fx["col"][j] & 0xFFFFFF) | (bits << 24))
    return dict(colm=colm, beyond=False, fx=fx, words=np.array(words, np.uint32) if fx["rc"] == 0 else None,
                must=must_assemble_shift(n, colm, width, fx))


def must_assemble_shift(n_out, colm, width, fx):
    """include/sina_hip.h, SINA_ASSEMBLE_SHIFT: the device finishes a query unless it has more than 4096 bases, a
    column at or beyond the width, more than 32 shifted runs, no free column on either side (the reference throws),
    or a widening that takes the column `width` for free and places a base there (a right scan that ends on a last
    base in column width - 1: the reference does not look, the result has a column beyond the alignment)."""
    if n_out > ASSEMBLE_MAX or any(c >= width for c in colm):
        return False
    if fx is None or fx["rc"] != 0 or len(fx["events"]) > SHIFT_LOG:
        return False
    return all(c < width for c in fx["col"])
