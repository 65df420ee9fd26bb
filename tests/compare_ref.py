"""A plain reference for the search-stage comparison: the lock-step walk of two base lists, written from traverse() and
match_counter::counter (reference src/cseq_comparator.cpp:57-117, 151-206) in their order of steps, on Python integers.

It shares no idea with compare_kernel (column bitmap, rank, counts derived from ranges) nor with the host's
cseq_comparator::counts (filter first, then classify by range): two cursors, four loops.  A packed base is
column | mask << 24; bit 4 of the mask byte is the lower-case flag.  tests/test_compare_cpu.py pins this walk to the
oracle's; tests/test_gpu_compare.py compares the kernel with it."""

RULES = ("optimistic", "pessimistic", "exact")
FIELDS = ("only_a_overhang", "only_b_overhang", "only_a", "only_b", "match", "mismatch")


def _pos(x):
    return x & 0xFFFFFF


def _same(x, y, rule):
    ma, mb = (x >> 24) & 0xF, (y >> 24) & 0xF
    if rule == 0:                                   # base_iupac::comp
        return (ma & mb) != 0
    if rule == 1:                                   # comp_pessimistic
        return bin(ma).count("1") <= 1 and ma == mb
    return ma == mb                                 # comp_exact


def compare_ref(a, b, rule, filter_lc):
    """(only_a_overhang, only_b_overhang, only_a, only_b, match, mismatch) of the walk over base lists a and b (any
    sequence of packed words, columns ascending).  rule: 0 optimistic, 1 pessimistic, 2 exact."""
    assert rule in (0, 1, 2)
    A = [int(x) for x in a]
    B = [int(x) for x in b]

    def filtered(x):
        return bool(filter_lc) and ((x >> 24) & 0x10) != 0

    oa_over = ob_over = oa = ob = match = mismatch = 0
    i, i_end, j, j_end = 0, len(A), 0, len(B)
    # skip filtered bases at the beginning, then at the end
    while i != i_end and filtered(A[i]):
        i += 1
    while j != j_end and filtered(B[j]):
        j += 1
    while i != i_end and filtered(A[i_end - 1]):
        i_end -= 1
    while j != j_end and filtered(B[j_end - 1]):
        j_end -= 1
    # a side without any remaining base: the project's rule is six zeros (the reference reads past the end here)
    if i == i_end or j == j_end:
        return (0, 0, 0, 0, 0, 0)
    # left overhang
    if _pos(A[i]) < _pos(B[j]):
        while i != i_end and _pos(A[i]) < _pos(B[j]):
            if not filtered(A[i]):
                oa_over += 1
            i += 1
    else:
        while j != j_end and _pos(A[i]) > _pos(B[j]):
            if not filtered(B[j]):
                ob_over += 1
            j += 1
    # overlapping zone
    while i != i_end and j != j_end:
        diff = _pos(A[i]) - _pos(B[j])
        if diff > 0:
            if not filtered(B[j]):
                ob += 1
            j += 1
        elif diff < 0:
            if not filtered(A[i]):
                oa += 1
            i += 1
        else:
            fa, fb = filtered(A[i]), filtered(B[j])
            if not fa and not fb:
                if _same(A[i], B[j], rule):
                    match += 1
                else:
                    mismatch += 1
            elif not fa:
                oa += 1
            elif not fb:
                ob += 1
            i += 1
            j += 1
    # right overhang
    while i != i_end:
        if not filtered(A[i]):
            oa_over += 1
        i += 1
    while j != j_end:
        if not filtered(B[j]):
            ob_over += 1
        j += 1
    return (oa_over, ob_over, oa, ob, match, mismatch)
