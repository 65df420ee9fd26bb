"""A plain restatement of the cell walk of backtrack() (src/mesh.h:567-721) and of the container steps behind it
(append rule, NAST fix-up: src/cseq.cpp:79-95, 456-594), for the tests of the device's trace-back stage.

It works on the ORACLE's full planes (oracle.mesh_compute: value, value_midx, value_sidx) and on the family
DAG as the oracle built it -- nothing of the device's cell encodings (type codes, predecessor ordinals,
Ext / OpLast) is in here.  It follows oracle/sina_oracle.c:so_backtrack step for step, but keeps what that
throws away: the end cell, the appended columns in append order, sum_weight, the path, and a few statistics
of the path that the tests use as coverage conditions.  tests/test_walk_cpu.py pins it against so_backtrack.
"""
import numpy as np

OVERHANG_ATTACH, OVERHANG_REMOVE, OVERHANG_EDGE = 0, 1, 2
ASSEMBLE_MAX = 4096     # include/sina_hip.h, sina_hip_align_out::assembled: "more than 4096 bases"


def opts_dict(**kw):
    """The options the walk reads, with the aligner's defaults (src/align.cpp:231-274)."""
    o = dict(match_score=2.0, mismatch_score=-1.0, gap_penalty=5.0, gap_ext_penalty=2.0, overhang=OVERHANG_ATTACH,
             weights=None)
    o.update(kw)
    return o


def _self_score16(ms, mms):
    """base_profile::comp of a base's own profile with itself (src/pseq.h:65-113) for the 16 iupac masks:
    sixteen float32 products added in i-outer, j-inner order (no contraction)."""
    out = np.zeros(16, np.float32)
    for mask in range(1, 16):
        order = bin(mask).count("1")
        v = [np.float32(1.0) / np.float32(order) if mask & (1 << i) else np.float32(0.0) for i in range(4)]
        res = np.float32(0.0)
        for i in range(4):
            for j in range(4):
                res = np.float32(res + np.float32(np.float32((ms if i == j else mms) * v[i]) * v[j]))
        out[mask] = res    # (+ gap * 0 + gap_ext * 0: a base's profile has no gap shares)
    return out


def end_cell(graph, value):
    """mesh.h:567-592: the smallest value of the last column over all rows (first row wins a tie, the first sink
    wins a tie against every row), then anything strictly smaller in a sink's row (sinks in order, first column
    wins)."""
    L = value.shape[1]
    col = value[:, L - 1]
    m = int(graph["snk"][0])
    if col.min() < col[m]:
        m = int(np.argmin(col))
    s = L - 1
    cur = value[m, s]
    for mt in graph["snk"]:
        row = value[int(mt)]
        if row.min() < cur:
            m, s = int(mt), int(np.argmin(row))
            cur = row[s]
    return m, s


def walk(graph, planes, qmask, width, opts):
    """The walk of one query.  graph: the oracle's DAG (util.graph_dict / oracle.pseq_build); planes: the structured
    cell array of oracle.mesh_compute; qmask: the query's iupac masks; opts: opts_dict().  Returns a dict:
    end_m, end_s, raw, sum_weight (np.float32, accumulated in the reference's order), cutoff_head, cutoff_tail,
    aligned_bases, n_out, cols (the columns handed to cseq::append, in append order), rows (the row of every path
    cell visited, in order) and stats (see path statistics below)."""
    value, vmid, vsid = planes["value"], planes["value_midx"], planes["value_sidx"]
    N, L = value.shape
    gpos = graph["pos"].astype(np.int64)
    gw = graph["weight"]
    pred_off, pred = graph["pred_off"], graph["pred"]
    srcs = set(int(x) for x in graph["src"])
    snks = set(int(x) for x in graph["snk"])
    profile = graph.get("prof") is not None
    ms = np.float32(-np.float32(opts["match_score"]))
    w = None if profile or opts.get("weights") is None else np.asarray(opts["weights"], np.float32)
    self16 = _self_score16(ms, np.float32(-np.float32(opts["mismatch_score"]))) if profile else None
    qmask = np.asarray(qmask, np.uint8)
    overhang = int(opts["overhang"])
    send = L - 1

    def match_term(m, s):  # scoring scheme's match(prev, master copy carrying the slave's base, slave): comp() is true
        if profile:
            return self16[int(qmask[s]) & 15]
        if w is None:
            return np.float32(ms * gw[m])
        return np.float32(np.float32(ms * w[min(int(gpos[m]), len(w) - 1)]) * gw[m])

    m, s = end_cell(graph, value)
    end_m, end_s = m, s
    cols, rows = [], [m]
    cutoff_tail = send - s
    if cutoff_tail and overhang != OVERHANG_REMOVE:   # right hand overhang, :594-615
        p = (width - 1 - int(gpos[m]) - cutoff_tail) if overhang == OVERHANG_ATTACH else 0
        for _ in range(cutoff_tail):
            cols.append(max(p, 0))
            p += 1
    raw = value[m, s]
    pos = width - 1 - int(gpos[m])
    cols.append(pos)
    aligned = 1
    sum_weight = np.float32(np.float32(0.0) + match_term(m, s))

    st = dict(longest_ins_run=0, ins_reaches_col0=0, max_row_jump=0, ord_ge4=0, max_npred=0, deletions=0,
              far_deletions=0, end_inner_sink=int(m in snks and s < send), end_last_col_nonsink=int(m not in snks and s == send))

    def visit(m_from, s_from, m_to):
        """statistics of one look-up: cell (m_from, s_from) points at row m_to"""
        pl = pred[pred_off[m_from]:pred_off[m_from + 1]]
        st["max_npred"] = max(st["max_npred"], len(pl))
        st["max_row_jump"] = max(st["max_row_jump"], abs(m_from - m_to))
        hit = np.flatnonzero(pl == m_to)
        if len(hit) and int(hit[0]) >= 4:
            st["ord_ge4"] += 1
        return len(hit) > 0

    while s != 0 and m not in srcs:    # :642-685
        snew = int(vsid[m, s])
        mnew = int(vmid[m, s])
        direct = visit(m, s, mnew)
        if snew == s:                   # a deletion cell: the gap's opener is value_midx
            st["deletions"] += 1
            st["far_deletions"] += int(not direct)
        elif mnew == m:                 # an insertion cell: bases s-1 .. snew share m's column
            st["longest_ins_run"] = max(st["longest_ins_run"], s - snew)
            st["ins_reaches_col0"] += int(snew == 0)
        m = mnew
        rows.append(m)
        if snew != 0 and int(vsid[m, snew]) == snew:   # the one-step deletion skip, :653-655
            m2 = int(vmid[m, snew])
            direct = visit(m, snew, m2)
            st["deletions"] += 1
            st["far_deletions"] += int(not direct)
            m = m2
            rows.append(m)
        pos = width - 1 - int(gpos[m])
        while s != snew:
            s -= 1
            cols.append(pos)
            aligned += 1
            sum_weight = np.float32(sum_weight + match_term(m, s))
    st["stop_col0"] = int(s == 0)
    st["stop_source_inner"] = int(s != 0)

    cutoff_head = 0
    if s != 0:                           # left hand overhang, :690-721
        cutoff_head = s
        if overhang == OVERHANG_ATTACH:
            while s != 0:
                s -= 1
                pos += 1
                cols.append(min(pos, width - 1))
        elif overhang == OVERHANG_EDGE:
            for k in range(s - 1, -1, -1):
                cols.append(width - k - 1)
    return dict(end_m=end_m, end_s=end_s, raw=np.float32(raw), sum_weight=np.float32(sum_weight),
                cutoff_head=cutoff_head, cutoff_tail=cutoff_tail, aligned_bases=aligned, n_out=len(cols),
                cols=np.asarray(cols, np.int64), rows=np.asarray(rows, np.int64), stats=st)


def container_facts(cols, width):
    """The append rule (a column left of the sequence's current width is moved up to it: a running maximum) and the
    runs of equal columns it leaves -- the insertions fix_duplicate_positions places.  In append order a run's
    first entry is its LAST base in sequence order; the base before the run (in append order) is the next base to
    the right, or the alignment ends there.  Returns dict(colm, beyond, fits, nast_total, nast_longest,
    nast_last_run, runs); the three numbers are the log line's where every run fits (a run that does not fit makes
    its neighbours move and counts them too)."""
    cols = np.asarray(cols, np.int64)
    colm = np.maximum.accumulate(cols) if len(cols) else cols
    beyond = bool((colm >= width).any())
    runs = []           # (first append index of the run, number of bases to place)
    i, n = 1, len(colm)
    while i < n:
        if colm[i] == colm[i - 1]:
            i0 = i - 1
            r = 0
            while i < n and colm[i] == colm[i - 1]:
                r += 1
                i += 1
            runs.append((i0, r))
        else:
            i += 1
    fits = True
    for i0, r in runs:
        anchor = width - 1 - int(colm[i0])
        nxt = width - 1 - int(colm[i0 - 1]) if i0 > 0 else width
        if nxt - (anchor + 1) < r:
            fits = False
    return dict(colm=colm, beyond=beyond, fits=fits, runs=runs,
                nast_total=sum(r for _, r in runs), nast_longest=max([r for _, r in runs] or [0]),
                nast_last_run=runs[0][1] if runs else 0)


def must_assemble(n_out, facts):
    """include/sina_hip.h, sina_hip_align_out::assembled: the device finishes a query unless an insertion does not
    fit its gap, a column lies beyond the alignment, or it has more than 4096 bases."""
    return bool(n_out <= ASSEMBLE_MAX and not facts["beyond"] and facts["fits"])


def out_masks(qmask, wk, overhang, lowercase_unaligned):
    """The query masks in append order (tail overhang, aligned bases from end_s downwards, head overhang), overhang
    bases lower-cased under --lowercase=unaligned."""
    qmask = np.asarray(qmask, np.uint8)
    keep = overhang != OVERHANG_REMOVE
    tail = wk["cutoff_tail"] if keep else 0
    head = wk["cutoff_head"] if keep else 0
    idx = [len(qmask) - 1 - i for i in range(tail)] + [wk["end_s"] - i for i in range(wk["aligned_bases"])] + \
          [wk["cutoff_head"] - 1 - i for i in range(head)]
    m = qmask[np.asarray(idx, np.int64)].copy()
    if lowercase_unaligned:
        m[:tail] |= 16
        if head:
            m[-head:] |= 16
    return m
