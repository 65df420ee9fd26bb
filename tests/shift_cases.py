"""Hand-built column lists for the device assembly with shifted insertions (assemble = 2), each with a predicate that
says which branch of the widening loop it is there for.  tests/test_shift_cpu.py checks every predicate with the plain
restatement (tests/shift_ref.py) and pins the restatement to the oracle and the host; tests/test_gpu_shift.py runs the
cases through sina_hip_debug_assemble.

A case gives its columns in SEQUENCE order (`cols`, non-descending: what the fix-up sees) or as the columns handed to
cseq::append (`emitted`, append order: where the append rule or a column at the width matters), and the alignment's
width.  Everything else the device entry wants -- the query's masks, the walk's counts -- is made by inputs().
"""
import numpy as np

from tests import shift_ref as sr


class Case:
    def __init__(self, name, width, cols=None, emitted=None, why=None, cap=False):
        self.name, self.width, self.cap = name, width, cap
        self.emitted = [width - 1 - c for c in reversed(cols)] if emitted is None else list(emitted)
        self.why = why or (lambda fx: True)   # fx: shift_ref.fix_up's dict (None where a column lies beyond the width)

    @property
    def n(self):
        return len(self.emitted)


def _sides(fx, run=None):
    return "".join(s["side"] for s in fx["steps"] if run is None or s["run"] == run)


def _packed(first_col, n):
    return list(range(first_col, first_col + n))


def _block_with_run(n, at, dup, first_col=1):
    """n bases column to column from first_col, but base `at` repeated over `dup` further bases (a run that has no room)."""
    cols, c = [], first_col
    for j in range(n):
        cols.append(c)
        if not (at <= j < at + dup):
            c += 1
    return cols


def _shifted_units(k):
    """k insertions of one base, each with no room: bases c, c, c+1 every ten columns."""
    cols = []
    for u in range(k):
        cols += [10 * u + 4, 10 * u + 4, 10 * u + 5]
    return cols


def _ballot_edge_cases():
    out = []
    for at in (63, 64, 65):
        # a run whose first base is list position `at`, in a block packed from position 0: the left scan crosses
        # the ballot's block boundary on its way to the free column in front of the block
        cols = _block_with_run(at + 120, at, 2, first_col=3)
        out.append(Case("run_at_%d" % at, cols[-1] + 2, cols=cols,
                        why=lambda fx, at=at: fx["events"] and fx["steps"][0]["side"] == "L" and fx["steps"][0]["absorbed"] == at + 1))
        # the free column on the right lies between list positions at-1 and at; the run is on the first bases
        cols = [0, 0, 0] + _packed(1, at - 3)
        cols += _packed(cols[-1] + 3, 30)
        out.append(Case("right_gap_at_%d" % at, cols[-1] + 1, cols=cols,
                        why=lambda fx, at=at: _sides(fx, 0)[:1] == "R" and fx["steps"][0]["absorbed"] == at - 3))
        # ... and on the left, for a run on the last bases
        cols = _packed(2, at) + _packed(at + 4, 100 - at)
        cols += [cols[-1]] * 2
        out.append(Case("left_gap_at_%d" % at, cols[-1] + 1, cols=cols,
                        why=lambda fx, at=at: _sides(fx) == "LL" and fx["steps"][0]["absorbed"] == 100 - at))
    return out


def _length_cases():
    out = [Case("len_1", 10, cols=[3], why=lambda fx: fx["n_runs"] == 0),
           Case("len_2", 10, cols=[9, 9], why=lambda fx: _sides(fx) == "L")]
    for n in (63, 64, 65, 129):
        cols = _block_with_run(n, n // 2, 3, first_col=2)
        out.append(Case("len_%d" % n, cols[-1] + 3, cols=cols, why=lambda fx: len(fx["events"]) == 1 and len(fx["steps"]) == 3))
    return out


def _capacity_cases():
    out = []
    for n in (4095, 4096, 4097):
        # one run in the middle of a packed block: every widening scans ~2000 bases each way
        cols = _block_with_run(n, n // 2, 5, first_col=3)
        out.append(Case("bases_%d" % n, cols[-1] + 4, cols=cols, cap=n > sr.ASSEMBLE_MAX,
                        why=lambda fx: len(fx["steps"]) == 5 and set(_sides(fx)) == {"L", "R"}))
    return out


CASES = [
    Case("fits", 40, cols=[5, 5, 5, 20], why=lambda fx: fx["n_runs"] == 1 and not fx["events"] and fx["col"][1:3] == [18, 19]),
    Case("append_rule_makes_the_run", 40, emitted=[10, 4, 7, 30], why=lambda fx: fx["n_runs"] == 1 and not fx["events"]),
    Case("left_only_alignment_ends", 10, cols=[2, 3, 9, 9, 9], why=lambda fx: _sides(fx) == "LL" and fx["col"][2:] == [7, 8, 9]),
    Case("right_only_from_column_0", 20, cols=[0, 0, 0, 1, 2, 5], why=lambda fx: _sides(fx) == "RR" and fx["col"][:5] == [0, 1, 2, 3, 4]),
    Case("tie_goes_left", 20, cols=[3, 5, 5, 5, 7], why=lambda fx: _sides(fx) == "L" and fx["steps"][0]["tie"]),
    # (blocks of 7, 5, 3 and 1 bases on the left -- the last is the run's anchor -- and of 2, 4 and 6 on the right, one
    # free column between blocks: the nearer free column changes sides with every widening)
    Case("alternating", 40, cols=_packed(1, 7) + _packed(9, 5) + _packed(15, 3) + [19] * 5 + _packed(20, 2) + _packed(23, 4) + _packed(28, 6),
         why=lambda fx: "LRLR" in _sides(fx) or "RLRL" in _sides(fx)),
    Case("reaches_first_base", 30, cols=[2, 3, 4, 4, 4] + _packed(5, 10),
         why=lambda fx: any(s["reached_first"] for s in fx["steps"])),
    Case("reaches_last_base", 30, cols=[0, 0, 0, 1, 2, 3], why=lambda fx: any(s["reached_last"] for s in fx["steps"])),
    Case("right_scan_absorbs_a_later_run", 20, cols=[0, 0, 0, 1, 2, 2, 2, 9],
         why=lambda fx: fx["steps"][0]["dup_absorbed"] == 2 and len(fx["events"]) == 1 and fx["n_runs"] == 1),
    Case("run_at_the_end_fits", 20, cols=[1, 2, 8, 8, 8], why=lambda fx: not fx["events"] and fx["col"][3:] == [18, 19]),
    Case("run_on_the_first_two_fits", 20, cols=[4, 4, 9], why=lambda fx: not fx["events"] and fx["col"][1] == 8),
    Case("run_on_the_first_two_shifts", 20, cols=[4, 4, 5], why=lambda fx: len(fx["events"]) == 1 and fx["events"][0] == (1, 5, 5)),
    Case("left_through_placed_bases", 30, cols=[1, 1, 1, 6, 7, 7, 7, 7] + _packed(8, 8),
         why=lambda fx: any(s["side"] == "L" and s["placed_absorbed"] == 2 for s in fx["steps"])),
    Case("two_shifted_runs", 60, cols=_shifted_units(2), why=lambda fx: len(fx["events"]) == 2),
    Case("no_free_column", 3, cols=[0, 1, 2, 2], cap=True, why=lambda fx: fx["rc"] == -1),
    Case("widening_takes_the_width", 9, cols=[1, 1, 1, 6, 7, 7, 7, 7, 8], cap=True,
         why=lambda fx: fx["rc"] == 0 and max(fx["col"]) >= 9),
    Case("column_at_the_width", 12, emitted=[0, 5, 12], cap=True, why=lambda fx: fx is None),
    Case("column_at_the_width_by_the_append_rule", 12, emitted=[0, 12, 3, 3], cap=True, why=lambda fx: fx is None),
    Case("shifted_runs_32", 400, cols=_shifted_units(32), why=lambda fx: len(fx["events"]) == 32),
    Case("shifted_runs_33", 400, cols=_shifted_units(33), cap=True, why=lambda fx: fx["rc"] == 0 and len(fx["events"]) == 33),
] + _length_cases() + _ballot_edge_cases() + _capacity_cases()

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def inputs(case, overhang, seed=0):
    """What sina_hip_debug_assemble takes for the case: (qmask, o) with o the walk's counts as a dict.  Where the list
    is long enough one base is a tail overhang and two are a head overhang (under overhang=remove the walk emits
    none: all n bases are aligned ones, and the query is longer by the three).  Some masks are lower case."""
    n = case.n
    tail, head = (1, 2) if n >= 6 else (0, 0)
    rng = np.random.default_rng(1000 + seed + n)
    if overhang == sr.OVERHANG_REMOVE:
        L, aligned = n + tail + head, n
        end_s = L - 1 - tail
    else:
        L, aligned = n, n - tail - head
        end_s = n - 1 - tail
    qmask = rng.choice(np.array([1, 2, 4, 8, 15, 5, 17, 24], np.uint8), size=L)
    return qmask, dict(n_out=n, end_s=end_s, cutoff_head=head, cutoff_tail=tail, aligned_bases=aligned, status=0)


def random_cols(rng):
    """A seeded random list for the comparison with the oracle and the host: (cols in sequence order, width) --
    blocks of consecutive columns, few free columns between them, runs sprinkled in; tight widths make the
    widening reach the ends, and now and then there are more bases than columns."""
    n = int(rng.integers(1, 200))
    cols, c = [], int(rng.integers(0, 3))
    p_dup, p_gap = float(rng.choice([0.03, 0.1, 0.3])), float(rng.choice([0.02, 0.1, 0.3]))
    for _ in range(n):
        cols.append(c)
        r = rng.random()
        if r < p_dup:
            continue
        c += 1 + (int(rng.integers(1, 4)) if rng.random() < p_gap else 0)
    slack = int(rng.choice([0, 0, 1, 3, 40]))
    width = max(1, cols[-1] + 1 + slack)
    return cols, width


# ---------------------------------------------------------------- through the DP: a store laid out in blocks
# References whose bases occupy blocks of B consecutive columns with G free columns between the blocks -- the layout
# of a curated alignment's conserved stretches, where an insertion rarely finds a free column beside it (on the even
# grid of synth.make_refs it almost always does).
BLOCK_B, BLOCK_G = 20, 6


def block_store(n_refs=48, length=200, seed=71, B=BLOCK_B, G=BLOCK_G):
    """synth.make_refs without insertions, base i of the ancestor moved to column i + G * (i // B)."""
    from sina_amd import synth
    refs = synth.make_refs(n_refs, length=length, width=2 * length, seed=seed, n_clades=3, ins_rate=0.0,
                           long_del_prob=0.0, del_rate=0.01)
    i = (refs.ab & 0xFFFFFF) // 2
    ab = ((i + G * (i // B)).astype(np.uint32) | (refs.ab & 0xFF000000)).astype(np.uint32)
    width = length + G * (length // B) + G
    return synth.RefSet(ab=ab, off=refs.off, width=int(width))


_DP_WORLD = {}


def dp_world(lowercase=sr.LOWERCASE_UNALIGNED):
    """The inputs of the through-DP tests and the oracle's answers, computed once: dict(refs, qs, fam_ids, fam_off,
    qmask, qoff, want) with want[q] = pyoracle.align's dict for query q (realign: the family as famfinder gave it)."""
    if lowercase in _DP_WORLD:
        return _DP_WORLD[lowercase]
    from oracle import pyoracle as po
    from sina_amd import synth
    from tests import util
    refs = block_store()
    qs = synth.make_queries(refs, 16, seed=72, sub=[0.005, 0.03, 0.1, 0.2], dele=0.01, ins=0.02)
    cs = util.cseqs_from_refs(refs)
    idx = po.Index(cs, k=8)
    fam_ids, fam_off, qmasks, want = [], [0], [], []
    for qi in range(qs.n):
        q = util.query_cseq(qs, qi)
        ids, _, _ = idx.famfinder(q)
        assert len(ids) > 0
        fam_ids += [int(x) for x in ids]
        fam_off.append(len(fam_ids))
        qmasks.append((q.packed() >> 24).astype(np.uint8))
        want.append(po.align([cs[int(i)] for i in ids], q, po.align_opts(realign=1, lowercase=lowercase)))
    qoff = np.zeros(qs.n + 1, np.uint64)
    qoff[1:] = np.cumsum([len(m) for m in qmasks])
    w = dict(refs=refs, qs=qs, fam_ids=np.array(fam_ids, np.uint32), fam_off=np.array(fam_off, np.uint64),
             qmask=np.concatenate(qmasks), qoff=qoff, want=want)
    _DP_WORLD[lowercase] = w
    return w


def log_events(log):
    """[(N, B, E)] of the "shifting bases to fit in N bases at pos B to E;" texts of a log, in order."""
    import re
    return [tuple(int(x) for x in m) for m in re.findall(r"shifting bases to fit in (\d+) bases at pos (\d+) to (\d+);", log)]


def log_totals(log):
    """(total, longest, before shifting) of a log's totals text, or (0, 0, 0)."""
    import re
    m = re.search(r"total inserted bases=(\d+);longest insertion=(\d+);total inserted bases before shifting=(\d+);", log)
    return tuple(int(x) for x in m.groups()) if m else (0, 0, 0)


def stage_world():
    """The store and queries of the stage-level test: (refs, queries, indices of the queries beyond the device's caps).
    Short blocks -- 6 columns, 2 free ones between -- so that insertions in different blocks stay runs of their own:
    sixteen mutated queries, and two copies of a reference with a base inserted in the middle of every block (some
    fifty shifted runs, more than SINA_HIP_SHIFT_LOG), which the host must finish whatever the options say."""
    from sina_amd import synth
    refs = block_store(n_refs=48, length=300, seed=74, B=6, G=2)
    qs = synth.make_queries(refs, 16, seed=75, sub=[0.005, 0.03, 0.1], dele=0.01, ins=0.02)
    rng = np.random.default_rng(76)
    parts = [qs.seq(i) for i in range(qs.n)]
    for src in (3, 17):
        m = ((refs.seq(src) >> 24) & 0x0F).astype(np.uint8)
        out = []
        for j, b in enumerate(m):
            out.append(b)
            if j % 6 == 2 and j + 2 < len(m):
                out.append(rng.choice([x for x in (1, 2, 4, 8) if x != m[j + 1] and x != b]))
        parts.append(np.array(out, np.uint8))
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return refs, synth.QuerySet(mask=np.concatenate(parts), off=off, src=np.concatenate([qs.src, [3, 17]])), (16, 17)
