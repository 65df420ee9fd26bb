"""The inputs of the trace-back tests, shared by tests/test_walk_cpu.py (which pins the plain walk against the oracle
and asserts that every directed case still reaches its edge) and tests/test_gpu_walk.py (which runs the same cases
through sina_hip_align_graphs).  Everything here is CPU work: synth + the oracle."""
import functools

import numpy as np

from oracle import pyoracle as po
from sina_amd import synth
from tests import util, walk_ref


class Case:
    """One launch: queries (iupac masks AS THE DEVICE GETS THEM, case bit included) with their families, one set of
    options.  variants: test-knob settings (util.set_knobs) the GPU test repeats the launch under."""

    def __init__(self, name, width, fams, qmasks, variants=None, **opts):
        self.name, self.width, self.fams = name, int(width), fams
        self.qmasks = [np.asarray(m, np.uint8) for m in qmasks]
        self.variants = variants or [{}]
        self.opts = dict(match_score=2.0, mismatch_score=-1.0, gap_penalty=5.0, gap_ext_penalty=2.0, fs_weight=1.0,
                         overhang=0, lowercase=0, insertion=0, weights=None, fs_no_graph=0)
        assert set(opts) <= set(self.opts), opts
        self.opts.update(opts)

    def oracle_opts(self):
        return po.align_opts(**self.opts)

    def walk_opts(self):
        return walk_ref.opts_dict(**{k: self.opts[k] for k in ("match_score", "mismatch_score", "gap_penalty",
                                                                "gap_ext_penalty", "overhang", "weights")})

    def oracle_masks(self, i):
        """What the aligner hands backtrack(): upper-cased unless --lowercase=original (src/align.cpp:324-326)."""
        m = self.qmasks[i]
        return m if self.opts["lowercase"] == 1 else (m & 0x0f)


def _cseq(name, masks):
    m = np.asarray(masks, np.uint8)
    return po.Cseq.from_packed(name, np.arange(len(m), dtype=np.uint32) | (m.astype(np.uint32) << 24), len(m))


def profile_tables(fam, opts):
    """(graph, node_score16 [n, 16], self_score16 [16]) of a family as a profile, the way host/family_graph.cpp builds
    them for the pipeline: base_profile::comp of the column with each of the 15 iupac masks (mask 0: +inf, no
    query base has it); the scheme gets the negated scores (src/align.cpp:406-414)."""
    g = po.pseq_build(fam)
    ms, mms = -opts["match_score"], -opts["mismatch_score"]
    gp, gpe = opts["gap_penalty"], opts["gap_ext_penalty"]
    n = g["n"]
    tab = np.full((n, 16), np.inf, np.float32)
    for node in range(n):
        for m in range(1, 16):
            tab[node, m] = po.profile_comp(g["prof"][node], m, ms, mms, gp, gpe)
    self16 = np.zeros(16, np.float32)
    for m in range(1, 16):
        self16[m] = po.profile_comp(None, m, ms, mms, gp, gpe)
    g["succ_minpos"] = np.append(g["pos"][1:], np.uint32(1000000)).astype(np.uint32)
    return g, tab, self16


def reference(case):
    """Per query: the oracle's DAG, planes, backtrack() result, and the plain walk with its container facts."""
    out, graphs = [], {}
    for i, (fam, qm) in enumerate(zip(case.fams, case.qmasks)):
        if id(fam) not in graphs:
            if case.opts["fs_no_graph"]:
                graphs[id(fam)] = profile_tables(fam, case.opts)
            else:
                graphs[id(fam)] = (util.graph_dict(fam, case.opts["fs_weight"]), None, None)
        g, tab, self16 = graphs[id(fam)]
        om = case.oracle_masks(i)
        orc = po.backtrack(fam, _cseq("q%d" % i, om), case.oracle_opts())
        assert orc["status"] == 0, (case.name, i)
        wk = walk_ref.walk(g, orc.pop("cells"), om, case.width, case.walk_opts())
        facts = walk_ref.container_facts(wk["cols"], case.width)
        out.append(dict(graph=g, score16=tab, self16=self16, orc=orc, walk=wk, facts=facts,
                        must=walk_ref.must_assemble(wk["n_out"], facts), oracle_masks=om))
    return out


def nast_numbers(log):
    """The three numbers of the fix-up's log line, (0, 0, 0) where none is printed."""
    import re
    m = re.search(r"total inserted bases=(\d+);longest insertion=(\d+);total inserted bases before shifting=(\d+);", log)
    return tuple(int(x) for x in m.groups()) if m else (0, 0, 0)


# ---------------------------------------------------------------- worlds

@functools.lru_cache(maxsize=None)
def world_small():
    """`small` of tests/test_gpu_parity.py."""
    refs = synth.make_refs(400, length=300, width=3000, seed=11, amb_rate=0.01, lower_rate=0.02)
    qs = synth.make_queries(refs, 12, seed=12, amb_rate=0.01, lower_rate=0.05)
    cs = util.cseqs_from_refs(refs)
    return refs, qs, cs, po.Index(cs, k=10)


@functools.lru_cache(maxsize=None)
def world_16s():
    refs = synth.make_refs(300, length=1500, width=50000, seed=21)
    qs = synth.make_queries(refs, 8, seed=22)
    cs = util.cseqs_from_refs(refs)
    return refs, qs, cs, po.Index(cs, k=10)


def _fam_of(world, qi, **ff):
    refs, qs, cs, idx = world
    ids, _, _ = idx.famfinder(util.query_cseq(qs, qi), po.ff_opts(**ff) if ff else None)
    assert len(ids) > 0
    return [cs[i] for i in ids]


def _splice(m, at, n, rng):
    return np.concatenate([m[:at], rng.choice([1, 2, 4, 8], size=n).astype(np.uint8), m[at:]])


def _cut(m, at, n):
    return np.concatenate([m[:at], m[at + n:]])


# ---------------------------------------------------------------- the parameter matrix on `small`

MATRIX_NAMES = tuple(["matrix-oh%d-lc%d" % (oh, lc) for oh in (0, 1, 2) for lc in (0, 1, 2)] +
                     ["matrix-weighted", "matrix-weighted-forbid", "matrix-profile", "matrix-profile-forbid"])


def cases_matrix():
    """The twelve queries of `small` (one in twenty bases lower case) under every overhang and lowercase mode, shift and
    forbid, the simple, the weighted and the profile scheme."""
    w = world_small()
    refs, qs = w[0], w[1]
    fams = [_fam_of(w, qi) for qi in range(qs.n)]
    qms = [qs.seq(qi) for qi in range(qs.n)]
    weights = np.random.default_rng(5).uniform(0.2, 1.5, size=refs.width).astype(np.float32)
    out = []
    for oh in (0, 1, 2):
        for lc in (0, 1, 2):
            out.append(Case("matrix-oh%d-lc%d" % (oh, lc), refs.width, fams, qms, overhang=oh, lowercase=lc,
                            insertion=(oh + lc) % 2))
    out.append(Case("matrix-weighted", refs.width, fams, qms, weights=weights, lowercase=2))
    out.append(Case("matrix-weighted-forbid", refs.width, fams, qms, weights=weights, insertion=1, overhang=2))
    out.append(Case("matrix-profile", refs.width, fams[:6], qms[:6], fs_no_graph=1, lowercase=1))
    out.append(Case("matrix-profile-forbid", refs.width, fams[6:], qms[6:], fs_no_graph=1, insertion=1, overhang=1))
    assert tuple(c.name for c in out) == MATRIX_NAMES
    return out


# ---------------------------------------------------------------- directed edges (the conditions: test_walk_cpu.py)

def cases_insertion_scan():
    """16S-length queries with 70 / 130 random bases spliced in mid-query: the insertion's emissions outnumber the 32
    columns of the wave walk's window (its leftward scan for the insertion's start refills mid-scan), and the
    insertion does not fit its gap."""
    w = world_16s()
    refs, qs = w[0], w[1]
    rng = np.random.default_rng(501)
    fams = [_fam_of(w, 0), _fam_of(w, 1)]
    qms = [_splice(qs.seq(0), 500, 70, rng), _splice(qs.seq(1), 500, 130, rng)]
    return [Case("ins-scan-default", refs.width, fams, qms),
            Case("ins-scan-6-0.5", refs.width, fams, qms, gap_penalty=6.0, gap_ext_penalty=0.5)]


def cases_insertion_col0():
    """Queries that begin with bases inserted relative to their family, the family's members being longer on that
    side: an alignment may start for free in column 0 of ANY row, so the first junk base sits on an inner row and
    the others are an insertion whose start is column 0 (value_sidx == 0: the leftward scan ends at k == 0).
    Mismatches are dear and gaps cheap here, or the junk would be aligned base for base."""
    w = world_small()
    refs, qs = w[0], w[1]
    rng = np.random.default_rng(502)
    fams, qms = [], []
    for qi in range(4):
        m = qs.seq(qi) & 0x0f
        fams.append(_fam_of(w, qi))
        qms.append(np.concatenate([rng.choice([1, 2, 4, 8], size=6 + 3 * qi).astype(np.uint8), m[100:220]]))
    sc = dict(match_score=0.2, mismatch_score=-8.0, gap_penalty=1.0, gap_ext_penalty=0.1)
    return [Case("ins-col0", refs.width, fams, qms, **sc), Case("ins-col0-forbid", refs.width, fams, qms, insertion=1, **sc)]


def cases_row_jump():
    """Queries with 150 (16S) / 60 (`small`) bases cut out: two consecutive path cells lie more rows apart than the 64
    of the window, across deletion cells whose opener is not a direct predecessor (the device resolves Ext there)."""
    w = world_16s()
    refs, qs = w[0], w[1]
    a = Case("row-jump-16s", refs.width, [_fam_of(w, 2), _fam_of(w, 3)],
             [_cut(qs.seq(2), 900, 150), _cut(qs.seq(3), 900, 150)])
    w = world_small()
    refs, qs = w[0], w[1]
    b = Case("row-jump-small", refs.width, [_fam_of(w, qi) for qi in range(4)],
             [_cut(qs.seq(qi), 120, 60) for qi in range(4)])
    c = Case("row-jump-small-forbid", refs.width, b.fams, b.qmasks, insertion=1)
    return [a, b, c]


def cases_many_predecessors():
    """Families with a dozen characters per column (nine in ten bases an ambiguity code, half of them lower case,
    long deletions): path steps to predecessors beyond the four the window caches per row."""
    refs = synth.make_refs(200, length=300, width=3000, seed=171, amb_rate=0.9, lower_rate=0.5, long_del_prob=0.5)
    cs = util.cseqs_from_refs(refs)
    rng = np.random.default_rng(14)
    out = []
    for F in (40, 128):
        ids = rng.choice(refs.n, size=F, replace=False)
        fam = [cs[int(i)] for i in ids]
        qms = [(refs.seq(int(i)) >> 24).astype(np.uint8) for i in ids[:3]]
        qms = [m for m in qms if len(m) >= 60]
        for ins in (0, 1):
            out.append(Case("many-preds-F%d-ins%d" % (F, ins), refs.width, [fam] * len(qms), qms, insertion=ins, lowercase=1))
    return out


ALIGN_LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)
# junk bases behind each (none behind the short ones: fifteen bases find a better place somewhere in the family than
# in front of their junk): end_s = L - 1 - tail then takes every residue modulo 8
ALIGN_TAILS = {1: 0, 2: 0, 7: 0, 8: 0, 9: 0, 15: 0, 16: 0, 17: 0, 31: 4, 32: 4, 33: 4, 63: 1, 64: 5, 65: 3, 255: 3, 256: 3, 257: 6}


def cases_load_alignment():
    """Query lengths around the 16-byte loads of the window refill, in ONE ragged launch and each alone; every query a
    piece of a family member that ends at a sink of the DAG (the family is cut off there), followed by junk the aligner cuts off as tail overhang, so
    the walk starts at a column inside the query."""
    w = world_small()
    refs, qs, cs, _ = w
    # the family cut off behind a base of its first member: that base's node is a sink and no node lies behind it,
    # so bases behind a piece that ends there can only be overhang
    full = _fam_of(w, 0)
    cutcol = int(full[0].packed()[-5] & 0xFFFFFF)
    fam = []
    for k, c in enumerate(full):
        ab = c.packed()
        fam.append(po.Cseq.from_packed("cut%d" % k, ab[(ab & 0xFFFFFF) <= cutcol], refs.width))
    src = (fam[0].packed() >> 24).astype(np.uint8) & 0x0f
    assert len(src) >= max(ALIGN_LENGTHS)
    rng = np.random.default_rng(503)
    qms = []
    for L in ALIGN_LENGTHS:
        t = ALIGN_TAILS[L]
        piece = src[len(src) - (L - t):]
        qms.append(np.concatenate([piece, rng.choice([1, 2, 4, 8], size=t).astype(np.uint8)]))
    sc = dict(fs_weight=0.0, mismatch_score=-3.0)   # (every node weighs the same: a short piece has no better place)
    out = []
    for ins in (0, 1):
        out.append(Case("load-align-ragged-ins%d" % ins, refs.width, [fam] * len(qms), qms, insertion=ins, **sc))
        for L, m in zip(ALIGN_LENGTHS, qms):
            out.append(Case("load-align-L%d-ins%d" % (L, ins), refs.width, [fam], [m], insertion=ins, **sc))
    return out


def cases_overhang_clamps():
    """A family that occupies the first and the last columns of the alignment, queries that overhang it on both sides by
    more bases than there are columns: the attached overhang is clamped to column 0 at the tail and to width - 1 at
    the head (both in the walk's mirrored columns); attach, remove, edge."""
    refs = synth.make_refs(40, length=200, width=400, seed=504, long_del_prob=0.0, del_rate=0.0)
    cs = util.cseqs_from_refs(refs)
    rng = np.random.default_rng(505)
    fam = [cs[i] for i in range(8)]
    qms = []
    for i in range(3):
        m = (refs.seq(i) >> 24).astype(np.uint8) & 0x0f
        qms.append(np.concatenate([rng.choice([1, 2, 4, 8], size=40 + 30 * i).astype(np.uint8), m,
                                   rng.choice([1, 2, 4, 8], size=50 + 20 * i).astype(np.uint8)]))
    qms.append((refs.seq(3) >> 24).astype(np.uint8) & 0x0f)    # (no overhang: its columns reach width - 1 on their own)
    return [Case("overhang-clamps-%s" % n, refs.width, [fam] * len(qms), qms, overhang=oh, lowercase=lc, mismatch_score=-3.0)
            for n, oh, lc in (("attach", 0, 2), ("remove", 1, 0), ("edge", 2, 2))]


def cases_capacity():
    """One launch with queries of 4095, 4096 and 4097 bases (overhang = attach: n_out is the query's length) and two short
    ones, against a 23S-shaped reference: the device assembles up to 4096 bases."""
    refs = synth.make_refs(6, length=4400, width=35200, seed=321, n_clades=2)
    cs = util.cseqs_from_refs(refs)
    src = (refs.seq(2) >> 24).astype(np.uint8) & 0x0f
    assert len(src) >= 4200
    fam = [cs[0]]
    qms = [src[50:50 + 4095], src[60:60 + 4096], src[40:40 + 4097], src[1000:1150], src[3000:3300]]
    return [Case("capacity", refs.width, [fam] * len(qms), qms)]


def cases_grid_tail():
    """65 and 130 short queries in one launch: the last wave of the lane walk's grid is partly empty."""
    w = world_small()
    refs, qs = w[0], w[1]
    fams = [_fam_of(w, qi) for qi in range(4)]
    rng = np.random.default_rng(506)
    out = []
    for n in (65, 130):
        fl, qms = [], []
        for i in range(n):
            m = qs.seq(i % 4) & 0x0f
            lo = int(rng.integers(0, len(m) - 70))
            fl.append(fams[i % 4])
            qms.append(m[lo:lo + int(rng.integers(20, 70))])
        out.append(Case("grid-tail-%d" % n, refs.width, fl, qms))
    return out


@functools.lru_cache(maxsize=None)
def _world_700():
    refs = synth.make_refs(200, length=700, width=5000, seed=507, amb_rate=0.01)
    qs = synth.make_queries(refs, 6, seed=508)
    cs = util.cseqs_from_refs(refs)
    return refs, qs, cs, po.Index(cs, k=10)


def cases_pruned_plane():
    """600 to 700-base queries under two-strip and three-strip geometries, the row skip's guess left alone, bold (0.97)
    and impossible (2: every query is swept again): the walk runs over a plane with rows nobody swept."""
    w = _world_700()
    refs, qs = w[0], w[1]
    fams = [_fam_of(w, qi) for qi in range(qs.n)]
    qms = [qs.seq(qi) for qi in range(qs.n)]
    variants = [dict(geom=g, rho=r) for g in ("128,8", "192,4") for r in (None, "0.97", "2")]
    a = Case("pruned-plane", refs.width, fams, qms, variants=variants)
    # (128,4 = 512 columns: queries cut to fit)
    b = Case("pruned-plane-512", refs.width, fams, [m[:500] for m in qms],
             variants=[dict(geom="128,4", rho=r) for r in (None, "0.97", "2")])
    return [a, b]


def cases_partial():
    """800-base windows of 16S queries at the alignment's start, in its middle and at its end: the alignment begins and
    ends somewhere inside the DAG."""
    refs = world_16s()[0]
    cs, idx = world_16s()[2], world_16s()[3]
    out = []
    for frac in (0.0, 0.3, 0.46):
        qs = synth.make_queries(refs, 2, seed=73, window=(frac, 800))
        fams = []
        for qi in range(qs.n):
            ids, _, _ = idx.famfinder(util.query_cseq(qs, qi), po.ff_opts(fs_min_len=100))
            assert len(ids)
            fams.append([cs[i] for i in ids])
        out.append(Case("partial-%s" % frac, refs.width, fams, [qs.seq(qi) for qi in range(qs.n)]))
    # the first and the last 800 bases of full-length queries with junk before / behind them: the walk stops at a source
    # with query bases left, and starts at a sink in an inner column
    w = world_16s()
    qs = w[1]
    rng = np.random.default_rng(509)
    junk = lambda n: rng.choice([1, 2, 4, 8], size=n).astype(np.uint8)  # noqa: E731
    qms = [np.concatenate([junk(25), qs.seq(4)[:800]]), np.concatenate([qs.seq(5)[-800:], junk(25)]),
           np.concatenate([junk(10), qs.seq(6), junk(40)])]
    out.append(Case("partial-overhang", refs.width, [_fam_of(w, 4), _fam_of(w, 5), _fam_of(w, 6)], qms, lowercase=2))
    return out


DIRECTED = dict(insertion_scan=cases_insertion_scan, insertion_col0=cases_insertion_col0, row_jump=cases_row_jump,
                many_predecessors=cases_many_predecessors, load_alignment=cases_load_alignment,
                overhang_clamps=cases_overhang_clamps, capacity=cases_capacity, grid_tail=cases_grid_tail,
                pruned_plane=cases_pruned_plane, partial=cases_partial)


@functools.lru_cache(maxsize=None)
def group(name):
    """[(case, reference(case))] of "matrix" or of one directed edge, computed once per process."""
    cases = cases_matrix() if name == "matrix" else DIRECTED[name]()
    return [(c, reference(c)) for c in cases]


# ---------------------------------------------------------------- fuzz

def fuzz_case(seed):
    """The world, family and scoring draws of test_mesh_plane_fuzz (util.fuzz_*), then 3 to 8 queries per launch, each a
    piece of a member, mutated, with a spliced-in run (0 / 5 / 40 bases) and a cut-out run (0 / 10 / 80); overhang,
    lowercase and positional weights at random; every fourth seed a profile batch (--fs-no-graph)."""
    rng, pick, refs, cs, usable = util.fuzz_world(seed)
    fam = util.fuzz_family(rng, pick, cs, usable)
    qms = []
    for _ in range(int(rng.integers(3, 9))):
        m = util.fuzz_query(rng, pick, refs, usable)
        cut = int(pick([0, 10, 80]))
        if cut and len(m) > cut + 20:
            m = _cut(m, int(rng.integers(5, len(m) - cut - 5)), cut)
        ins = int(pick([0, 5, 40]))
        if ins and len(m) > 12:
            m = _splice(m, int(rng.integers(5, len(m) - 5)), ins, rng)
        if rng.integers(0, 4) == 0:
            m = m | (rng.random(len(m)) < 0.2).astype(np.uint8) * 16
        qms.append(m.astype(np.uint8))
    knobs, opts = util.fuzz_knobs_and_scoring(rng, pick, refs, max(len(m) for m in qms))
    opts["overhang"] = int(pick([0, 1, 2]))
    opts["lowercase"] = int(pick([0, 1, 2]))
    if seed % 4 == 3:
        opts["fs_no_graph"] = 1
        opts.pop("weights", None)     # (scoring_scheme_profile takes no positional weights)
    return Case("fuzz-%d" % seed, refs.width, [fam] * len(qms), qms, variants=[knobs], **opts)
