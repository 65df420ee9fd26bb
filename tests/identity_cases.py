"""The inputs of the in-place family identity's tests (family_identity_kernel), shared by
tests/test_identity_cpu.py (which asserts that they are worth running) and tests/test_gpu_identity.py (which runs them
through sina_hip_align_families / _families_wsets / _profiles).  Everything here is CPU work: synth, the oracle, the
plain comparison walk of tests/compare_ref.py.

A launch is a small store, queries (iupac masks as the device gets them) with their families as lists of reference
ids, one set of aligner options.  Its expected rows: where the device must assemble the query (walk_cases decides
that, from the plain walk), compare_ref -- optimistic, no lower-case filter -- of the oracle's finished sequence
(oracle.align(...)["packed"]) against every family member, the overlap score in numpy float32, the maximum's bits and
the number of members whose denominator is not 0; two zeros elsewhere."""
import functools

import numpy as np

from oracle import pyoracle as po
from sina_amd import synth
from tests import compare_ref as cr, util, walk_cases as wc


class Launch:
    """refs: the store (a synth.RefSet); fam_ids: per query a list of reference ids, in family order -- queries that
    share a list OBJECT share a family; qmasks: per query uint8; opts: walk_cases.Case options; sets / weight_vectors:
    the launch is one of sina_hip_align_families_wsets (a vector per query)."""

    def __init__(self, name, refs, fam_ids, qmasks, sets=None, weight_vectors=None, **opts):
        self.name, self.refs, self.fam_ids = name, refs, fam_ids
        self.qmasks = [np.asarray(m, np.uint8) for m in qmasks]
        self.sets, self.weight_vectors, self.opts = sets, weight_vectors, opts

    @property
    def width(self):
        return self.refs.width

    def packed_families(self):
        foff = np.zeros(len(self.fam_ids) + 1, np.uint64)
        foff[1:] = np.cumsum([len(f) for f in self.fam_ids])
        return np.concatenate([np.asarray(f, np.uint32) for f in self.fam_ids]), foff

    def packed_queries(self):
        qoff = np.zeros(len(self.qmasks) + 1, np.uint64)
        qoff[1:] = np.cumsum([len(m) for m in self.qmasks])
        return np.concatenate(self.qmasks), qoff


def add_refs(refs, extra):
    """The store with hand-made references (packed words, ascending columns) behind its own."""
    ab = np.concatenate([refs.ab] + [np.asarray(e, np.uint32) for e in extra])
    off = np.concatenate([refs.off, refs.off[-1] + np.cumsum([len(e) for e in extra])]).astype(np.int64)
    return synth.RefSet(ab=ab, off=off, width=refs.width)


def score_bits(counts):
    """(float32 bits of match / (match + mismatch + only_a + only_b), True), or (0, False) where the denominator is 0."""
    _, _, oa, ob, match, mismatch = counts
    denom = match + mismatch + oa + ob
    if denom == 0:
        return 0, False
    return int(np.asarray(np.float32(match) / np.float32(denom), np.float32).view(np.uint32)), True


def row_of(packed, members):
    """The expected row of a finished sequence against its family's members (packed words each): (best bits, number
    scored, index of the first member that has the best score or -1, the members' bits or None)."""
    bits = [score_bits(cr.compare_ref(packed, m, 0, False)) for m in members]
    scored = [b for b, ok in bits if ok]
    best = max(scored) if scored else 0      # (scores are not negative: the order of the bits is the order of the floats)
    first = next((i for i, (b, ok) in enumerate(bits) if ok and b == best), -1)
    return best, len(scored), first, [b if ok else None for b, ok in bits]


def _cseq(name, masks):
    m = np.asarray(masks, np.uint8)
    return po.Cseq.from_packed(name, np.arange(len(m), dtype=np.uint32) | (m.astype(np.uint32) << 24), len(m))


@functools.lru_cache(maxsize=None)
def _cseqs(refs_id):
    return util.cseqs_from_refs(_REFS[refs_id])


_REFS = {}


def _walk_case(launch, which, weights):
    """The walk_cases.Case of the launch's queries `which` under one weight vector (or none)."""
    refs = launch.refs
    _REFS[id(refs)] = refs
    cs = _cseqs(id(refs))
    fams = {}
    for q in which:
        if id(launch.fam_ids[q]) not in fams:
            fams[id(launch.fam_ids[q])] = [cs[int(i)] for i in launch.fam_ids[q]]
    return wc.Case(launch.name, refs.width, [fams[id(launch.fam_ids[q])] for q in which], [launch.qmasks[q] for q in which],
                   weights=weights, **launch.opts)


def reference(launch):
    """Per query: dict(must, packed -- oracle.align's finished sequence --, idty -- the oracle's own --, row = (bits,
    scored), first, member_bits, walk_packed -- backtrack()'s finished sequence)."""
    nq = len(launch.qmasks)
    out = [None] * nq
    groups = [(None, list(range(nq)))] if launch.sets is None else \
        [(launch.weight_vectors[s], [q for q in range(nq) if launch.sets[q] == s]) for s in range(len(launch.weight_vectors))]
    for weights, which in groups:
        if not which:
            continue
        case = _walk_case(launch, which, weights)
        ref = wc.reference(case)
        for x, q in enumerate(which):
            fam = case.fams[x]
            orc = po.align(fam, _cseq("q%d" % q, launch.qmasks[q]), case.oracle_opts())
            assert orc["status"] == 0, (launch.name, q, orc["log"])
            d = dict(must=ref[x]["must"], packed=orc["packed"], idty=orc["idty"], walk_packed=ref[x]["orc"]["packed"])
            best, scored, first, bits = row_of(orc["packed"], [launch.refs.seq(int(i)) for i in launch.fam_ids[q]])
            d["row"] = (best, scored) if d["must"] else (0, 0)
            d["full_row"], d["first"], d["member_bits"] = (best, scored), first, bits
            out[q] = d
    return out


def rows(ref):
    return np.array([r["row"] for r in ref], np.uint32).reshape(len(ref), 2)


# ---------------------------------------------------------------- the worlds

@functools.lru_cache(maxsize=None)
def world():
    """160 references of about 300 bases in 3200 columns (a base every tenth column), a few ambiguity codes and
    lower-case bases."""
    return synth.make_refs(160, length=300, width=3200, seed=611, amb_rate=0.01, lower_rate=0.02)


def _family(rng, refs, src, F):
    """F distinct reference ids with `src` among them, and not first where there is a choice."""
    others = rng.choice(np.setdiff1d(np.arange(refs.n), [src]), size=F - 1, replace=False)
    ids = [int(x) for x in others]
    ids.insert(int(rng.integers(1, F)) if F > 1 else 0, int(src))
    return ids


def _queries(refs, n, seed, **kw):
    qs = synth.make_queries(refs, n, seed=seed, **kw)
    return qs, [qs.seq(i) for i in range(qs.n)]


FAMILY_SIZES = (1, 3, 4, 5, 8, 9, 40, 128)


def launches_family_sizes():
    """Fewer members than waves, exactly as many, one more, two whole passes, two passes plus one, the default fs-max,
    the device route's maximum."""
    refs = world()
    rng = np.random.default_rng(612)
    qs, qms = _queries(refs, len(FAMILY_SIZES), 613, amb_rate=0.01, lower_rate=0.05)
    fams = [_family(rng, refs, int(qs.src[i]), F) for i, F in enumerate(FAMILY_SIZES)]
    return [Launch("family-sizes", refs, fams, qms)]


def launches_shared_family():
    """Queries 0 and 2 have the same ordered family, query 1 another: the chunk's lists are packed.  Query 3 has query
    0's members in another order: a DAG of its own, the same identity."""
    refs = world()
    rng = np.random.default_rng(614)
    qs, qms = _queries(refs, 3, 615)
    fam_a = _family(rng, refs, int(qs.src[0]), 6)
    fam_b = _family(rng, refs, int(qs.src[1]), 9)
    return [Launch("shared-family", refs, [fam_a, fam_b, fam_a, fam_a[::-1]], [qms[0], qms[1], qms[2], qms[0]])]


def launches_member_outside():
    """A windowed query (the first 110 bases of its source) whose family holds a fragment lying wholly to the right of
    the query's last aligned column: that member's denominator is 0."""
    base = world()
    qs, qms = _queries(base, 2, 616, window=(0.0, 110))
    frag = [base.seq(int(qs.src[i]))[-40:] for i in range(2)]
    refs = add_refs(base, frag)
    rng = np.random.default_rng(617)
    # (the other members have bases where the query lies -- a reference with a long deletion there would have no score
    # either: the fragment is the only one, the second word is F - 1)
    dense = [i for i in range(base.n) if int(((base.seq(i) & 0xFFFFFF) < 1100).sum()) >= 90]
    fams = []
    for i in range(2):
        src = int(qs.src[i])
        f = [src] + [int(x) for x in rng.choice(np.setdiff1d(dense, [src]), size=3, replace=False)]
        f.insert(2, base.n + i)
        fams.append(f[::-1])
    return [Launch("member-outside", refs, fams, qms)]


@functools.lru_cache(maxsize=None)
def _world_iupac():
    return synth.make_refs(60, length=300, width=3200, seed=618, amb_rate=0.3, lower_rate=0.3)


def launches_iupac_and_case():
    """A third of the bases an ambiguity code, a third lower case, in the members and in the queries; --lowercase=original
    keeps the queries' case in the finished words (calc-idty does not filter it)."""
    refs = _world_iupac()
    rng = np.random.default_rng(619)
    qs, qms = _queries(refs, 4, 620, amb_rate=0.2, lower_rate=0.3)
    fams = [_family(rng, refs, int(qs.src[i]), F) for i, F in enumerate((5, 7, 2, 12))]
    return [Launch("iupac-case-lc%d" % lc, refs, fams, qms, lowercase=lc) for lc in (1, 0)]


def launches_overhang():
    """Windowed queries with junk on both sides against families cut to columns 800 .. 2200 (hand-made references: the
    family ends inside the alignment, so the junk overhangs it and has columns to go to) under attach, remove and
    edge: the finished words differ between the three, and under remove there are fewer of them than query bases."""
    base = world()
    rng = np.random.default_rng(621)
    qs, qms = _queries(base, 3, 622)
    junk = lambda n: rng.choice([1, 2, 4, 8], size=n).astype(np.uint8)  # noqa: E731
    qms = [np.concatenate([junk(12 + 3 * i), m[85:215], junk(9 + 2 * i)]) for i, m in enumerate(qms)]
    whole = [_family(rng, base, int(qs.src[i]), 5 + i) for i in range(3)]
    cut_of, extra = {}, []
    for f in whole:
        for i in f:
            if i not in cut_of:
                ab = base.seq(i)
                cut_of[i] = base.n + len(extra)
                extra.append(ab[((ab & 0xFFFFFF) >= 800) & ((ab & 0xFFFFFF) <= 2200)])
    refs = add_refs(base, extra)
    fams = [[cut_of[i] for i in f] for f in whole]
    return [Launch("overhang-%s" % n, refs, fams, qms, overhang=oh, lowercase=lc, mismatch_score=-3.0)
            for n, oh, lc in (("attach", 0, 2), ("remove", 1, 0), ("edge", 2, 2))]


def launches_unassembled():
    """Queries with 30 bases spliced in -- nine free columns lie between two bases of this world: the insertion does not
    fit its gap and the host finishes the query -- mixed with ordinary ones."""
    refs = world()
    rng = np.random.default_rng(623)
    qs, qms = _queries(refs, 5, 624)
    for i in (1, 3):
        qms[i] = np.concatenate([qms[i][:140], rng.choice([1, 2, 4, 8], size=30).astype(np.uint8), qms[i][140:]])
    fams = [_family(rng, refs, int(qs.src[i]), 4 + i) for i in range(5)]
    return [Launch("unassembled", refs, fams, qms)]


RANGES_KNOBS = (dict(dp_range_q=3), dict(fam_chunk_q=4), dict(dp_range_q=3, fam_chunk_q=4))


def launches_ranges():
    """Ten queries for SINA_HIP_TEST=dp_range_q=3 and fam_chunk_q=4 (chunks 0-3, 4-7, 8-9): queries 3 and 4 share a
    family across the chunk boundary, 5 and 7 one inside a chunk."""
    refs = world()
    rng = np.random.default_rng(625)
    qs, qms = _queries(refs, 10, 626, window=(0.2, 150))
    fams = [_family(rng, refs, int(qs.src[i]), 3 + (i * 5) % 11) for i in range(10)]
    fams[4] = fams[3]
    fams[7] = fams[5]
    return [Launch("ranges", refs, fams, qms)]


def launches_widest():
    """524 288 columns -- the widest alignment of the family routes, the largest LDS table --, two members of 60 bases
    and a query of 50."""
    rng = np.random.default_rng(627)
    width = 524288
    cols = np.sort(rng.choice(np.arange(width // 64), size=60, replace=False)).astype(np.uint32) * 64 + 7
    cols[-1] = width - 1
    m0 = rng.choice([1, 2, 4, 8], size=60).astype(np.uint32)
    m1 = m0.copy()
    m1[::7] = rng.choice([1, 2, 4, 8], size=len(m1[::7]))
    refs = synth.RefSet(ab=np.concatenate([cols | (m0 << 24), cols[2:] | (m1[2:] << 24)]).astype(np.uint32),
                        off=np.array([0, 60, 118], np.int64), width=width)
    q = m1[8:58].astype(np.uint8)
    q[::9] = rng.choice([1, 2, 4, 8], size=len(q[::9]))
    return [Launch("widest", refs, [[0, 1]], [q])]


def launches_profiles():
    """--fs-no-graph: sina_hip_align_profiles builds the families as profiles; the shared-family launch again."""
    l = launches_shared_family()[0]
    return [Launch("profiles", l.refs, l.fam_ids, l.qmasks, fs_no_graph=1)]


def launches_wsets():
    """sina_hip_align_families_wsets: two positional weight vectors, chosen per query."""
    refs = world()
    rng = np.random.default_rng(628)
    W = [rng.uniform(0.2, 1.5, size=refs.width).astype(np.float32) for _ in range(2)]
    qs, qms = _queries(refs, 4, 629)
    fams = [_family(rng, refs, int(qs.src[i]), 4 + 2 * i) for i in range(4)]
    return [Launch("wsets", refs, fams, qms, sets=np.array([0, 1, 1, 0], np.uint32), weight_vectors=W)]


GROUPS = dict(family_sizes=launches_family_sizes, shared_family=launches_shared_family, member_outside=launches_member_outside,
              iupac_and_case=launches_iupac_and_case, overhang=launches_overhang, unassembled=launches_unassembled,
              ranges=launches_ranges, widest=launches_widest, profiles=launches_profiles, wsets=launches_wsets)
# the cases of the issue; `profiles` and `wsets` carry the other two entries
NAMED = ("family_sizes", "shared_family", "member_outside", "iupac_and_case", "overhang", "unassembled", "ranges", "widest")


@functools.lru_cache(maxsize=None)
def group(name):
    """[(launch, reference(launch))] of a group, computed once per process and left unchanged."""
    return [(l, reference(l)) for l in GROUPS[name]()]
