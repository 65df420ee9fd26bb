"""The inputs of the in-place ranking's tests (rank_assembled_kernel), shared by
tests/test_search_inplace_cpu.py (which asserts that they are worth running) and tests/test_gpu_search_inplace.py (which
runs them through the align entries with sina_hip_align_rank on).  Everything here is CPU work: synth, the oracle, the
plain comparison walk of tests/compare_ref.py and the ranking of tests/rank_ref.py.

A launch is one of tests/identity_cases.py -- a small store, queries with their families, aligner options -- with the
search stage's settings beside it.  Its expected row of a query, [n, flags, 64 ids, 64 score bits]:
  1. the oracle's k-mer search (Index.find) over the INPUT bases gives the top min(kmer_candidates, n_refs) ids;
  2. compare_ref walks the oracle's finished sequence (oracle.align(...)["packed"]) against each of them;
  3. rank_ref.rank_query scores and orders them by the cover rule and the names ref0, ref1, ... (byte-wise: ref10 < ref2).
A query the device must not rank -- one it does not assemble, or one that lost a base -- has an all-zero row."""
import functools

import numpy as np

from oracle import pyoracle as po
from tests import compare_ref as cr, identity_cases as ic, rank_cases as rc, rank_ref, shift_cases as sc, util, walk_cases as wc

ROW_WORDS = 130
MAX_BEST = 64
RANKED, NAN = 2, 1


class Launch(ic.Launch):
    """search: dict(k, cands, n_best, cover, rule, flc); assemble: 1 or 2; knobs: the SINA_HIP_TEST settings the GPU test
    runs the launch under; align_key: launches that share it share queries, families and aligner options, i.e. their
    alignments (computed once)."""

    def __init__(self, name, base, align_key=None, assemble=1, knobs=None, k=10, cands=1000, n_best=10, cover="query", rule=0,
                 flc=False):
        ic.Launch.__init__(self, name, base.refs, base.fam_ids, base.qmasks, base.sets, base.weight_vectors, **base.opts)
        self.align_key = align_key or base.name
        self.assemble, self.knobs = assemble, dict(knobs or {})
        self.search = dict(k=k, cands=cands, n_best=n_best, cover=cover, rule=rule, flc=flc)
        self.names = rc._names(self.refs.n)

    @property
    def stride(self):
        return min(self.search["cands"], self.refs.n)


_STORES, _ALIGNED = {}, {}


def _index(refs, k):
    key = (id(refs), k)
    if key not in _STORES:
        cs = util.cseqs_from_refs(refs)
        _STORES[key] = (refs, cs, po.Index(cs, k=k))
    return _STORES[key][1:]


def _alignments(launch):
    """Per query (must, packed): whether the device must assemble it, and the oracle's finished sequence."""
    key = (launch.align_key, launch.assemble)
    if key in _ALIGNED:
        return _ALIGNED[key]
    if launch.assemble == 1:
        out = [(bool(r["must"]), r["packed"]) for r in ic.reference(launch)]
    else:           # assemble = 2: the shifted-insertion world, every query of which the device finishes (tests/shift_cases.py)
        cs = _index(launch.refs, launch.search["k"])[0]
        opts = wc.Case("opts", launch.width, [], [], **launch.opts).oracle_opts()
        opts.realign = 1
        out = []
        for q, m in enumerate(launch.qmasks):
            al = po.align([cs[int(i)] for i in launch.fam_ids[q]], ic._cseq("q%d" % q, m), opts)
            assert al["status"] == 0, (launch.name, q)
            out.append((True, al["packed"]))
    _ALIGNED[key] = out
    return out


def candidates(launch, q):
    """The k-mer search's ids for query q's input bases, as the oracle finds them."""
    _, idx = _index(launch.refs, launch.search["k"])
    ids, _ = idx.find(ic._cseq("q%d" % q, launch.qmasks[q]), launch.stride)
    return np.asarray(ids, np.uint32)


def reference(launch):
    """Per query: dict(must, packed, kept -- no base was dropped --, ranked, cand, row [130], full -- the row it would
    have if it were ranked)."""
    s = launch.search
    name_rank = rank_ref.name_order(launch.names)
    out = []
    for q, (must, packed) in enumerate(_alignments(launch)):
        cand = candidates(launch, q)
        counters = [cr.compare_ref(packed, launch.refs.seq(int(i)), s["rule"], s["flc"]) for i in cand]
        ids, bits, flag = rank_ref.rank_query(counters, cand, name_rank, s["cover"], s["n_best"])
        full = np.zeros(ROW_WORDS, np.uint32)
        full[0], full[1] = len(ids), RANKED | (NAN if flag else 0)
        full[2:2 + len(ids)] = ids
        full[2 + MAX_BEST:2 + MAX_BEST + len(bits)] = bits
        kept = len(packed) == len(launch.qmasks[q])
        ranked = must and kept
        out.append(dict(must=must, packed=packed, kept=kept, ranked=ranked, cand=cand, full=full,
                        row=full if ranked else np.zeros(ROW_WORDS, np.uint32)))
    return out


def rows(ref):
    return np.stack([r["row"] for r in ref]).astype(np.uint32)


# ---------------------------------------------------------------- the launches

N_BEST = 10
CANDS = (1, 3, 4, 5, N_BEST - 1, N_BEST, N_BEST + 1, 1000)


@functools.lru_cache(maxsize=None)
def _base_four():
    """Four mutated queries of identity_cases' world with families of 4 to 10 members."""
    refs = ic.world()
    rng = np.random.default_rng(701)
    qs, qms = ic._queries(refs, 4, 702, amb_rate=0.01, lower_rate=0.05)
    fams = [ic._family(rng, refs, int(qs.src[i]), 4 + 2 * i) for i in range(4)]
    return ic.Launch("four", refs, fams, qms)


def launches_cands():
    """kmer_candidates of 1, N - 1, N, N + 1, fewer than, as many as and one more than the waves of a workgroup, and
    more than there are references (the search's max clamps to n_refs)."""
    return [Launch("cands-%d" % c, _base_four(), cands=c, n_best=N_BEST) for c in CANDS]


def launches_n_best():
    """max_result of 1, 10 and 64, every reference a candidate."""
    return [Launch("best-%d" % n, _base_four(), n_best=n) for n in (1, 10, 64)]


def launches_covers():
    """Each cover rule once, the iupac rules and the lower-case filter spread over them."""
    return [Launch("cover-%s" % c, _base_four(), cands=40, cover=c, rule=i % 3, flc=bool(i % 2)) for i, c in enumerate(rank_ref.COVERS)]


def launches_no_hit():
    """A query with an N at every ninth base has no 10-mer without one: every reference scores 0, and the search --
    which always fills its rows, zero scores included, largest ids first -- hands over the last references of the
    store.  (So a ranked row with n = 0 cannot come out of a search: max is at least 1.)  The query beside it is an
    ordinary one."""
    base = _base_four()
    m = base.qmasks[1].copy()
    m[4::9] = 15
    return [Launch("no-hit", ic.Launch("no-hit", base.refs, [base.fam_ids[1], base.fam_ids[0]], [m, base.qmasks[0]]), cands=12)]


def launches_tie():
    """Reference 7 and seven copies of it behind the store (ids 160 .. 166) score alike against a query derived from
    it; max_result cuts the tie after three of the eight.  By name, descending, ref7 comes before ref166, ref165; by
    id it would come last."""
    base = ic.world()
    src = 7
    refs = ic.add_refs(base, [base.seq(src)] * 7)
    rng = np.random.default_rng(703)
    m = ((base.seq(src) >> 24) & 0x0f).astype(np.uint8)
    sub = rng.random(len(m)) < 0.04
    m[sub] = rng.choice([1, 2, 4, 8], size=int(sub.sum()))
    fam = ic._family(rng, base, src, 5)
    probe = Launch("tie-probe", ic.Launch("tie", refs, [fam], [m]), n_best=64)
    full = reference(probe)[0]["full"]
    tied = [src] + list(range(160, 167))
    at = [i for i in range(int(full[0])) if int(full[2 + i]) in tied]
    assert len(at) == 8 and at == list(range(at[0], at[0] + 8)) and len({int(full[2 + MAX_BEST + i]) for i in at}) == 1
    return [Launch("tie", ic.Launch("tie", refs, [fam], [m]), n_best=at[0] + 3)]


def launches_nan():
    """A windowed query (the first 110 bases of its source, mutated) and, behind the store, its first 40 bases laid
    into the columns of the source's last 40: a k-mer candidate that shares no column with the query -- under the overlap rule
    its denominator is 0 and the row carries bit 0."""
    base = ic.world()
    qs, qms = ic._queries(base, 2, 616, window=(0.0, 110))
    extra = []
    for i in range(2):
        ab = base.seq(int(qs.src[i]))
        extra.append(((qms[i][:40].astype(np.uint32) & 0x0f) << 24 | (ab[-40:] & 0xFFFFFF)).astype(np.uint32))
    refs = ic.add_refs(base, extra)
    rng = np.random.default_rng(704)
    fams = [ic._family(rng, base, int(qs.src[i]), 4) for i in range(2)]
    return [Launch("nan-overlap", ic.Launch("nan", refs, fams, qms), cover="overlap")]


def launches_overhang_remove():
    """identity_cases' --overhang remove launch: the junk on both sides is dropped, n_out < L -- the aligned sequence's
    k-mers are not the input's, the device leaves the query to the host."""
    base = [l for l in ic.launches_overhang() if l.name == "overhang-remove"][0]
    return [Launch("overhang-remove", base)]


def launches_unassembled():
    """identity_cases' launch with two queries the host finishes (assemble = 1): their rows stay zero."""
    return [Launch("unassembled", ic.launches_unassembled()[0])]


@functools.lru_cache(maxsize=None)
def _shift_base():
    w = sc.dp_world()
    fams = [[int(x) for x in w["fam_ids"][int(w["fam_off"][q]):int(w["fam_off"][q + 1])]] for q in range(len(w["want"]))]
    qms = [w["qmask"][int(w["qoff"][q]):int(w["qoff"][q + 1])] for q in range(len(fams))]
    return ic.Launch("shifted", w["refs"], fams, qms, lowercase=2)


def launches_shifted():
    """shift_cases' block-layout world with assemble = 2: insertions that shift their neighbours, finished on the
    device and ranked -- without and with the lower-case filter (--lowercase unaligned lower-cases the shifted bases)."""
    return [Launch("shifted-flc%d" % f, _shift_base(), assemble=2, flc=bool(f), cover="all") for f in (0, 1)]


RANGES_KNOBS = (dict(dp_range_q=3), dict(rank_chunk=16), dict(dp_range_q=3, rank_chunk=16))


def launches_ranges():
    """identity_cases' ten queries under dp_range_q=3 (four launch ranges: rows of the call's candidates 3, 6 and 9
    queries in), rank_chunk=16 (160 candidates in ten chunks, the merge launch) and both."""
    base = ic.launches_ranges()[0]
    return [Launch("ranges", base)] + [Launch("ranges-%s" % "-".join(sorted(k)), base, align_key="ranges", knobs=k) for k in RANGES_KNOBS]


def launches_profiles():
    return [Launch("profiles", ic.launches_profiles()[0], cover="all")]


def launches_wsets():
    return [Launch("wsets", ic.launches_wsets()[0], cover="target")]


def launches_graphs():
    """sina_hip_align_graphs: the shared-family launch, its DAGs built by the oracle."""
    return [Launch("graphs", ic.launches_shared_family()[0])]


GROUPS = dict(cands=launches_cands, n_best=launches_n_best, covers=launches_covers, no_hit=launches_no_hit, tie=launches_tie,
              nan=launches_nan, overhang_remove=launches_overhang_remove, unassembled=launches_unassembled,
              shifted=launches_shifted, ranges=launches_ranges, profiles=launches_profiles, wsets=launches_wsets,
              graphs=launches_graphs)
NAMED = ("cands", "n_best", "covers", "no_hit", "tie", "nan", "overhang_remove", "unassembled", "shifted", "ranges")
OTHER_ENTRIES = ("profiles", "wsets", "graphs")


@functools.lru_cache(maxsize=None)
def group(name):
    """[(launch, reference(launch))] of a group, computed once per process and left unchanged."""
    return [(l, reference(l)) for l in GROUPS[name]()]
