"""The inputs of the auto-filter tests (famfinder --auto-filter-field / --auto-filter-threshold and the device entries
that take a positional weight vector PER QUERY, sina_hip_align_graphs_wsets / sina_hip_align_families_wsets), shared by
tests/test_autofilter_cpu.py (which pins them and asserts that every case reaches the edge it is there for) and
tests/test_gpu_autofilter.py (which runs them on the device).  Everything here is CPU work: synth + the oracle."""
import functools

import numpy as np

from oracle import pyoracle as po
from sina_amd import synth
from tests import util, walk_cases as wc

# ---------------------------------------------------------------- the vote, restated

def vote(filter_names, field_texts, prefix, threshold):
    """src/famfinder.cpp:403-428: index of the chosen filter, or -1.  A relative's text is prefix + ":" + field; a filter
    counts the texts that start with its name, whatever the case; only a strictly larger count displaces the best; the
    best is taken iff its count exceeds relatives * threshold, the product computed in float."""
    best, best_n = -1, 0
    for x, name in enumerate(filter_names):
        n = sum(1 for f in field_texts if (prefix + ":" + f).lower().startswith(name.lower()))
        if n > best_n:
            best, best_n = x, n
    return best if np.float32(best_n) > np.float32(len(field_texts)) * np.float32(threshold) else -1


# ---------------------------------------------------------------- weight sets on `small`

N_SETS = 3
SET_PATTERN = (0, 1, 2, 2, 1, 0)       # repeated over the queries: the first and the last set are both used
CLAMP = 37                              # the vectors end this many columns before the alignment does
SPLICE_LONG = 230                       # bases spliced into one query: more than 512 bases, a second strip of B = 8
SPLICE_END = 40                         # ... and into another near its end: a long insertion (extension weights)
GEOMS = (None, "128,8")                 # the launch's own geometry, and two strips of 512 columns


@functools.lru_cache(maxsize=None)
def weight_vectors():
    """[N_SETS, width - CLAMP]: three positional weight vectors from different seeds.  They are shorter than the
    alignment: the nodes in the last columns read the vector's last entry (the clamp), each inside its own vector."""
    width = wc.world_small()[0].width
    return np.stack([np.random.default_rng(700 + s).uniform(0.2, 1.5, size=width - CLAMP).astype(np.float32)
                     for s in range(N_SETS)])


@functools.lru_cache(maxsize=None)
def graph_queries():
    """(families, query masks, set ids): the 12 queries of `small`, one more with SPLICE_LONG bases spliced in mid-query
    and one with SPLICE_END bases spliced in near its end."""
    w = wc.world_small()
    qs = w[1]
    rng = np.random.default_rng(701)
    fams = [wc._fam_of(w, qi) for qi in range(qs.n)]
    qms = [qs.seq(qi) for qi in range(qs.n)]
    fams += [fams[3], fams[7]]
    qms += [wc._splice(qs.seq(3), 150, SPLICE_LONG, rng), wc._splice(qs.seq(7), len(qs.seq(7)) - 30, SPLICE_END, rng)]
    sets = [SET_PATTERN[i % len(SET_PATTERN)] for i in range(len(qms))]
    return fams, qms, sets


def _per_set_reference(fams, qms, sets, width, **opts):
    """The plain walk of every query under ITS set's weights: one walk_cases.Case per set holding that set's queries,
    walk_cases.reference() of each, put back into the queries' order."""
    W = weight_vectors()
    out = [None] * len(qms)
    for s in range(N_SETS):
        mine = [i for i in range(len(qms)) if sets[i] == s]
        if not mine:
            continue
        case = wc.Case("set%d" % s, width, [fams[i] for i in mine], [qms[i] for i in mine], weights=W[s], **opts)
        for i, r in zip(mine, wc.reference(case)):
            out[i] = r
    return out


@functools.lru_cache(maxsize=None)
def graphs_reference(insertion):
    """(case, per-query reference) of the graphs route under --insertion shift (0) / forbid (1).  The case carries the
    launch's options (its `weights` are unused: the launch takes weight_vectors())."""
    fams, qms, sets = graph_queries()
    width = wc.world_small()[0].width
    case = wc.Case("wsets-ins%d" % insertion, width, fams, qms, insertion=insertion)
    return case, _per_set_reference(fams, qms, sets, width, insertion=insertion)


@functools.lru_cache(maxsize=None)
def family_queries():
    """(family ids, query masks, set ids) of the families route: the queries of `small` cut to different lengths, so that
    the launch's dispatch order (decreasing work) is not the input order; query 1 is query 0 again -- the same bases
    against the same ordered family, which share one DAG -- under another set."""
    refs, qs, cs, idx = wc.world_small()
    ids, qms = [], []
    for qi in range(qs.n):
        f, _, _ = idx.famfinder(util.query_cseq(qs, qi))
        m = qs.seq(qi)
        cut = (len(m), 90, 200, 140)[qi % 4]
        ids.append(np.asarray(f, np.uint32))
        qms.append(m[:cut])
    ids[1], qms[1] = ids[0], qms[0]
    sets = [SET_PATTERN[i % len(SET_PATTERN)] for i in range(len(qms))]
    assert sets[0] != sets[1]
    return ids, qms, sets


@functools.lru_cache(maxsize=None)
def families_reference():
    ids, qms, sets = family_queries()
    refs, _, cs, _ = wc.world_small()
    shared = {}
    fams = [shared.setdefault(f.tobytes(), [cs[int(i)] for i in f]) for f in ids]   # (one list per ordered family: one DAG)
    case = wc.Case("wsets-families", refs.width, fams, qms)
    return case, _per_set_reference(fams, qms, sets, refs.width)


# ---------------------------------------------------------------- the pipeline world

TAX_FIELD = "tax_slv"
# registration order matters: "pv:Archaea;Eury" and "pv:Archaea" both count a euryarchaeon, the first registered stays.
# No filter is called "pv" (or "pv:all"): with --filter pv a query without a match falls back to the simple scheme.
FILTER_NAMES = ("pv:Bacteria", "pv:Archaea;Eury", "pv:Archaea", "other:all")
N_BACTERIA, N_EURY, N_CREN = 290, 85, 25      # 400 references; fewer crenarchaea than a family has members
PIPE_GROUPS = (0, 1, 2, 0, 2, 1, 0, 2, 0, 1, 0, 0)   # the group of the reference each of the 12 queries is derived from


def _concat(parts):
    off = [np.zeros(1, np.int64)]
    for p in parts:
        off.append(p.off[1:] + off[-1][-1])
    return synth.RefSet(ab=np.concatenate([p.ab for p in parts]), off=np.concatenate(off), width=parts[0].width)


@functools.lru_cache(maxsize=None)
def world_pipeline():
    """400 references of 300 bases, width 3000, in three unrelated groups (each its own random ancestor) with a taxonomy
    path per reference -- every 29th reference has none --, four filters of the alignment's width, and 12 queries: (refs,
    queries, cseqs, oracle index, {ref id: taxonomy}, [(filter name, weights)])."""
    kw = dict(length=300, width=3000, amb_rate=0.01, lower_rate=0.02)
    refs = _concat([synth.make_refs(N_BACTERIA, seed=801, **kw), synth.make_refs(N_EURY, seed=802, n_clades=4, **kw),
                    synth.make_refs(N_CREN, seed=803, n_clades=2, **kw)])
    assert refs.n == 400
    tax = {}
    for i in range(refs.n):
        if i % 29 == 28:
            continue
        tax[i] = ("Bacteria;Proteobacteria;g%d" % (i % 7) if i < N_BACTERIA else
                  "Archaea;Euryarchaeota;g%d" % (i % 5) if i < N_BACTERIA + N_EURY else "archaea;Crenarchaeota")
    filters = [(n, np.random.default_rng(810 + x).uniform(0.3, 1.4, size=refs.width).astype(np.float32))
               for x, n in enumerate(FILTER_NAMES)]
    # (make_queries draws its sources itself: 400 derived queries, of which the first few of every group are taken)
    allq = synth.make_queries(refs, refs.n, seed=804, amb_rate=0.01, lower_rate=0.05)
    group = np.where(allq.src < N_BACTERIA, 0, np.where(allq.src < N_BACTERIA + N_EURY, 1, 2))
    of = [list(np.flatnonzero(group == g)) for g in range(3)]
    qs = synth.pick_queries(allq, [of[g].pop(0) for g in PIPE_GROUPS])
    cs = util.cseqs_from_refs(refs)
    return refs, qs, cs, po.Index(cs, k=10), tax, filters


PIPE_FF = dict(fs_min_len=100, fs_full_len=250)
PIPE_FF_HOST = {"fs-min-len": 100, "fs-full-len": 250, "auto-filter-field": TAX_FIELD}


@functools.lru_cache(maxsize=None)
def pipeline_expected(prefix, threshold=0.8):
    """Per query of the pipeline world under --filter `prefix` (may be empty): the oracle's famfinder, the restated vote
    over the family it leaves, the oracle's align() with the chosen filter's weights -- dict(status, ids, sc, chosen
    (index or -1), filter (name, "" for the simple scheme), packed, head, tail, qual, log)."""
    refs, qs, cs, idx, tax, filters = world_pipeline()
    names = [n for n, _ in filters]
    default = None
    for x, n in enumerate(names):     # src/famfinder.cpp:386-395: the last of the three spellings
        if prefix and n in (prefix, prefix + ":ALL", prefix + ":all"):
            default = x
    out = []
    for qi in range(qs.n):
        q = util.query_cseq(qs, qi, upper=False)
        ids, sc, fflog = idx.famfinder(q, po.ff_opts(**PIPE_FF))
        chosen = vote(names, [tax.get(int(i), "") for i in ids], prefix, threshold)
        auto = "autofilter: %s;" % names[chosen] if chosen >= 0 else "autofilter: no match;"
        use = chosen if chosen >= 0 else default
        if len(ids) == 0:
            out.append(dict(status=2, ids=ids, sc=sc, chosen=chosen, filter="", log=auto + fflog))
            continue
        r = po.align([cs[i] for i in ids], q, po.align_opts(weights=None if use is None else filters[use][1]))
        r.update(ids=ids, sc=sc, chosen=chosen, log=auto + fflog + r["log"],
                 filter=(names[use] if use is not None and r["status"] == 0 else ""))
        out.append(r)
    return out
