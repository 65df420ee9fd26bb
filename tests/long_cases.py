"""The inputs of the long-query tests, shared by tests/test_long_cpu.py (which pins them to the oracle and asserts
that every case reaches the edge it is there for) and tests/test_gpu_long.py (which runs them through
sina_hip_kmer_topk_any / sina_hip_kmer_scores_any and the pipeline).  A case is a reference world -- references, k,
fast / no-fast --, the queries of one batch and the `max` values to search with; the expected results are the
oracle's (Index.find, Index.scores), computed once per process.  Everything here is CPU work."""
import functools

import numpy as np

from oracle import pyoracle as po
from sina_amd import capi, synth
from tests import util

C = capi.KMER_LONG_CHUNK          # windows (by the index of their last base) per chunk of the long count kernel
FAST_MAX = capi.MAX_QUERY_LEN     # longest query of the fast count kernel
LONG_MAX = capi.MAX_LONG_QUERY_LEN
K = 10
N_MASK = 15
SEAMS = [m * C for m in range(1, LONG_MAX // C + 1) if m * C < LONG_MAX]


def _packed(masks, first_col=0):
    m = np.asarray(masks, np.uint32)
    return ((first_col + np.arange(len(m), dtype=np.uint32)) | (m << 24)).astype(np.uint32)


def _refset(seqs, width):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return synth.RefSet(ab=np.concatenate(seqs), off=off, width=width)


def _bases_of(refs, i):
    return ((refs.seq(i) >> 24) & 0x0f).astype(np.uint8)


def concat_query(refs, length, seed, sub=0.01):
    """`length` bases: references drawn at random, one after the other, with a few substitutions."""
    rng = np.random.default_rng(seed)
    parts, n = [], 0
    while n < length:
        parts.append(_bases_of(refs, int(rng.integers(0, refs.n))))
        n += len(parts[-1])
    m = np.concatenate(parts)[:length].copy()
    mut = rng.random(length) < sub
    m[mut] = synth.CODE_TO_MASK[rng.integers(0, 4, size=int(mut.sum()))]
    return m


# ---------------------------------------------------------------- worlds

BLOCK_LEN, BLOCK_REPEATS, N_TIED = 5000, 6, 4


@functools.lru_cache(maxsize=None)
def block():
    return synth.CODE_TO_MASK[np.random.default_rng(4101).integers(0, 4, size=BLOCK_LEN)]


@functools.lru_cache(maxsize=None)
def world(name):
    """(references, k, nofast).  "main": 5000 references of 200 bases (more than the select kernel's 4096) and behind
    them the special ones of the multiplicity case -- one that contains the 5000-base block, N_TIED identical ones that
    hold the same 300 bases of it.  "full": 50 short references and one of 32767 random bases, no-fast.
    "tiles-<k>-<fast|nofast>": the 70 000 short references of tests/test_gpu_scale.py (three reference tiles, posting
    lists longer than 1/64 of the references)."""
    if name == "main":
        refs = synth.make_refs(5000, length=200, width=BLOCK_LEN + 8, seed=4100, n_clades=8)
        special = [_packed(block())] + [_packed(block()[1200:1500], 1200) for _ in range(N_TIED)]
        return _refset([refs.seq(i) for i in range(refs.n)] + special, refs.width), K, False
    if name == "full":
        refs = synth.make_refs(50, length=200, width=LONG_MAX + 8, seed=4200, n_clades=2)
        return _refset([refs.seq(i) for i in range(refs.n)] + [_packed(full_bases())], refs.width), K, True
    kind, k, mode = name.split("-")
    assert kind == "tiles"
    return synth.make_refs(70000, length=200, width=2000, seed=5, n_clades=6), int(k), mode == "nofast"


@functools.lru_cache(maxsize=None)
def full_bases():
    return synth.CODE_TO_MASK[np.random.default_rng(4201).integers(0, 4, size=LONG_MAX)]


@functools.lru_cache(maxsize=None)
def oracle_index(wname):
    refs, k, nofast = world(wname)
    return po.Index(util.cseqs_from_refs(refs), k=k, nofast=nofast)


@functools.lru_cache(maxsize=None)
def oracle_csr(wname):
    """(offsets, ids) of the oracle's index (slow on a large world: the tiles worlds use posting_lengths)."""
    return oracle_index(wname).csr()


def posting_lengths(refs, k, fast, kmers):
    """In how many references each of `kmers` occurs as a k-mer of K(reference) -- the length of its posting list --
    from the packed references alone."""
    m = ((refs.ab >> 24) & 0x0f).astype(np.int64)
    code = np.full(len(m), -1, np.int64)
    for c in range(4):
        code[m == (1 << c)] = c
    n = len(m)
    owner = np.repeat(np.arange(refs.n, dtype=np.int64), np.diff(refs.off))
    v = np.zeros(n - k + 1, np.int64)         # v[i]: the window of bases i .. i + k - 1
    ok = np.ones(n - k + 1, bool)
    for x in range(k):
        cx = code[x:n - k + 1 + x]
        ok &= cx >= 0
        v = (v << 2) | np.maximum(cx, 0)
    end = np.arange(k - 1, n)
    ok &= owner[end] == owner[end - (k - 1)]                          # inside one reference
    ok &= np.append(owner[end[:-1] + 1] == owner[end[:-1]], False)    # not on its last base
    if fast:
        ok &= (v >> (2 * (k - 1))) == 0
    ok &= np.isin(v, kmers)
    pairs = np.unique(v[ok] * refs.n + owner[end][ok])
    vals, cnt = np.unique(pairs // refs.n, return_counts=True)
    out = np.zeros(len(kmers), np.int64)
    at = np.searchsorted(vals, kmers)
    hit = (at < len(vals)) & (vals[np.minimum(at, len(vals) - 1)] == kmers) if len(vals) else np.zeros(len(kmers), bool)
    out[hit] = cnt[at[hit]]
    return out


# ---------------------------------------------------------------- cases

class Case:
    def __init__(self, name, wname, qmasks, maxes=(1, 41)):
        self.name, self.world, self.maxes = name, wname, tuple(maxes)
        self.qmasks = [np.ascontiguousarray(m, np.uint8) for m in qmasks]

    @property
    def qmask(self):
        return np.concatenate(self.qmasks)

    @property
    def qoff(self):
        off = np.zeros(len(self.qmasks) + 1, np.uint64)
        off[1:] = np.cumsum([len(m) for m in self.qmasks])
        return off

    def is_long(self):
        return [len(m) > FAST_MAX for m in self.qmasks]


def seam_lengths():
    """10240 (stays on the fast kernel), 10241, every length k + 1 either side of every seam, 32767."""
    ls = {FAST_MAX, FAST_MAX + 1, LONG_MAX}
    for s in SEAMS:
        ls.update(range(s - (K + 1), s + (K + 1) + 1))
    return sorted(ls)


@functools.lru_cache(maxsize=None)
def lengths():
    refs = world("main")[0]
    whole = concat_query(refs, LONG_MAX, seed=4110)
    # (prefixes of one sequence: what a length adds or drops at its end is what differs between neighbours)
    return Case("lengths", "main", [whole[:n] for n in seam_lengths()])


@functools.lru_cache(maxsize=None)
def seam_n():
    """One N at each offset -k .. +k around the first seam: 2k + 1 queries in one batch."""
    refs = world("main")[0]
    base = concat_query(refs, C + 300, seed=4120, sub=0.0)
    qs = []
    for d in range(-K, K + 1):
        m = base.copy()
        m[C + d] = N_MASK
        qs.append(m)
    return Case("seam-n", "main", qs)


@functools.lru_cache(maxsize=None)
def multiplicity():
    return Case("multiplicity", "main", [np.tile(block(), BLOCK_REPEATS)], maxes=(1, 3, 41))


@functools.lru_cache(maxsize=None)
def fullest():
    return Case("fullest", "full", [full_bases()], maxes=(1, 41))


def too_long():
    """One base more than the k-mer search takes."""
    return np.concatenate([full_bases(), full_bases()[:1]])


TILE_WORLDS = ("tiles-10-fast", "tiles-10-nofast", "tiles-8-fast", "tiles-8-nofast")


@functools.lru_cache(maxsize=None)
def tiles(wname):
    refs = world(wname)[0]
    return Case(wname, wname, [concat_query(refs, 2 * C + 37, seed=4130, sub=0.005)], maxes=(1, 41, 410))


@functools.lru_cache(maxsize=None)
def degenerate():
    return Case("degenerate", "main", [np.full(C + 1760, N_MASK, np.uint8)])


@functools.lru_cache(maxsize=None)
def mixed():
    refs = world("main")[0]
    short = synth.make_queries(refs, 5, seed=4140)
    qs = []
    for i, n in enumerate((FAST_MAX + 1, 2 * C + 5, LONG_MAX, FAST_MAX + 700)):
        qs.append(short.seq(i))
        qs.append(concat_query(refs, n, seed=4141 + i))
    qs.append(short.seq(4))
    qs.insert(3, concat_query(refs, FAST_MAX, seed=4150))    # (the longest query of the fast kernel among them)
    return Case("mixed", "main", qs, maxes=(1, 41, 410, 4096))


def kmer_cases():
    return [lengths(), seam_n(), multiplicity(), fullest(), degenerate(), mixed()] + [tiles(w) for w in TILE_WORLDS]


def case(name):
    return next(c for c in kmer_cases() if c.name == name)


def as_cseq(mask):
    m = np.asarray(mask, np.uint8) & 0x0f
    return po.Cseq.from_packed("q", _packed(m), len(m))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's answers for a case: per query its score vector and, per max, (ids, scores) of Index.find."""
    c = case(name)
    idx = oracle_index(c.world)
    out = []
    for m in c.qmasks:
        q = as_cseq(m)
        out.append(dict(scores=idx.scores(q), find={mx: idx.find(q, mx) for mx in c.maxes}))
    return out


# ---------------------------------------------------------------- the chunk arithmetic, as a plain model

def windows(mask, k, fast):
    """K(query) of csrc/kmer.hip's header comment: value of the k-mer ending on base e, or -1, for every e."""
    m = np.asarray(mask, np.int64) & 0x0f
    n = len(m)
    out = np.full(n, -1, np.int64)
    code = np.full(n, -1, np.int64)
    for c in range(4):
        code[m == (1 << c)] = c
    for e in range(k - 1, n - 1):                 # (the window ending on the last base is never produced)
        w = code[e + 1 - k:e + 1]
        if (w < 0).any():
            continue
        v = 0
        for x in w:
            v = (v << 2) | int(x)
        if fast and (v >> (2 * (k - 1))) != 0:
            continue
        out[e] = v
    return out


def chunk_windows(mask, k, fast, chunk=None):
    """The same, the way the long count kernel goes about it: per chunk of `chunk` window ends e0 .. e1 - 1 only the
    bases b0 .. e1 - 1 are looked at, b0 = e0 - (k - 1) (or 0)."""
    chunk = chunk or C
    m = np.asarray(mask, np.uint8)
    n = len(m)
    out = np.full(n, -1, np.int64)
    for e0 in range(0, n, chunk):
        e1 = min(n, e0 + chunk)
        b0 = e0 + 1 - k if e0 + 1 >= k else 0
        local = m[b0:e1]
        for e in range(e0, e1):
            le, llen = e - b0, n - b0               # kmer_at(qb, len - b0, e - b0, ...)
            if le + 1 < k or le + 2 > llen:
                continue
            w = local[le + 1 - k:le + 1] & 0x0f
            if any(bin(int(x)).count("1") != 1 for x in w):
                continue
            v = 0
            for x in w:
                v = (v << 2) | (int(x).bit_length() - 1)
            if fast and (v >> (2 * (k - 1))) != 0:
                continue
            out[e] = v
    return out


# ---------------------------------------------------------------- the pipeline cases

PIPE_FF = {"fs-min-len": 100, "fs-full-len": 250, "fs-min": 8, "fs-max": 8}
PIPE_OFF = dict(fs_min_len=100, fs_full_len=250, fs_min=8, fs_max=8)
PIPE_LONG_AT = (1, 4, 6)       # where the long queries sit in the batch

COMPLEMENT = np.zeros(32, np.uint8)
for _m in range(32):   # A<->T/U, G<->C, case bit kept
    COMPLEMENT[_m] = ((_m & 2) << 1) | ((_m & 4) >> 1) | ((_m & 1) << 3) | ((_m & 8) >> 3) | (_m & 16)


@functools.lru_cache(maxsize=None)
def pipe_world():
    """260 references of about 11 000 bases in two clades (the store tests/test_gpu_pipeline.py builds for its
    9000-base queries, longer), with their oracle cseqs and index."""
    refs = synth.make_refs(260, length=11000, width=36000, seed=4301, n_clades=2, long_del_prob=0.0)
    cs = util.cseqs_from_refs(refs)
    return refs, cs, po.Index(cs, k=K)


@functools.lru_cache(maxsize=None)
def pipe_queries():
    """Eight queries: three whole-length ones (more than 10 240 bases) among five 1200-base windows."""
    refs = pipe_world()[0]
    long_q = synth.make_queries(refs, len(PIPE_LONG_AT), seed=4302)
    short_q = synth.make_queries(refs, 5, seed=4303, window=(0.3, 1200))
    masks, li, si = [], 0, 0
    for i in range(8):
        if i in PIPE_LONG_AT:
            masks.append(long_q.seq(li))
            li += 1
        else:
            masks.append(short_q.seq(si))
            si += 1
    off = np.zeros(len(masks) + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in masks])
    return synth.QuerySet(mask=np.concatenate(masks), off=off, src=np.zeros(len(masks), np.int64))


@functools.lru_cache(maxsize=None)
def pipe_expected(insertion):
    """The oracle's run of every pipeline query (famfinder, then align) under --insertion=shift (0) / forbid (1)."""
    refs, cs, idx = pipe_world()
    qs = pipe_queries()
    out = []
    for qi in range(qs.n):
        q = util.query_cseq(qs, qi, upper=False)
        ids, sc, fflog = idx.famfinder(q, po.ff_opts(**PIPE_OFF))
        if len(ids) == 0:
            out.append(dict(status=2, log=fflog, ids=ids, sc=sc))
            continue
        r = po.align([cs[i] for i in ids], q, po.align_opts(insertion=insertion))
        r["log"] = fflog + r["log"]
        r["ids"], r["sc"] = ids, sc
        out.append(r)
    return out
