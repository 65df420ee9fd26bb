"""The case table of the scoring gates (tests/test_gates_cpu.py, tests/test_gpu_gates.py, tests/golden/
make_gate_vectors.py) and a plain model of the gates themselves.

Several host-side comparisons on the scoring parameters and the node weights decide which DP kernel a launch runs and
whether the certified row skip and the scout pass take part (sina_amd/csrc/dp_plan.h: dp_kernel_kind, prune_plan_for,
scout_allowed; common.h: dp_below_init).  The table walks the parameter space ACROSS those comparisons -- signs, zeros,
either side of every threshold -- on the smallest shape at which the kernels can still go wrong: a family DAG of a few
hundred rows, a query of two strips whose second strip is mostly padding.  expected_path() says, from the documented
rules alone and without calling the library, what a launch of a case must run.

Out of scope: non-finite scoring parameters and fs_weight == -1 (node weights 1 / (fs_weight + 1): infinite).  The
reference itself produces infinite planes there; there is nothing to compare with."""
import functools

import numpy as np

from oracle import pyoracle as po
from sina_amd import synth

F32 = np.float32

# ---- the project's own constants (common.h: kPruneMaxStep, dp_below_init; dp_plan.h: prune_plan_for)
PRUNE_MAX_STEP = 250
BELOW_INIT_LIMIT = F32(900000.0)
PRUNE_EXACT_UNITS = 1 << 23

KERNELS = ("none", "simple", "simple_skip", "generic_below", "generic", "weighted", "forbid", "weighted_forbid")

# ---- worlds, families, queries
# name -> (reference length, alignment width, seed, family size, query length, geometries SINA_HIP_TEST=geom=)
# "64,8": a single strip -- no skip, no scout; "128,4": two strips, the second holds 28 real columns; "128,8": two
# strips of 512 columns for the longer query of the second world.
FAMILIES = {
    "A12": dict(length=300, width=2400, seed=4100, F=12, qlen=284, geoms=("64,8", "128,4")),
    "A1": dict(length=300, width=2400, seed=4100, F=1, qlen=284, geoms=("64,8", "128,4")),
    "B12": dict(length=600, width=4800, seed=4200, F=12, qlen=560, geoms=("128,8",)),
}


@functools.lru_cache(maxsize=None)
def world(length, width, seed):
    """60 references with ambiguity codes, lower case and long deletions (as util.mesh_case_inputs makes small cases)."""
    return synth.make_refs(60, length=length, width=width, seed=seed, n_clades=3, amb_rate=0.03, lower_rate=0.05,
                           long_del_prob=0.3, del_rate=0.03, ins_rate=0.02)


@functools.lru_cache(maxsize=None)
def family(name):
    """(refs, ids of the family's members, the query's iupac masks): the members are the first F references long enough
    to cut the query from; the query is the first member with a 30-base deletion, a 30-base insertion and 8 % of
    its bases mutated, cut to the family's query length."""
    f = FAMILIES[name]
    refs = world(f["length"], f["width"], f["seed"])
    sizes = np.diff(refs.off)
    usable = [int(i) for i in np.flatnonzero(sizes >= f["qlen"] + 4)]
    ids = np.asarray(usable[:f["F"]], np.uint32)
    assert len(ids) == f["F"]
    rng = np.random.default_rng(f["seed"] + 7)
    src = ((refs.seq(int(ids[0])) >> 24) & 0x0f).astype(np.uint8)
    a = len(src) // 3
    b = 2 * len(src) // 3
    ins = rng.choice(np.array([1, 2, 4, 8], np.uint8), size=30)
    qm = np.concatenate([src[:a], src[a + 30:b], ins, src[b:]])[:f["qlen"]].copy()
    mut = rng.random(len(qm)) < 0.08
    qm[mut] = rng.choice(np.array([1, 2, 4, 8, 15, 3], np.uint8), size=int(mut.sum()))
    assert len(qm) == f["qlen"]
    return refs, ids, qm


def family_cseqs(name):
    refs, ids, _ = family(name)
    return [po.Cseq.from_packed("ref%d" % i, refs.seq(int(i)), refs.width) for i in ids]


def query_cseq(name):
    qm = family(name)[2]
    return po.Cseq.from_packed("q", np.arange(len(qm), dtype=np.uint32) | (qm.astype(np.uint32) << 24), len(qm))


@functools.lru_cache(maxsize=None)
def dag_facts(name, fs_weight):
    """(nodes, largest node weight, smallest node weight) of the family's DAG under fs_weight."""
    g = po.mseq_build(family_cseqs(name), fs_weight)
    return int(g["n"]), float(g["weight"].max()), float(g["weight"].min())


# ---- positional weights: plain, a fifth zeroed, a tenth negated
WEIGHT_VARIANTS = ("plain", "zeros", "neg")


@functools.lru_cache(maxsize=None)
def positional_weights(name, variant):
    refs, _, qm = family(name)
    rng = np.random.default_rng(FAMILIES[name]["seed"] + 11)
    w = rng.uniform(0.2, 2.0, size=refs.width + len(qm) + 8).astype(np.float32)
    pick = rng.random(len(w))
    if variant == "zeros":
        w[pick < 0.2] = 0.0
    elif variant == "neg":
        w[pick < 0.1] *= F32(-1.0)
    else:
        assert variant == "plain"
    w.setflags(write=False)
    return w


# ---- float32 restatements of the gate arithmetic (common.h, dp_plan.h), used to FIND the threshold pairs and by the model
def gain_units(w, kappa64):
    """prune_gain_units: w * kappa64 rounded up to a whole unit, plus one unit of margin."""
    x = F32(F32(w) * F32(kappa64))
    u = int(x)
    if F32(u) < x:
        u += 1
    return u + 1


def kappa64_of(match, mismatch):
    kappa = max(F32(0.0), F32(match), F32(mismatch))
    return F32(F32(F32(64.0) * F32(1.0001)) * kappa)


def below_init_sum(n, gp, gpe):
    return F32(F32(F32(F32(1.0) + F32(F32(F32(n) * F32(gp)) * F32(1.01))) + F32(gp)) + F32(gpe))


def below_init(n, gp, gpe):
    return bool(F32(gp) >= 0 and F32(gpe) >= 0 and below_init_sum(n, gp, gpe) < BELOW_INIT_LIMIT)


def _last_true(pred, lo, hi):
    """The largest float32 x in [lo, hi] with pred(x), pred being true at lo, false at hi and monotone: bisection on
    the bit patterns (positive floats order like their bits)."""
    lo_b, hi_b = int(F32(lo).view(np.uint32)), int(F32(hi).view(np.uint32))
    assert pred(F32(lo)) and not pred(F32(hi))
    while hi_b - lo_b > 1:
        mid = (lo_b + hi_b) // 2
        if pred(np.uint32(mid).view(np.float32)):
            lo_b = mid
        else:
            hi_b = mid
    return np.uint32(lo_b).view(np.float32)


# ---- scoring sets (match, mismatch, gap, gapext, fs_weight); w: also run with positional weights
BASE_SETS = [
    ("default", (2, -1, 5, 2, 1), True),
    ("mismatch_gains", (2, 1, 5, 2, 1), True),
    ("both_cost", (-1, -2, 5, 2, 1), True),               # kappa == 0
    ("mismatch_above_match", (-1, 2, 5, 2, 1), False),
    ("all_zero_scores", (0, 0, 5, 2, 1), False),          # kappa == 0, every diagonal step ties
    ("free_gaps", (2, -1, 0, 0, 1), True),
    ("free_open", (2, -1, 0, 2, 1), False),
    ("extend_above_open", (2, -1, 2, 3, 1), True),
    ("negative_gaps", (2, -1, -1, -0.5, 1), False),
    ("free_extend", (2, -1, 5, 0, 1), False),
    ("negative_extend", (2, -1, 5, -1, 1), True),
    ("fs_weight_-0.5", (2, -1, 5, 2, -0.5), False),
    ("fs_weight_-2", (2, -1, 5, 2, -2), True),            # negative node weights
    ("fs_weight_5", (2, -1, 5, 2, 5), False),             # amax > 250
    ("tiny", (1e-3, -1e-3, 2e-3, 1e-3, 1), False),
    ("large", (200, -100, 500, 200, 1), True),
    ("open_1200", (2, -1, 1200, 2, 1), True),
    ("gaps_1e30", (2, -1, 1e30, 1e30, 1), False),
]


@functools.lru_cache(maxsize=None)
def threshold_sets(name):
    """Either side of each float comparison, from the family's own largest node weight and node count."""
    n, wmax, _ = dag_facts(name, 1.0)
    # amax == 250 and amax == 251: the largest match score that still gives 250 units, and the float above it
    m250 = _last_true(lambda m: gain_units(wmax, kappa64_of(m, -1)) <= PRUNE_MAX_STEP, 1.0, 100.0)
    m251 = np.nextafter(m250, F32(np.inf))
    assert gain_units(wmax, kappa64_of(m250, -1)) == 250 and gain_units(wmax, kappa64_of(m251, -1)) == 251
    # dp_below_init's sum just under and just over 900000
    g_in = _last_true(lambda g: below_init(n, g, 2), 5.0, 1e6)
    g_out = np.nextafter(g_in, F32(np.inf))
    assert below_init(n, g_in, 2) and not below_init(n, g_out, 2)
    return [
        ("amax_250", (float(m250), -1, 5, 2, 1), False),
        ("amax_251", (float(m251), -1, 5, 2, 1), False),
        ("below_init_in", (2, -1, float(g_in), 2, 1), False),
        ("below_init_out", (2, -1, float(g_out), 2, 1), False),
        ("extend_equals_open", (2, -1, 5, 5, 1), False),
        ("extend_just_above_open", (2, -1, 5, float(np.nextafter(F32(5), F32(np.inf))), 1), False),
    ]


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case: dict(id, fam, set, match, mismatch, gap, gapext, fs_weight, forbid, wvar).  Every scoring set runs
    unweighted under both insertion rules; those marked w also weighted under both rules with the three weight vectors
    (the first world's two families; the second world's longer query runs the unweighted sets)."""
    cases = []
    for fam in FAMILIES:
        for sname, sc, w in BASE_SETS + threshold_sets(fam):
            variants = [None] + (list(WEIGHT_VARIANTS) if (w and fam != "B12") else [])
            for wvar in variants:
                for forbid in (False, True):
                    cid = "%s-%s-%s-%s" % (fam, sname, wvar or "unweighted", "forbid" if forbid else "shift")
                    cases.append(dict(id=cid, fam=fam, set=sname, match=float(sc[0]), mismatch=float(sc[1]), gap=float(sc[2]),
                                      gapext=float(sc[3]), fs_weight=float(sc[4]), forbid=forbid, wvar=wvar))
    return tuple(cases)


def case_by_id(cid):
    return next(c for c in all_cases() if c["id"] == cid)


def case_weights(case):
    return positional_weights(case["fam"], case["wvar"]) if case["wvar"] else None


def oracle_opts(case, **kw):
    return po.align_opts(weights=case_weights(case), match_score=case["match"], mismatch_score=case["mismatch"],
                         gap_penalty=case["gap"], gap_ext_penalty=case["gapext"], fs_weight=case["fs_weight"],
                         insertion=1 if case["forbid"] else 0, **kw)


def device_params(ctx, case, **kw):
    return ctx.params(weights=case_weights(case), match_score=case["match"], mismatch_score=case["mismatch"],
                      gap_penalty=case["gap"], gap_ext_penalty=case["gapext"], fs_weight=case["fs_weight"],
                      insertion=1 if case["forbid"] else 0, **kw)


# ---- the model of the gates
def expected_path(case, entry, geom, generic=False, prune=True, rho_fixed=False):
    """What a launch of `case` must run, from the documented rules.
    entry: "debug_mesh" / "align_graphs" (caller-built DAG: the weights' range is the DAG's own, no chain to scout along)
    or "align_families" (device-built DAG: the range is what fs_weight allows, 1/(w+1) + w at most and, for a negative
    fs_weight, possibly below 0; the family's first member is the scout's chain).
    geom: "T,B" as forced; generic: SINA_HIP_TEST=generic=1; prune: False for debug_mesh(prune=False); rho_fixed:
    SINA_HIP_TEST=rho=.  Returns dict(kernel, skip, prune_step, scout)."""
    T = int(geom.split(",")[0])
    strips = T // 64
    n, wmax, wmin = dag_facts(case["fam"], case["fs_weight"])
    if entry == "align_families":
        fsw = case["fs_weight"]
        wmax = float(F32(1.0 / (float(F32(fsw)) + 1.0) + float(F32(fsw))))
        wmin = 0.0 if fsw >= 0 else -1.0
    weighted, forbid = case["wvar"] is not None, case["forbid"]
    gp, gpe = F32(case["gap"]), F32(case["gapext"])
    binit = (not weighted) and (not forbid) and below_init(n, gp, gpe)
    # prune_plan
    plan_on, amax = False, 0
    kappa = max(F32(0.0), F32(case["match"]), F32(case["mismatch"]))
    if (prune and np.isfinite(wmax) and np.isfinite(wmin) and not weighted and not forbid and gp >= 0 and gpe >= 0
            and wmin >= 0 and np.isfinite(kappa)):
        amax = gain_units(wmax, kappa64_of(case["match"], case["mismatch"]))
        qlen = FAMILIES[case["fam"]]["qlen"]
        plan_on = amax <= PRUNE_MAX_STEP and amax * qlen < PRUNE_EXACT_UNITS and strips > 1
    # launch_tb
    if not weighted and not forbid and binit and gp >= gpe and not generic:
        kernel = "simple_skip" if (plan_on and strips >= 2) else "simple"
    elif not weighted and not forbid:
        kernel = "generic_below" if binit else "generic"
    elif weighted:
        kernel = "weighted_forbid" if forbid else "weighted"
    else:
        kernel = "forbid"
    # choose_bound
    scout = (entry == "align_families" and not weighted and not forbid and plan_on and not rho_fixed and binit and gp >= gpe
             and T > 64 and not generic)
    return dict(kernel=kernel, skip=kernel == "simple_skip", prune_step=amax if plan_on else 0, scout=bool(scout))


def path_cells(graph, cells):
    """The cells the trace-back walk reads on the optimal path of the oracle's planes (src/mesh.h:567-685): the end cell,
    every cell its value_midx / value_sidx lead to, and the cell behind a one-step deletion skip.  [(m, s)]."""
    from tests import walk_ref
    value, vmid, vsid = cells["value"], cells["value_midx"], cells["value_sidx"]
    srcs = set(int(x) for x in graph["src"])
    m, s = walk_ref.end_cell(graph, value)
    out = [(m, s)]
    while s != 0 and m not in srcs:
        snew, mnew = int(vsid[m, s]), int(vmid[m, s])
        m = mnew
        out.append((m, snew))
        if snew != 0 and int(vsid[m, snew]) == snew:
            m = int(vmid[m, snew])
            out.append((m, snew))
        s = snew
    return out
